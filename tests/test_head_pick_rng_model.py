"""The model of the seeded pick's noise (tests/head_pick_rng_model.py) checked without a GPU: Philox4x32-10 against known answers, the
counter mapping, the exactness and range of the noise, the distribution of the model's own samples, and that the cases the GPU tests
run (tests/test_hip_head_pick_rng.py) are decisive on the reference alone."""
import numpy as np
import pytest

import head_pick_model as hm
import head_pick_rng_model as rm

# counter, key -> output (Random123's known answers for philox4x32-10: zeros, ones, digits of pi)
KNOWN = [((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
         ((0xffffffff,) * 4, (0xffffffff,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
         ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), "d16cfe09 94fdcceb 5001e420 24126ea1")]


@pytest.mark.parametrize("counter,key,want", KNOWN, ids=["zeros", "ones", "pi"])
def test_philox_known_answers(counter, key, want):
    got = rm.philox4x32_10(counter, key)
    assert " ".join(f"{int(v):08x}" for v in got) == want
    # the vectorised path: the same counter among others
    many = rm.philox4x32_10(tuple(np.array([1, c, 2], dtype=np.uint64) for c in counter), key)
    assert [int(v[1]) for v in many] == [int(v) for v in got]


def test_counter_mapping():
    seed = 0x0123456789ABCDEF
    key = (seed & rm.MASK32, seed >> 32)
    for offset in (0, 7, (1 << 32) - 1, 1 << 32, (1 << 64) - 1):
        w = rm.words(seed, offset, 11, 5)
        for row, o in ((0, 0), (3, 4), (4, 1), (10, 2)):
            ctr, word = rm.counter_of(row, o, offset)
            assert ctr == (o, row >> 2, offset & rm.MASK32, offset >> 32) and word == row & 3
            assert int(w[row, o]) == int(rm.philox4x32_10(ctr, key)[word])
    # a 64-bit carry: offset 2^32 - 1 -> 2^32 turns (c2, c3) from (ffffffff, 0) into (0, 1)
    assert rm.counter_of(0, 0, (1 << 32) - 1)[0][2:] == (0xffffffff, 0) and rm.counter_of(0, 0, 1 << 32)[0][2:] == (0, 1)
    assert not np.array_equal(rm.words(seed, (1 << 32) - 1, 4, 4), rm.words(seed, 1 << 32, 4, 4))
    # rows given explicitly are the global rows: a slice of a larger call
    assert np.array_equal(rm.words(seed, 7, 3, 9, rows=[64, 65, 66]), rm.words(seed, 7, 67, 9)[64:])
    # the four rows of a group share one evaluation, and different seeds give different words
    assert len({int(v) for v in rm.words(seed, 0, 4, 1)[:, 0]}) == 4
    assert not np.array_equal(rm.words(seed, 0, 4, 4), rm.words(seed + 1, 0, 4, 4))


def test_uniform_is_exact_in_fp32_and_the_range_of_g():
    w = np.array([0, 0x1ff, 0x200, 0xffffffff], dtype=np.uint32)
    u = rm.uniform_from_words(w)
    assert u.tolist() == [2.0 ** -24, 2.0 ** -24, 3 * 2.0 ** -24, 1 - 2.0 ** -24]
    assert np.array_equal(u.astype(np.float32).astype(np.float64), u), "u is not representable in fp32"
    # the steps the device takes in fp32 give the same u: an odd 24-bit integer, then a power of two
    k = (w >> np.uint32(9)).astype(np.uint32)
    u32 = (2 * k + 1).astype(np.float32) * np.float32(2.0 ** -24)
    assert np.array_equal(u32.astype(np.float64), u)
    g = rm.gumbel_from_words(w)
    assert np.isfinite(g).all() and g[0] == g[1] and g[0] == g.min() and g[3] == g.max()
    assert rm.G_MIN < g.min() < rm.G_MIN + 0.01 and rm.G_MAX - 0.01 < g.max() < rm.G_MAX
    # g is monotone in the word: every other word lies between
    ws = np.linspace(0, 0xffffffff, 4097).astype(np.uint32)
    assert (np.diff(rm.gumbel_from_words(ws)) >= 0).all()


@pytest.mark.parametrize("seed", rm.DIST_SEEDS)
def test_model_samples_follow_softmax(seed):
    """m = 8 fixed logits with probabilities over two decades, 4096 rows of ONE call: Pearson's chi-square of the model's tokens
    against softmax stays below the 0.999 quantile at 7 degrees of freedom.  The seeds are crc32 of the case id, fixed in advance:
    a failure is a bug in the mapping."""
    bits, dtype, M, m, n, _, _, inv_t = rm.DIST_CASE
    inp, logits = rm.dist_inputs()
    p = np.exp(logits)
    p /= p.sum()
    assert p.max() / p.min() >= 99 and p.min() * M >= 5
    g = rm.noise(seed, 0, M, m)
    ref = rm.reference(inp, dtype, inv_t, g)
    assert np.array_equal(ref["s"], np.broadcast_to(logits, (M, m))), "the inputs do not give the same logits on every row"
    chi2 = rm.chi_square(ref["token"], logits)
    print(f"seed {seed}: chi-square {chi2:.3f} (bound {rm.CHI2_7_999}), decisive rows {ref['decisive'].mean():.4f}")
    assert chi2 < rm.CHI2_7_999
    assert ref["decisive"].mean() >= 0.9
    # the token through the kernels' merge order is the same argmax
    assert np.array_equal(hm.head_pick(ref["s"], 1.0, g)[0], ref["token"])


def test_cases_cover_the_axes():
    import itertools

    assert len({hm.case_id(c) for c in rm.CASES}) == len(rm.CASES)
    vals = [(c[2], c[3], c[4], (c[0], c[1]), c[5], c[7]) for c in rm.CASES]
    for a, b in itertools.combinations(range(len(rm.AXES)), 2):
        seen = {(v[a], v[b]) for v in vals}
        assert seen == set(itertools.product(rm.AXES[a], rm.AXES[b])), (a, b)
    assert {hm.launch_plan(M)[1][0] for M in rm.MS} == {1, 2, 3, 4} and max(hm.launch_plan(M)[0] for M in rm.MS) == 2
    assert {rm.case_state(c)[1] for c in rm.CASES} == set(rm.OFFSETS)


@pytest.mark.parametrize("case", rm.CASES + [rm.LARGE_VOCAB], ids=hm.case_id)
def test_gpu_cases_are_decisive(case):
    """on the reference alone: at least 90 % of the rows have an fp64 gap above 2 (E1 + Eg)"""
    inp, g, ref, seed, offset = rm.gaussian_case(case)
    assert rm.G_MIN < g.min() and g.max() < rm.G_MAX
    assert ref["Eg"] == 2.0 ** -21 * (1 + np.abs(g).max())
    assert ref["decisive"].mean() >= 0.9, (hm.case_id(case), float(ref["decisive"].mean()))


@pytest.mark.parametrize("case", hm.PADDING_CASES, ids=hm.case_id)
def test_padding_cases_are_decisive(case):
    inp, g, ref, seed, offset = rm.padding_case(case)
    assert float(ref["lse"].max()) < -40 + np.log(case[3])  # (so every logit is below -40)
    # a padding feature that took part with a logit of 0 would win whatever it drew: the best real z stays below its smallest z
    assert float(ref["z"].max()) < rm.G_MIN
    assert ref["decisive"].mean() >= 0.9
