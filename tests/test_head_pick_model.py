"""The arithmetic of csrc/lut_head_pick.hip without a GPU: the numpy fp64 model of its tile and merge steps (tests/head_pick_model.py)
against the definition itself (np.argmax of z, which takes the first maximum, and a plain log-sum-exp) with planted exact ties and
the padding case, the workspace layout and the launch plan against the library's sizer and plan query (pure host code), the
coverage of the shared case list and the condition its seeds have to meet."""
import itertools

import numpy as np
import pytest

import head_pick_model as hm


@pytest.mark.parametrize("M", hm.MS)
@pytest.mark.parametrize("m", hm.OUTS + (1000, 2200))
@pytest.mark.parametrize("with_noise", [False, True])
def test_model_against_brute_force(M, m, with_noise):
    """per-block records, the lane exchanges, tiles, waves, the ascending merge in 64 ranges (m = 128: one block, m = 2200: 18 blocks,
    one per range; tests/test_head_pick_model.py::test_case_seeds_are_decisive runs the 1002 blocks of m = 128256, 16 per range);
    fp64 leaves the orders indistinguishable, so lse must agree to a few ulps and token and score exactly"""
    rng = np.random.default_rng(1000 * M + m + with_noise)
    logits = 4.0 * rng.standard_normal((M, m)) + 3.0 * rng.standard_normal((M, 1))
    logits[0, rng.integers(0, m)] = 60.0  # one dominant feature, wherever it falls
    noise = hm.gumbel(M, m, M + m) if with_noise else None
    for inv_t in hm.INV_TS:
        got, want = hm.head_pick(logits, inv_t, noise), hm.brute_force(logits, inv_t, noise)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
        for g, w, name in zip(got[2:], want[2:], ("lse", "logprob")):
            assert np.abs(g - w).max() <= 64 * np.finfo(np.float64).eps * max(1.0, np.abs(w).max()), name
        assert (got[0] >= 0).all() and (got[0] < m).all()


@pytest.mark.parametrize("m", [128, 300, 2200])
def test_planted_ties_keep_the_smallest_index(m):
    """exact ties inside a tile, across the two tiles of a wave, across waves, across blocks and across merge ranges: the smallest
    index wins, wherever the members lie; integer logits (many accidental ties) against np.argmax"""
    rng = np.random.default_rng(m)
    M = 9
    logits = rng.standard_normal((M, m))
    groups = [(5, 7), (5, 21), (5, 40), (21, 40, 100), (3, m - 1), (40, m // 2, m - 1), (127, m - 1)]
    if m > 133:
        groups += [(5, 21, 40, 133), (133, 5), (127, 128), (m - 2, 133, 21)]
    for g in (g for g in groups if len(set(g)) == len(g)):
        l = logits.copy()
        l[:, list(g)] = 9.0
        token, score, _, _ = hm.head_pick(l)
        assert (token == min(g)).all() and (score == 9.0).all(), g
        noise = np.zeros((M, m), dtype=np.float32)
        noise[:, min(g)] = -1.0  # the smallest member drops out: the next one takes over
        token = hm.head_pick(l, 1.0, noise)[0]
        assert (token == sorted(g)[1]).all(), g
    ints = rng.integers(-3, 4, (64, m)).astype(np.float64)
    halves = rng.integers(-2, 3, (64, m)).astype(np.float32) / 2
    for noise in (None, halves):
        got, want = hm.head_pick(ints, 1.0, noise), hm.brute_force(ints, 1.0, noise)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])


@pytest.mark.parametrize("m", [129, 300])
def test_padding_features_take_no_part(m):
    """every real logit <= -40: a padding feature of the last block counted as a logit of 0 would lift lse by more than 30 and win
    the pick with an index past m"""
    rng = np.random.default_rng(m)
    logits = np.minimum(-48.0 + rng.standard_normal((65, m)), -40.0)
    token, score, lse, logprob = hm.head_pick(logits)
    want = hm.brute_force(logits)
    assert np.array_equal(token, want[0]) and (token < m).all()
    assert np.abs(lse - want[2]).max() <= 1e-12 * 48 and (lse < -40 + np.log(m)).all()
    wrong = hm.head_pick(logits, count_padding=True)
    assert (wrong[2] - lse).min() > 30 and (wrong[0] >= m).all()


@pytest.mark.parametrize("M,m", [(M, m) for M in hm.MS for m in hm.OUTS] + [(5, 128256), (4096, 128256), (4096, 50272)])
def test_workspace_formula_matches_the_layout(M, m):
    """16 + 4 bytes per row and 128-feature block, whatever n and bits are; inside the 32 bytes per row and 32 features the design
    allows; the sizer is host code: no GPU"""
    from ganq_amd import _lib

    _lib.build()
    lay = hm.workspace_layout(M, m)
    T = -(-m // 128)
    assert lay["rec4_offset"] == 0 and lay["reco_offset"] == lay["rec4_bytes"] == 16 * M * T and lay["reco_offset"] % 16 == 0
    assert lay["total"] == lay["reco_offset"] + 4 * M * T
    for n, bits in ((32, 2), (512, 3), (2048, 4)):
        assert _lib.lib().ganq_lut_head_pick_workspace_bytes(M, m, n, bits) == lay["total"]
    assert lay["total"] <= 32 * M * -(-m // 32)
    assert _lib.lib().ganq_lut_head_pick_workspace_bytes(0, m, 32, 4) == 0


@pytest.mark.parametrize("M", hm.MS + (32, 33, 48, 49, 128, 129, 300))
def test_launch_plan(M):
    """one tile launch per 64 rows with RT = ceil(rows / 16) row tiles, one merge launch of ceil(M / 4) workgroups (a wave per row)"""
    import ctypes

    from ganq_amd import _lib

    _lib.build()
    launches, rts, merge_wgs = hm.launch_plan(M)
    assert launches == -(-M // 64) and all(rt == 4 for rt in rts[:-1]) and rts[-1] == -(-(M - 64 * (launches - 1)) // 16)
    for m, n, bits in ((1, 32, 2), (300, 96, 3), (128256, 2048, 4)):
        assert _lib.debug_head_pick_plan(M, m, n, bits) == (launches, -(-m // 128), merge_wgs, rts)
    out = (ctypes.c_int * 3)()
    assert _lib.lib().ganq_debug_head_pick_plan(M, 300, 96, 4, ctypes.cast(out, ctypes.c_void_p), 3) == 0  # no room for RT: none written
    assert list(out) == [launches, 3, merge_wgs]
    assert _lib.lib().ganq_debug_head_pick_plan(M, 300, 96, 4, ctypes.cast(out, ctypes.c_void_p), 2) == -3
    assert _lib.lib().ganq_debug_head_pick_plan(M, 300, 48, 4, ctypes.cast(out, ctypes.c_void_p), 3) == -2
    assert _lib.lib().ganq_debug_head_pick_plan(M, 300, 96, 5, ctypes.cast(out, ctypes.c_void_p), 3) == -2
    assert _lib.lib().ganq_debug_head_pick_plan(0, 300, 96, 4, ctypes.cast(out, ctypes.c_void_p), 3) == -1


def test_case_list_covers_the_axes():
    """every value pair of every two of the seven axes is met by some case"""
    cases = hm.CASES
    assert len(cases) == len(set(cases)) and 30 <= len(cases) <= 48
    as_axes = [(c[2], c[3], c[4], (c[0], c[1]), c[5], c[6], c[7]) for c in cases]
    for a, b in itertools.combinations(range(len(hm.AXES)), 2):
        assert {(c[a], c[b]) for c in as_axes} == set(itertools.product(hm.AXES[a], hm.AXES[b])), (a, b)
    assert hm.LARGE_VOCAB[:5] == (4, "fp16", 5, 128256, 64)


@pytest.mark.parametrize("case", hm.CASES + [hm.LARGE_VOCAB], ids=hm.case_id)
def test_case_seeds_are_decisive(case):
    """the condition the GPU test relies on, from the fp64 reference alone: on at least 90 % of a case's rows the gap between the best
    and the second-best z exceeds 2 E1, so the fp32 argmax has to be the fp64 argmax there; the model agrees with the definition"""
    inp, noise, ref = hm.gaussian_case(case)
    assert hm.decisive_share(ref) >= 0.9
    token, score, lse, _ = hm.head_pick(ref["s"], 1.0, noise)
    assert np.array_equal(token, ref["token"]) and np.array_equal(score, ref["score"])
    assert np.abs(lse - ref["lse"]).max() <= 1e-12 * max(1.0, np.abs(ref["lse"]).max())
