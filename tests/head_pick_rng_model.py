"""A numpy model of the noise the seeded pick of csrc/lut_head_pick.hip draws inside its tile kernel, and the cases its tests share
(tests/test_head_pick_rng_model.py without a GPU, tests/test_hip_head_pick_rng.py on one).  A helper module like
tests/head_pick_model.py, which serves everything after the noise; not a conftest.

The draw (include/ganq_hip.h):
  Philox4x32-10 (Salmon, Moraes, Dror, Shaw, SC'11) with key (seed_lo, seed_hi) and counter (o, row >> 2, offset_lo, offset_hi),
  o the feature and row the global row of x; word `row & 3` of the four results belongs to (row, o).
  w -> k = w >> 9 -> u = (2 k + 1) 2^-24 (exact in fp32, in [2^-24, 1 - 2^-24]) -> E = -log(u) -> g = -log(E).
The model takes both logs in fp64.  The device takes them with the accurate fp32 logf, at most 2 ulp each: E carries a relative error
of 2^-22, which moves g by 2^-22 absolutely, and the second log adds 2^-22 |g|: |g_device - g| <= 2^-22 (1 + |g|); the tests allow
    Eg = 2^-21 (1 + max |g|),
twice that.  A row is decisive where the fp64 gap between its best and second-best z exceeds 2 (E1 + Eg), E1 the bound of
tests/head_pick_model.py::reference on everything but the noise."""
import zlib

import numpy as np

import head_pick_model as hm

M0, M1 = 0xD2511F53, 0xCD9E8D57  # the multipliers of the round
W0, W1 = 0x9E3779B9, 0xBB67AE85  # the Weyl constants the key is bumped by
MASK32 = 0xFFFFFFFF
G_MIN, G_MAX = -2.82, 16.64      # the range of g, as the header states it


def philox4x32_10(counter, key):
    """counter: four arrays (or ints) of 32-bit values, key: two -> four uint32 arrays of their broadcast shape"""
    c = [np.asarray(v, dtype=np.uint64) & np.uint64(MASK32) for v in np.broadcast_arrays(*counter)]
    k0, k1 = (int(v) & MASK32 for v in key)
    lo32 = np.uint64(MASK32)
    s32 = np.uint64(32)
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c[0], np.uint64(M1) * c[2]  # 32 x 32 bits: the product fits 64
        c = [(p1 >> s32) ^ c[1] ^ np.uint64(k0), p1 & lo32, (p0 >> s32) ^ c[3] ^ np.uint64(k1), p0 & lo32]
        k0, k1 = (k0 + W0) & MASK32, (k1 + W1) & MASK32
    return tuple(v.astype(np.uint32) for v in c)


def counter_of(row, o, offset):
    """the counter of element (row, o) under `offset` (a Python int below 2^64) and the index of its word"""
    return (o, row >> 2, offset & MASK32, (offset >> 32) & MASK32), row & 3


def words(seed, offset, M, m, rows=None):
    """uint32 [M, m]: the raw word of every element (rows: the global rows, default 0 .. M - 1)"""
    rows = np.arange(M, dtype=np.int64) if rows is None else np.asarray(rows, dtype=np.int64)
    o = np.arange(m, dtype=np.int64)
    ctr, _ = counter_of(rows[:, None], o[None, :], int(offset))
    out = philox4x32_10(ctr, (int(seed) & MASK32, (int(seed) >> 32) & MASK32))
    sel = (rows & 3)[:, None]
    return np.choose(np.broadcast_to(sel, out[0].shape), out)


def uniform_from_words(w):
    """fp64 u = (2 (w >> 9) + 1) 2^-24: an odd multiple of 2^-24 below 1, so exact in fp32 too"""
    return (2.0 * (np.asarray(w, dtype=np.uint32) >> np.uint32(9)).astype(np.float64) + 1.0) * 2.0 ** -24


def gumbel_from_words(w):
    """fp64 g = -log(-log(u))"""
    return -np.log(-np.log(uniform_from_words(w)))


def noise(seed, offset, M, m):
    """fp64 [M, m]"""
    return gumbel_from_words(words(seed, offset, M, m))


def noise_bound(g):
    """Eg of the module docstring"""
    return 2.0 ** -21 * (1.0 + float(np.abs(g).max()))


def reference(inp, dtype, inv_t, g):
    """tests/head_pick_model.py::reference on the fp64 noise g (not rounded to fp32), with Eg and the decisive rows of the seeded pick"""
    ref = hm.reference(inp, dtype, inv_t, np.asarray(g, dtype=np.float64))
    ref["Eg"] = noise_bound(g)
    ref["decisive"] = ref["gap"] > 2 * (ref["E1"] + ref["Eg"])
    return ref


# ---- the cases of the GPU tests
MS = (1, 16, 17, 33, 49, 64, 65)        # every RT, and the second tile launch
OUTS = (1, 127, 128, 129, 300)
INS = (32, 96, 512)
AXES = (MS, OUTS, INS, hm.PAIRS, (True, False), (1.0, 1 / 0.7))  # M, m, n, (bits, dtype), bias, inv_t
OFFSETS = (0, 7, 1 << 32)


def build_cases():
    """a greedy pairwise cover of the six axes, as hm.build_cases -> tuples (bits, dtype, M, m, n, bias, True, inv_t): the layout of
    the cases of tests/head_pick_model.py, so that its case_id and Gaussian inputs serve"""
    import itertools

    idx = [range(len(a)) for a in AXES]
    combos = np.array(list(itertools.product(*idx)), dtype=np.int64)
    pairs = list(itertools.combinations(range(len(AXES)), 2))
    keys = np.stack([combos[:, a] * 8 + combos[:, b] for a, b in pairs], axis=1)
    open_ = [set((i * 8 + j) for i in range(len(AXES[a])) for j in range(len(AXES[b]))) for a, b in pairs]
    cases = []
    while any(open_):
        gain = np.zeros(len(combos), dtype=np.int64)
        for p, todo in enumerate(open_):
            gain += np.isin(keys[:, p], list(todo))
        c = int(np.argmax(gain))
        for p, todo in enumerate(open_):
            todo.discard(int(keys[c, p]))
        M, m, n, (bits, dtype), bias, inv_t = (AXES[a][i] for a, i in enumerate(combos[c]))
        cases.append((bits, dtype, M, m, n, bias, True, inv_t))
    return cases


CASES = build_cases()
LARGE_VOCAB = hm.LARGE_VOCAB
DIST_CASE = (4, "fp16", 4096, 8, 32, True, True, 1.0)  # the distribution test: 64 tile launches
DIST_SEEDS = tuple(zlib.crc32(f"head_pick_rng-dist-{k}".encode()) for k in range(3))
CHI2_7_999 = 24.32  # the 0.999 quantile of chi-square at 7 degrees of freedom


def case_state(c):
    """(seed, offset) of a case, fixed in advance: the seed is crc32 of the case id (spread over 64 bits so that seed_hi is not 0),
    the offset walks OFFSETS"""
    h = zlib.crc32(("rng-" + hm.case_id(c)).encode())
    return (h * 0x9E3779B97F4A7C15 + h) & 0xFFFFFFFFFFFFFFFF, OFFSETS[h % len(OFFSETS)]


def gaussian_case(c):
    """(inp, g fp64, ref, seed, offset) of a case: tests/lut_arena.py's Gaussian inputs with x doubled (as hm.gaussian_case, seed
    crc32(case id)) and the model's noise under case_state(c).  Nothing is searched."""
    import lut_arena as la

    bits, dtype, M, m, n, with_bias, _, inv_t = c
    inp = la.gaussian(bits, M, m, n, "plain" if with_bias else "nobias", zlib.crc32(hm.case_id(c).encode()))
    inp["x"] *= 2.0
    seed, offset = case_state(c)
    g = noise(seed, offset, M, m)
    return inp, g, reference(inp, dtype, inv_t, g), seed, offset


def padding_case(c):
    """(inp, g, ref, seed, offset) of a case of hm.PADDING_CASES: every real logit <= -40 (bias -48), inv_t = 1"""
    import lut_arena as la

    bits, dtype, M, m, n = c
    inp = la.gaussian(bits, M, m, n, "plain", 11 * m + n)
    inp["bias"] = np.full(m, -48.0, dtype=np.float32)
    seed, offset = case_state(c + (True, True, 1.0))
    g = noise(seed, offset, M, m)
    return inp, g, reference(inp, dtype, 1.0, g), seed, offset


def dist_inputs():
    """the distribution case: m = 8 features whose logits are the SAME on every row, with probabilities spanning two decades.
    x = e_0 (the first column 1, the rest 0), every codebook entry of feature o equal to c_o, no spread from the indices: the logit
    of feature o is c_o + bias_o exactly.  -> (inp of tests/lut_arena.py's layout, logits fp64 [8])"""
    bits, dtype, M, m, n = DIST_CASE[:5]
    V = 2 ** bits
    logits = np.log(np.array([1.0, 0.5, 0.25, 0.12, 0.06, 0.03, 0.02, 0.01]))  # probabilities 1 : ... : 0.01, two decades
    c = np.round(logits * 256) / 256  # representable in fp16
    x = np.zeros((M, n), dtype=np.float32)
    x[:, 0] = 1.0
    inp = dict(Q=np.zeros((m, n), dtype=np.uint8), lut=np.repeat(c[:, None], V, axis=1).astype(np.float32), x=x,
               bias=np.zeros(m, dtype=np.float32), addend=None, outliers=None, A=None, B=None)
    return inp, c.astype(np.float64)


def chi_square(tokens, logits):
    """Pearson's chi-square of the token counts against softmax(logits)"""
    p = np.exp(logits - logits.max())
    p /= p.sum()
    counts = np.bincount(tokens, minlength=p.size).astype(np.float64)
    expect = p * tokens.size
    return float(((counts - expect) ** 2 / expect).sum())
