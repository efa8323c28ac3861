"""A numpy fp64 model of the arithmetic of csrc/lut_head_pick.hip, and the case list its tests share (tests/test_head_pick_model.py
without a GPU, tests/test_hip_head_pick.py on one).  A helper module like tests/head_nll_model.py, not a conftest.

Semantics (include/ganq_hip.h):  s = logits * inv_t,  lse = log sum_o exp(s),  z = s + noise,  token = the SMALLEST o with
z[o] = max z,  score = s[token],  logprob = score - lse; only valid features (o < m) take part.

The model follows the kernels step by step -- what takes part, and in which order it is merged:
  tile kernel   a feature block holds 128 features: wave w (of 4) owns features 32 w .. 32 w + 31 of it as two tiles of 16, lane
                `col` of a row's 16 lanes owns feature 16 t + col of tile t.  A valid feature starts as the record
                (mx, sm, zb, sb, ob) = (s, 1, z, s, o), a padding feature (o >= m) as (NEG, 0, -inf, 0, NONE).  Records merge as
                M = max(m1, m2), S = s1 exp(m1 - M) + s2 exp(m2 - M); a strictly larger z wins, an equal z keeps the smaller index.
                Order: the 16 lanes by four exchanges at lane distances 1, 2, 4, 8, then tile 1 into tile 0, then waves 1, 2, 3
                into wave 0.
  merge kernel  one wave per row; its 64 lanes take 64 contiguous ranges of ceil(T / 64) feature blocks: the row's maximum over all
                blocks, then every lane walks its range in ascending block order (sum of sm exp(mx - max); best z by the same tie
                rule) and the 64 merge by exchanges at lane distances 1, 2, ..., 32.  lse = max + log(sum).
  workspace     rec4[M][T] of four fp32 (16 bytes) from byte 0, then reco[M][T] int32: 20 M T bytes.
  launches      one tile launch per 64 rows, RT = ceil(rows / 16) row tiles each; one merge launch of ceil(M / 4) workgroups."""
import zlib

import numpy as np

BLOCK = 128
WAVES = 4
LANES = 16
MERGE_LANES = 64
MERGE_ROWS = 4
ROWS_PER_LAUNCH = 64
NEG = -float(np.finfo(np.float32).max)
NONE = int(np.iinfo(np.int32).max)
U = 2.0 ** -24


def blocks_of(m):
    return -(-m // BLOCK)


def workspace_layout(M, m):
    """byte offsets and sizes of the two arrays the kernels keep in the caller's workspace"""
    T = blocks_of(m)
    return dict(rec4_offset=0, rec4_bytes=16 * M * T, reco_offset=16 * M * T, reco_bytes=4 * M * T, total=20 * M * T)


def launch_plan(M):
    """(tile launches, [RT of each], workgroups of the merge launch)"""
    rows = [min(ROWS_PER_LAUNCH, M - r) for r in range(0, M, ROWS_PER_LAUNCH)]
    return len(rows), [-(-r // 16) for r in rows], -(-M // MERGE_ROWS)


def _merge(a, b):
    """record b joins record a (tuples of equally shaped arrays)"""
    m1, s1, z1, c1, o1 = a
    m2, s2, z2, c2, o2 = b
    mm = np.maximum(m1, m2)
    sm = s1 * np.exp(m1 - mm) + s2 * np.exp(m2 - mm)
    take = (z2 > z1) | ((z2 == z1) & (o2 < o1))
    return mm, sm, np.where(take, z2, z1), np.where(take, c2, c1), np.where(take, o2, o1)


def block_records(s, z, count_padding=False):
    """s, z fp64 [M, m] -> the record (mx, sm, zb, sb, ob), each [M, T], every feature block leaves per row.
    count_padding=True is the BUG the padding test looks for: features past m counted as logits of 0."""
    M, m = s.shape
    T = blocks_of(m)
    sp, zp = np.zeros((M, T * BLOCK)), np.zeros((M, T * BLOCK))
    sp[:, :m], zp[:, :m] = s, z
    o = np.arange(T * BLOCK)
    valid = o < (T * BLOCK if count_padding else m)
    shape = (M, T, WAVES, 2, LANES)  # [row][block][wave][tile][lane]
    valid = np.broadcast_to(valid, (M, T * BLOCK)).reshape(shape)
    sp, zp, o = sp.reshape(shape), zp.reshape(shape), np.broadcast_to(o, (M, T * BLOCK)).reshape(shape)
    rec = (np.where(valid, sp, NEG), np.where(valid, 1.0, 0.0), np.where(valid, zp, -np.inf), np.where(valid, sp, 0.0),
           np.where(valid, o, NONE))
    for w in (1, 2, 4, 8):  # lane meets lane ^ w
        partner = np.arange(LANES) ^ w
        rec = _merge(rec, tuple(a[..., partner] for a in rec))
    rec = tuple(a[..., 0] for a in rec)                                      # every lane holds the row's record
    rec = _merge(tuple(a[..., 0] for a in rec), tuple(a[..., 1] for a in rec))  # the wave's two tiles
    out = tuple(a[..., 0] for a in rec)
    for w in range(1, WAVES):                                                # wave order
        out = _merge(out, tuple(a[..., w] for a in rec))
    return out


def combine(rec):
    """records [M, T] -> (token, score, lse)"""
    mx, sm, zb, sb, ob = rec
    M, T = mx.shape
    per = -(-T // MERGE_LANES)
    mrow = mx.max(axis=1)

    def better(cur, z, c, o):
        take = (z > cur[0]) | ((z == cur[0]) & (o < cur[2]))
        return np.where(take, z, cur[0]), np.where(take, c, cur[1]), np.where(take, o, cur[2])

    lanes = []
    for l in range(MERGE_LANES):
        s = np.zeros(M)
        mine = (np.full(M, -np.inf), np.zeros(M), np.full(M, NONE))
        for t in range(min(T, l * per), min(T, (l + 1) * per)):
            s = s + sm[:, t] * np.exp(mx[:, t] - mrow)
            mine = better(mine, zb[:, t], sb[:, t], ob[:, t])
        lanes.append((s,) + mine)
    lanes = tuple(np.stack(a, axis=1) for a in zip(*lanes))  # [M, lane]
    w = 1
    while w < MERGE_LANES:  # lane meets lane ^ w
        partner = np.arange(MERGE_LANES) ^ w
        s, best = lanes[0] + lanes[0][:, partner], better(lanes[1:], *(a[:, partner] for a in lanes[1:]))
        lanes = (s,) + best
        w *= 2
    return lanes[3][:, 0].astype(np.int64), lanes[2][:, 0], mrow + np.log(lanes[0][:, 0])


def head_pick(logits, inv_t=1.0, noise=None, count_padding=False):
    """-> (token int64, score, lse, logprob fp64) [M]"""
    s = np.asarray(logits, dtype=np.float64) * inv_t
    z = s if noise is None else s + np.asarray(noise, dtype=np.float64)
    token, score, lse = combine(block_records(s, z, count_padding))
    return token, score, lse, score - lse


def brute_force(logits, inv_t=1.0, noise=None):
    """the definition itself: np.argmax takes the first maximum; a log-sum-exp around the row maximum"""
    s = np.asarray(logits, dtype=np.float64) * inv_t
    z = s if noise is None else s + np.asarray(noise, dtype=np.float64)
    token = np.argmax(z, axis=1)
    mx = s.max(axis=1)
    lse = mx + np.log(np.exp(s - mx[:, None]).sum(axis=1))
    score = s[np.arange(s.shape[0]), token]
    return token.astype(np.int64), score, lse, score - lse


# ---- the cases both test files run
MS = (1, 16, 17, 64, 65)
OUTS = (1, 127, 128, 129, 300)
INS = (32, 96, 160, 512)
PAIRS = [(b, d) for b in (2, 3, 4) for d in ("fp16", "bf16")]
INV_TS = (1.0, 0.5, 1 / 0.7)
AXES = (MS, OUTS, INS, PAIRS, (True, False), (True, False), INV_TS)  # M, m, n, (bits, dtype), bias, noise, inv_t


def build_cases():
    """a greedy pairwise cover of the seven axes: the next case is the combination (in the product's own order) that meets the most
    value pairs of two axes no earlier case has met, until every pair of values of every two axes is met
    (tests/test_head_pick_model.py checks the coverage).  -> tuples (bits, dtype, M, m, n, bias, noise, inv_t)"""
    import itertools

    idx = [range(len(a)) for a in AXES]
    combos = np.array(list(itertools.product(*idx)), dtype=np.int64)
    pairs = list(itertools.combinations(range(len(AXES)), 2))
    keys = np.stack([combos[:, a] * 8 + combos[:, b] for a, b in pairs], axis=1)  # [combo][axis pair] -> value pair
    open_ = [set((i * 8 + j) for i in range(len(AXES[a])) for j in range(len(AXES[b]))) for a, b in pairs]
    cases = []
    while any(open_):
        gain = np.zeros(len(combos), dtype=np.int64)
        for p, todo in enumerate(open_):
            gain += np.isin(keys[:, p], list(todo))
        c = int(np.argmax(gain))
        for p, todo in enumerate(open_):
            todo.discard(int(keys[c, p]))
        M, m, n, (bits, dtype), bias, noise, inv_t = (AXES[a][i] for a, i in enumerate(combos[c]))
        cases.append((bits, dtype, M, m, n, bias, noise, inv_t))
    return cases


CASES = build_cases()
PADDING_CASES = [(4, "fp16", 65, 129, 96), (3, "bf16", 17, 300, 512)]  # every real logit <= -40 (bias -48)
LARGE_VOCAB = (4, "fp16", 5, 128256, 64, True, True, 1 / 0.7)
TIE_FEATURES = (5, 21, 40, 133)  # the same wave's other tile, another wave, another workgroup


def case_id(c):
    bits, dtype, M, m, n = c[:5]
    tail = "" if len(c) < 8 else f"-{'bias' if c[5] else 'nobias'}-{'noise' if c[6] else 'greedy'}-t{1 / c[7]:.2g}"
    return f"b{bits}-{dtype}-{M}x{m}x{n}" + tail


def rounded(a, dtype):
    """fp32 values -> what the fp16 / bf16 tensor of them holds, as fp64"""
    import torch

    return torch.from_numpy(np.ascontiguousarray(a)).to(torch.float16 if dtype == "fp16" else torch.bfloat16).double().numpy()


def gumbel(M, m, seed):
    """fp32 [M, m]: -log(E), E ~ Exp(1)"""
    e = np.random.default_rng(seed).exponential(size=(M, m))
    return (-np.log(np.maximum(e, np.finfo(np.float32).tiny))).astype(np.float32)


def reference(inp, dtype, inv_t, noise):
    """fp64 reference of the inputs of tests/lut_arena.py (dict of numpy arrays; rounded to `dtype` as the device tensors are):
    dict(s, z [M, m], lse, E, E1, gap [M], token [M]).  Per row
        E  = n 2^-23 max_o sum_j |x_j w_oj|           bounds the error of every fp32 logit (tests/test_hip_head_nll.py),
        E1 = E inv_t + 4 2^-24 max_o |z_o|            that of s and of z: the logit's error scaled, one rounding each of the sum with
                                                      the bias, the product with inv_t and the sum with the noise (2^-24
                                                      relative each, and one to spare),
        gap = the best z minus the second best (inf for m = 1): above 2 E1 the fp32 argmax IS the fp64 argmax."""
    x = rounded(inp["x"], dtype)
    W = np.take_along_axis(rounded(inp["lut"], dtype), inp["Q"].astype(np.int64), axis=1)
    logits = x @ W.T
    if inp["bias"] is not None:
        logits = logits + rounded(inp["bias"], dtype)
    E = x.shape[1] * 2.0 ** -23 * (np.abs(x) @ np.abs(W).T).max(axis=1)
    s = logits * float(np.float32(inv_t))
    z = s if noise is None else s + noise.astype(np.float64)
    E1 = E * inv_t + 4 * U * np.abs(z).max(axis=1)
    token, score, lse, logprob = brute_force(logits, float(np.float32(inv_t)), noise)
    if z.shape[1] > 1:
        top2 = np.partition(z, -2, axis=1)[:, -2:]
        gap = top2[:, 1] - top2[:, 0]
    else:
        gap = np.full(z.shape[0], np.inf)
    return dict(s=s, z=z, lse=lse, E=E, E1=E1, gap=gap, token=token, score=score, logprob=logprob)


def decisive_share(ref):
    return float((ref["gap"] > 2 * ref["E1"]).mean())


def gaussian_case(c):
    """(inp, noise, ref) of a case: tests/lut_arena.py's Gaussian inputs with x doubled (logits of a few units), Gumbel noise, from
    the first seed crc32(case id) + k, k = 0, 1, ..., at which the fp64 gap between the best and the second-best z exceeds 2 E1 on
    at least 90 % of the rows (a condition on the reference alone; tests/test_head_pick_model.py checks it for every case)"""
    import lut_arena as la

    bits, dtype, M, m, n, with_bias, with_noise, inv_t = c
    base = zlib.crc32(case_id(c).encode())
    for k in range(16):
        inp = la.gaussian(bits, M, m, n, "plain" if with_bias else "nobias", base + k)
        inp["x"] *= 2.0
        noise = gumbel(M, m, base + k + 1) if with_noise else None
        ref = reference(inp, dtype, inv_t, noise)
        if decisive_share(ref) >= 0.9:
            return inp, noise, ref
    raise AssertionError(f"{case_id(c)}: no seed with 90 % decisive rows")
