"""A numpy fp64 model of the arithmetic of csrc/lut_head_nll.hip, and the case list its tests share (tests/test_head_nll_model.py
without a GPU, tests/test_hip_head_nll.py on one).  A helper module like tests/lut_arena.py, not a conftest.

The model follows the kernels step by step -- what takes part, and in which order it is merged:
  tile kernel     a feature tile holds 128 features; lane l of a half-wave owns features 32 t + l (t = 0..3) of the tile.  Only
                  VALID features (o < m) take part: a lane without one starts from (NEG, 0), NEG the finite "nothing yet".
                  In the lane: mx = max over its valid features, sm = sum of exp(logit - mx).  Across the 32 lanes: five exchanges
                  at lane distances 16, 8, 4, 2, 1, each merging two pairs as M = max(m1, m2), S = s1 exp(m1 - M) + s2 exp(m2 - M).
  combine kernel  16 waves take 16 contiguous ranges of ceil(T / 16) feature tiles: the row's maximum over all tiles, then every wave
                  sums sm exp(mx - max) over its range in ascending tile order and the 16 sums are added in wave order.
  outputs         lse = max + log(sum); a target inside [0, m) gives tgt_logit = logits[row][target] and nll = lse - tgt_logit, any
                  other target (-100, -1, m, ...) an ignored row: nll = tgt_logit = 0, lse still written.
  workspace       partial[T][M] pairs of fp32 (8 bytes each) from byte 0, then tgt[M] fp32: 8 M T + 4 M bytes."""
import numpy as np

TILE = 128
LANES = 32
WAVES = 16
NEG = -float(np.finfo(np.float32).max)


def tiles_of(m):
    return -(-m // TILE)


def workspace_layout(M, m):
    """byte offsets and sizes of the two arrays the kernels keep in the caller's workspace"""
    T = tiles_of(m)
    return dict(partial_offset=0, partial_bytes=8 * M * T, tgt_offset=8 * M * T, tgt_bytes=4 * M, total=8 * M * T + 4 * M)


def _merge(m1, s1, m2, s2):
    mm = np.maximum(m1, m2)
    return mm, s1 * np.exp(m1 - mm) + s2 * np.exp(m2 - mm)


def tile_pairs(logits, count_padding=False):
    """logits fp64 [M, m] -> (mx, sm) fp64 [T, M]: the pair every feature tile leaves per row.
    count_padding=True is the BUG the padding test looks for: features past m counted as logits of 0."""
    M, m = logits.shape
    T = tiles_of(m)
    padded = np.zeros((M, T * TILE))
    padded[:, :m] = logits
    valid = np.arange(T * TILE) < (T * TILE if count_padding else m)
    mx_out, sm_out = np.empty((T, M)), np.empty((T, M))
    for tn in range(T):
        v = padded[:, tn * TILE:(tn + 1) * TILE].reshape(M, 4, LANES)      # [row][t][lane]
        ok = valid[tn * TILE:(tn + 1) * TILE].reshape(4, LANES)
        mx = np.full((M, LANES), NEG)
        for t in range(4):
            mx = np.where(ok[t], np.maximum(mx, v[:, t]), mx)
        sm = np.zeros((M, LANES))
        for t in range(4):
            sm = sm + np.where(ok[t], np.exp(np.where(ok[t], v[:, t] - mx, 0.0)), 0.0)
        W = LANES // 2
        while W >= 1:  # lane i meets lane i + W
            lo = (np.arange(mx.shape[1]) & W) == 0
            mx, sm = _merge(mx[:, lo], sm[:, lo], mx[:, ~lo], sm[:, ~lo])
            W //= 2
        mx_out[tn], sm_out[tn] = mx[:, 0], sm[:, 0]
    return mx_out, sm_out


def combine(mx, sm):
    """(mx, sm) [T, M] -> lse [M]"""
    T = mx.shape[0]
    per = -(-T // WAVES)
    mrow = mx.max(axis=0)
    tot = np.zeros(mx.shape[1])
    for w in range(WAVES):
        s = np.zeros(mx.shape[1])
        for t in range(min(T, w * per), min(T, (w + 1) * per)):
            s = s + sm[t] * np.exp(mx[t] - mrow)
        tot = tot + s
    return mrow + np.log(tot)


def head_nll(logits, targets, count_padding=False):
    """-> (nll, lse, tgt_logit) fp64 [M]"""
    logits = np.asarray(logits, dtype=np.float64)
    targets = np.asarray(targets, dtype=np.int64)
    M, m = logits.shape
    lse = combine(*tile_pairs(logits, count_padding))
    hit = (targets >= 0) & (targets < m)
    tgt = np.where(hit, logits[np.arange(M), np.clip(targets, 0, m - 1)], 0.0)
    return np.where(hit, lse - tgt, 0.0), lse, tgt


# ---- the cases both test files run
MS = (1, 65, 256, 257)
OUTS = (1, 127, 128, 129, 300)
INS = (32, 96, 160, 512)
PAIRS = [(b, d) for b in (2, 3, 4) for d in ("fp16", "bf16")]


def special_targets(m):
    return [0, 127, 128, m - 1, -100, m, -1]


def make_targets(M, m, seed):
    """int64 [M]: the special values first (rotated by the seed, so that the one-row cases meet different ones), then uniform ids"""
    rng = np.random.default_rng(seed)
    t = rng.integers(0, m, M).astype(np.int64)
    sp = special_targets(m)
    k = seed % len(sp)
    sp = sp[k:] + sp[:k]
    t[:min(M, len(sp))] = sp[:M]
    return t


def build_cases():
    """40 of the 4 x 5 x 4 x 6 x 2 combinations: every (M, m) pair twice, every n with every m and every M, every (bits, dtype) with
    ragged and whole in_features, with and without a bias (tests/test_head_nll_model.py checks the coverage)"""
    cases = []
    for i in range(40):
        M, m = MS[i % 4], OUTS[i % 5]
        n = INS[(i // 5) % 4]
        bits, dtype = PAIRS[(i + i // 4) % 6]
        cases.append((bits, dtype, M, m, n, (i // 3) % 2 == 0))
    return cases


CASES = build_cases()
PADDING_CASES = [(4, "fp16", 65, 129, 96), (3, "bf16", 257, 300, 512)]  # every real logit <= -40 (bias -48)
LARGE_VOCAB = (4, "fp16", 300, 128256, 256)


def case_id(c):
    bits, dtype, M, m, n = c[:5]
    return f"b{bits}-{dtype}-{M}x{m}x{n}" + ("" if len(c) < 6 else ("-bias" if c[5] else "-nobias"))
