"""The arithmetic of csrc/lut_head_nll.hip without a GPU: the numpy fp64 model of its tile, merge and combine steps
(tests/head_nll_model.py) against np.logaddexp.reduce on the shapes, targets and the padding case the GPU test runs, the workspace
layout against the library's sizer (pure host code), and the coverage of the shared case list."""
import numpy as np
import pytest

import head_nll_model as hm


def reference(logits, targets):
    M, m = logits.shape
    lse = np.logaddexp.reduce(logits, axis=1)
    hit = (targets >= 0) & (targets < m)
    tgt = np.where(hit, logits[np.arange(M), np.clip(targets, 0, m - 1)], 0.0)
    return np.where(hit, lse - tgt, 0.0), lse, tgt


@pytest.mark.parametrize("M", hm.MS)
@pytest.mark.parametrize("m", hm.OUTS + (1000, 2200))
def test_model_against_logaddexp(M, m):
    """per-tile (max, sum), the lane tree, the ascending merge in 16 ranges (m = 2200: 18 tiles, two per range) and ignored rows;
    fp64 leaves the orders indistinguishable, so the model must agree to a few ulps"""
    rng = np.random.default_rng(1000 * M + m)
    logits = 4.0 * rng.standard_normal((M, m)) + 3.0 * rng.standard_normal((M, 1))
    logits[0, rng.integers(0, m)] = 60.0  # one dominant feature, wherever it falls
    targets = hm.make_targets(M, m, M + m)
    got, want = hm.head_nll(logits, targets), reference(logits, targets)
    for g, w, name in zip(got, want, ("nll", "lse", "tgt_logit")):
        assert np.abs(g - w).max() <= 64 * np.finfo(np.float64).eps * max(1.0, np.abs(w).max()), name
    hit = (targets >= 0) & (targets < m)
    assert (got[0][~hit] == 0).all() and (got[2][~hit] == 0).all() and np.isfinite(got[1]).all()
    if M >= 7:  # every special target met: the four inside the vocabulary score, the three outside do not
        sp = np.array(hm.special_targets(m))
        assert set(sp.tolist()) <= set(targets.tolist())
        for v in sp:
            assert bool(hit[targets == v].all()) == (0 <= v < m)


@pytest.mark.parametrize("m", [129, 300])
def test_padding_features_take_no_part(m):
    """every real logit <= -40: a padding feature of the last tile counted as a logit of 0 would lift lse by more than 30"""
    rng = np.random.default_rng(m)
    logits = -48.0 + rng.standard_normal((65, m))
    logits = np.minimum(logits, -40.0)
    targets = hm.make_targets(65, m, m)
    nll, lse, tgt = hm.head_nll(logits, targets)
    want = reference(logits, targets)
    assert np.abs(lse - want[1]).max() <= 1e-12 * 48 and np.abs(nll - want[0]).max() <= 1e-12 * 48
    assert (lse < -40 + np.log(m)).all()
    wrong = hm.head_nll(logits, targets, count_padding=True)[1]
    assert (wrong - lse).min() > 30


@pytest.mark.parametrize("M,m", [(M, m) for M in hm.MS for m in hm.OUTS] + [(300, 128256), (4096, 128256), (4096, 50272)])
def test_workspace_formula_matches_the_layout(M, m):
    """8 bytes per row and 128-feature tile, then 4 bytes per row; within the 16 M ceil(m / 128) bytes (plus tgt) the design allows;
    the sizer is host code: no GPU"""
    from ganq_amd import _lib

    _lib.build()
    lay = hm.workspace_layout(M, m)
    T = -(-m // 128)
    assert lay["partial_offset"] == 0 and lay["tgt_offset"] == lay["partial_bytes"] == 8 * M * T
    assert lay["tgt_offset"] % 4 == 0 and lay["total"] == lay["tgt_offset"] + 4 * M
    for n, bits in ((32, 2), (512, 3), (2048, 4)):
        assert _lib.lib().ganq_lut_head_nll_workspace_bytes(M, m, n, bits) == lay["total"]
    assert lay["total"] <= 16 * M * T + 4 * M
    assert _lib.lib().ganq_lut_head_nll_workspace_bytes(0, m, 32, 4) == 0


def test_case_list_covers_the_axes():
    cases = hm.CASES
    assert len(cases) == len(set(cases)) == 40
    assert {(c[2], c[3]) for c in cases} == {(M, m) for M in hm.MS for m in hm.OUTS}
    assert {(c[3], c[4]) for c in cases} == {(m, n) for m in hm.OUTS for n in hm.INS}
    assert {(c[2], c[4]) for c in cases} == {(M, n) for M in hm.MS for n in hm.INS}
    for pair in hm.PAIRS:
        mine = [c for c in cases if (c[0], c[1]) == pair]
        assert {c[4] % 64 for c in mine} == {0, 32} and {c[5] for c in mine} == {True, False}, pair
    assert {c[2] for c in cases if c[5]} == set(hm.MS) == {c[2] for c in cases if not c[5]}
