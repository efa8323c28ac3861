"""The cases of tests/test_hip_mupdate_top.py are what they claim (no GPU): the model's exception counts give the D each case means,
the named columns have the listed partners they are named for, every change count at the kernel's tile and pass borders is reached,
and ganq_debug_mu_planes follows GANQ_MU_TOP.  Also the identity the kernel's diagonal term rests on: the low D balanced digits of a
word are its residue modulo 256^D shifted into [-B, 256^D - 1 - B]."""
import numpy as np
import pytest

import mupdate_top_cases as C
import t_update_model as M

OPTIONS = ("GANQ_ACCUM_W4", "GANQ_T_TOP", "GANQ_T_TOP_CAP", "GANQ_MU_TOP")


@pytest.fixture(scope="module")
def built():
    return {c["name"]: C.build(c) for c in C.CASES}


def test_names_are_unique_and_shapes_are_the_prescribed_ones():
    names = [c["name"] for c in C.CASES]
    assert len(set(names)) == len(names)
    assert {c["n"] for c in C.CASES} == set(C.MU_N) and {c["m"] for c in C.CASES} == set(C.MU_M)
    assert {c["V"] for c in C.CASES} == {4, 8, 16} and {c["ext_mode"] for c in C.CASES} == {0, 1}
    for kind, _, D in C.KINDS:
        mine = [c for c in C.CASES if c["hessian"] == kind and c["D"] == D and c["name"].startswith("borders")]
        assert {c["n"] for c in mine} == set(C.MU_N) and {c["m"] for c in mine} == set(C.MU_M), (kind, D)


@pytest.mark.parametrize("case", C.CASES, ids=[c["name"] for c in C.CASES])
def test_case_means_its_D_and_its_changes(built, case):
    H, q, (c3, c2), cap, Qseq, changes, sets, pc = built[case["name"]]
    n = case["n"]
    eff = min(cap if cap >= 0 else C.default_cap(n), 131072)
    assert C.rule(c3, c2, eff) == case["D"], (c3, c2, cap)
    assert len(Qseq) == len(case["expect"]) and (Qseq < case["V"]).all()
    thr = case["options"]["GANQ_T_INCR_THR"]
    path = "F" + "".join("I" if changes[k].sum() <= thr else "F" for k in range(1, len(Qseq)))
    assert path == case["expect"]
    if case["name"].startswith("borders") or case["name"].startswith("overflow"):
        assert set(C.BORDER_COUNTS) <= set(changes[1:].ravel().tolist())
    if case["name"].startswith("long"):
        assert changes.max() == n and ((changes > 512) & (changes < n)).any()
    if case["name"].startswith("gate"):
        assert changes.sum(axis=1).tolist()[1:5] == [36, 45, 36, 40]
    if case["name"].startswith("columns"):
        big, small, lonely = sets["massive"][0], sets["partner"][0], sets["lonely"][0]
        assert pc[big] == pc.max() > 0 and pc[small] >= 1 and pc[lonely] == 0, (pc[big], pc[small], pc[lonely])
        _, top = C.partner_counts(q, case["D"])
        assert top[big, small] and top[small, big]
        if case["hessian"] == "massive" and case["D"] == 2:
            assert pc[big] > 32  # more than a thread of the kernel takes alone
        if case["hessian"] == "planted":  # both signs of the top digit are among the listed entries, and columns 0 and n - 1 are ends
            ds, _ = M.digits(q["I"], 4)
            assert ds[3].min() == -64 and ds[3].max() == 64 and pc[0] >= 1 and pc[n - 1] >= 1


def test_long_list_case_has_a_long_list(built):
    H, q, (c3, c2), cap, *_, pc = built["long-ordinary-D3"]
    assert 65536 < c3 <= 131072 < c2 and (pc > 64).sum() > 64  # more big columns in a row than the kernel's table of them holds


def test_low_digits_identity():
    rng = np.random.default_rng(5)
    x = np.concatenate([rng.integers(-2 ** 30, 2 ** 30 + 1, size=20000), [2 ** 30, -2 ** 30, 0, 32639, 32640, -32896, -32897, 8355711, 8355712]])
    for D, B in ((2, 0x8080), (3, 0x808080)):
        ds, _ = M.digits(x, D)
        assert np.array_equal(M.recombine(ds), ((x + B) & (256 ** D - 1)) - B)
    ds, rest = M.digits(x, 4)
    assert not rest.any() and np.array_equal(M.recombine(ds), x)


def test_mu_planes_rule_follows_the_option():
    from ganq_amd import _lib

    try:
        for name in OPTIONS:
            _lib.debug_option(name, None)
        _lib.debug_option("GANQ_ACCUM_W4", 1)
        for cap, c3, c2, D in ((100, 0, 100, 2), (100, 100, 101, 3), (100, 101, 200, 4), (0, 0, 0, 2)):
            _lib.debug_option("GANQ_T_TOP_CAP", cap)
            _lib.debug_option("GANQ_MU_TOP", -1)
            assert _lib.debug_mu_planes(9, 512, c3, c2) == {"D": D, "D_full": D}
            _lib.debug_option("GANQ_MU_TOP", 3)  # the full sum's planes, but at least three
            assert _lib.debug_mu_planes(9, 512, c3, c2) == {"D": max(D, 3), "D_full": D}
            _lib.debug_option("GANQ_MU_TOP", 0)
            assert _lib.debug_mu_planes(9, 512, c3, c2) == {"D": 4, "D_full": D}
        _lib.debug_option("GANQ_MU_TOP", -1)
        _lib.debug_option("GANQ_T_TOP", 0)  # no lists: four planes on both sides
        assert _lib.debug_mu_planes(9, 512, 0, 0) == {"D": 4, "D_full": 4}
        _lib.debug_option("GANQ_T_TOP", None)
        _lib.debug_option("GANQ_ACCUM_W4", 0)  # the first kernel sums the layer: no lists either
        assert _lib.debug_mu_planes(9, 512, 0, 0) == {"D": 4, "D_full": 4}
        _lib.debug_option("GANQ_ACCUM_W4", None)
        _lib.debug_option("GANQ_T_TOP_CAP", None)
        assert _lib.debug_mu_planes(4096, 4096, 2, 10 ** 6)["D"] == 3  # the benchmark layer under the defaults
        with pytest.raises(_lib.GanqHipError):
            _lib.debug_mu_planes(9, 512, 5, 4)
    finally:
        for name in OPTIONS:
            _lib.debug_option(name, None)
