"""How many digit planes of H the four-wave full bucket sum multiplies (no GPU): ganq_debug_top_rule evaluates top_dense_planes and
top_cap_in_force of csrc/update_t.hip, the functions the kernels and the preparation ask.  With c3 entries whose digit 3 is not
zero and c2 whose digit 2 or 3 is not: D = 2 if c2 <= cap, else 3 if c3 <= cap, else 4; no list (cap < 0, D = 4) under GANQ_T_TOP=0
and wherever the first kernel sums the layer."""
import pytest

from ganq_amd import _lib

OPTIONS = ("GANQ_ACCUM_W4", "GANQ_T_TOP", "GANQ_T_TOP_CAP")


@pytest.fixture(autouse=True)
def _reset():
    for name in OPTIONS:
        _lib.debug_option(name, None)
    yield
    for name in OPTIONS:
        _lib.debug_option(name, None)


def rule(c3, c2, m=8, n=256):
    return _lib.debug_top_rule(m, n, c3, c2)


def test_counts_and_cap_give_the_number_of_dense_planes():
    _lib.debug_option("GANQ_ACCUM_W4", 1)
    _lib.debug_option("GANQ_T_TOP_CAP", 100)
    for c3, c2, D in ((0, 0, 2), (0, 100, 2), (100, 100, 2), (0, 101, 3), (100, 101, 3), (100, 10 ** 9, 3), (101, 101, 4),
                      (101, 10 ** 9, 4)):
        r = rule(c3, c2)
        assert r["D"] == D and r["cap"] == 100, (c3, c2, r)


def test_cap_zero_takes_only_empty_lists():
    _lib.debug_option("GANQ_ACCUM_W4", 1)
    _lib.debug_option("GANQ_T_TOP_CAP", 0)
    assert rule(0, 0)["D"] == 2 and rule(0, 1)["D"] == 3 and rule(1, 1)["D"] == 4
    assert rule(0, 0)["cap"] == 0


def test_cap_is_clamped_to_the_capacity_of_a_list():
    _lib.debug_option("GANQ_ACCUM_W4", 1)
    _lib.debug_option("GANQ_T_TOP_CAP", 10 ** 9)
    top = rule(0, 0)["list_max"]
    assert 0 < top < 10 ** 9
    assert rule(0, top) == dict(D=2, cap=top, list_max=top)
    assert rule(0, top + 1)["D"] == 3 and rule(top, top + 1)["D"] == 3
    assert rule(top + 1, top + 1)["D"] == 4


def test_default_cap_lies_inside_the_list_and_grows_with_in_features():
    _lib.debug_option("GANQ_ACCUM_W4", 1)
    caps = [rule(0, 0, m=8, n=n)["cap"] for n in (256, 1024, 4096, 16384, 32768)]
    top = rule(0, 0)["list_max"]
    assert all(0 <= c <= top for c in caps) and caps == sorted(caps), caps
    assert len({rule(0, 0, m=m, n=4096)["cap"] for m in (1, 32, 4096)}) == 1  # the break-even count does not depend on m


def test_switch_0_is_the_four_plane_sum_whatever_the_counts():
    _lib.debug_option("GANQ_ACCUM_W4", 1)
    _lib.debug_option("GANQ_T_TOP", 0)
    for cap in (-1, 0, 10 ** 9):
        _lib.debug_option("GANQ_T_TOP_CAP", cap)
        for c3, c2 in ((0, 0), (0, 5), (5, 5)):
            r = rule(c3, c2)
            assert r["D"] == 4 and r["cap"] < 0, (cap, c3, c2, r)


def test_first_kernel_always_sums_four_planes():
    _lib.debug_option("GANQ_T_TOP_CAP", 10 ** 9)
    for w4, m, n in ((0, 8, 256), (0, 4096, 4096), (1, 8, 255), (1, 8, 1000), (-1, 8, 256)):
        _lib.debug_option("GANQ_ACCUM_W4", w4)
        assert _lib.accum_plan(m, n)["kernel"] == "onehot_accum"
        r = rule(0, 0, m=m, n=n)
        assert r["D"] == 4 and r["cap"] < 0, (w4, m, n, r)
    _lib.debug_option("GANQ_ACCUM_W4", -1)
    assert _lib.accum_plan(4096, 4096)["kernel"] == "onehot_accum_w4" and rule(0, 0, m=4096, n=4096)["D"] == 2


def test_bad_arguments_are_errors():
    for m, n, c3, c2 in ((0, 256, 0, 0), (8, 0, 0, 0), (8, 256, -1, 0), (8, 256, 2, 1)):
        with pytest.raises(_lib.GanqHipError):
            _lib.debug_top_rule(m, n, c3, c2)
