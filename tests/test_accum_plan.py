"""Which kernel sums the T-update's buckets in full (no GPU): ganq_debug_accum_plan evaluates accum_plan of csrc/update_t.hip, the
function the launch itself asks.  The four-wave kernel (onehot_accum_w4_kernel) serves in_features that are a multiple of 256 and
every m >= 1; GANQ_ACCUM_W4 = 0 forbids it, 1 takes it wherever it is supported, -1 (the default) decides by shape -- and may only
ever pick it inside the supported set."""
import pytest

from ganq_amd import _lib

M_ALL = range(1, 71)
N_ALL = (1, 255, 256, 257, 512, 1000, 4096, 11008, 14336, 16384)


@pytest.fixture(autouse=True)
def _reset():
    yield
    _lib.debug_option("GANQ_ACCUM_W4", None)


def supported(n):
    return n % 256 == 0


def test_other_in_features_stay_on_the_first_kernel_under_every_option():
    for opt in (None, -1, 0, 1):
        _lib.debug_option("GANQ_ACCUM_W4", opt)
        for n in N_ALL:
            if supported(n):
                continue
            for m in M_ALL:
                p = _lib.accum_plan(m, n)
                assert p == dict(kernel="onehot_accum", supported=False), (opt, m, n, p)


def test_option_0_never_takes_the_four_wave_kernel():
    _lib.debug_option("GANQ_ACCUM_W4", 0)
    for n in N_ALL:
        for m in M_ALL:
            p = _lib.accum_plan(m, n)
            assert p["kernel"] == "onehot_accum" and p["supported"] == supported(n), (m, n, p)


def test_option_1_takes_it_exactly_on_the_supported_set():
    _lib.debug_option("GANQ_ACCUM_W4", 1)
    for n in N_ALL:
        for m in M_ALL:
            p = _lib.accum_plan(m, n)
            assert p["supported"] == supported(n), (m, n, p)
            assert p["kernel"] == ("onehot_accum_w4" if supported(n) else "onehot_accum"), (m, n, p)


def test_default_plan_stays_inside_the_supported_set():
    for opt in (None, -1):
        _lib.debug_option("GANQ_ACCUM_W4", opt)
        for n in N_ALL:
            for m in M_ALL:
                p = _lib.accum_plan(m, n)
                assert p["kernel"] == "onehot_accum" or p["supported"], (m, n, p)


def test_bad_shapes_are_errors():
    for m, n in ((0, 256), (1, 0), (-1, 256)):
        with pytest.raises(_lib.GanqHipError):
            _lib.accum_plan(m, n)
