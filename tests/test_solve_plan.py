"""The S-solve's helper plan on the host (no GPU): ganq_debug_solve_plan / ganq_debug_solve_role evaluate the two functions the
kernel itself runs (solve_plan, solve_role in csrc/solve_s.hip).  For every active tile count from 1 to 400 on parts of 32, 64, 256
and 304 CUs, in the grid the host launches and in the 256-workgroup grid of a 4096-row layer whose rows have partly converged:

  * the roles stay within the grid, within min(grid, CUs) in total and within every ticket class (blockIdx mod 8);
  * every active tile is dealt exactly once, has at most one first helper (exactly one in a helped launch) and, in a trio, one
    second helper; the tiles of a group draw their tickets before the group's helper;
  * no helper serves more than SHARE_MAX_K = 4 tiles, and a shared launch uses the smallest k that fits;
  * with at most half as many tiles as CUs the decision is the duo / trio rule as it stood before the shared helpers.
"""
import pytest

SHARE_MAX_K = 4
DUO_MAX_TILES, DUO_TRIO_TILES = 128, 80


def class_size(total, cls):
    return (total - cls + 7) // 8 if total > cls else 0


def old_rule(A, grid, ncu):
    """the kernel's decision before the shared regime (duo_pol, trio_pol both set)"""
    cap, g8 = min(grid, ncu), (A + 7) // 8
    if A <= DUO_TRIO_TILES and 24 * g8 <= cap:
        return "trio"
    if A <= DUO_MAX_TILES and 16 * g8 <= cap:
        return "duo"
    return "none"


def old_grid(tiles, ncu):
    grid = max(tiles, min(16 * ((tiles + 7) // 8), ncu // 16 * 16))
    return max(grid, min(24 * ((tiles + 7) // 8), ncu // 24 * 24))


@pytest.mark.parametrize("ncu", [32, 64, 256, 304])
def test_plan_within_grid_and_classes(ncu):
    from ganq_amd import _lib

    seen = set()
    for A in range(1, 401):
        for grid in (0, 256):
            if grid and grid < A:
                continue
            p = _lib.debug_solve_plan(A, grid=grid, ncu=ncu)
            g = p["grid"]
            assert g >= A and (grid == 0 or g == grid)
            if 2 * A <= ncu:
                assert g >= old_grid(A, ncu) if grid == 0 else True
                assert p["regime"] == old_rule(A, g, ncu), (A, g, ncu, p)
            if p["regime"] == "none":
                assert p["helpers"] == 0
                continue
            seen.add((p["regime"], p["k"]))
            assert A + p["helpers"] <= min(g, ncu), (A, ncu, p)
            first, second, tiles, helpers = {}, {}, set(), 0
            for cls in range(8):
                in_class = class_size(g, cls)
                started = set()
                for tk in range(in_class):
                    r = _lib.debug_solve_role(A, cls, tk, grid=g, ncu=ncu)
                    if r["tile"] is None:
                        continue
                    assert r["tile"] % 8 == cls and r["tile"] < A
                    if r["stage"] == 0:
                        assert r["tile"] not in tiles
                        tiles.add(r["tile"])
                        started.add(r["tile"])
                        continue
                    helpers += 1
                    assert 1 <= r["serves"] <= (SHARE_MAX_K if p["regime"] == "shared" else 1)
                    assert r["serves"] <= p["k"]
                    book = first if r["stage"] == 1 else second
                    for i in range(r["serves"]):
                        t = r["tile"] + 8 * i
                        assert t < A and t not in book, (A, ncu, cls, tk, r)
                        assert t in started, "a helper's tiles draw before it"
                        book[t] = (cls, tk)
                # the tickets beyond the class's share of the grid have no role: nothing the plan needs is left out
                r = _lib.debug_solve_role(A, cls, in_class, grid=g, ncu=ncu)
                assert r["tile"] is None, (A, ncu, cls, in_class, r)
            assert tiles == set(range(A))
            assert set(first) == tiles and helpers == p["helpers"]
            assert set(second) == (tiles if p["regime"] == "trio" else set())
            if p["regime"] == "shared":
                assert 2 <= p["k"] <= SHARE_MAX_K and 2 * A > ncu
                assert old_rule(A, g, ncu) == "none"
    if ncu == 256:
        assert {("shared", 2), ("shared", 3), ("shared", 4), ("duo", 1), ("trio", 1)} <= seen
        # the benchmark layer's launches (256 workgroups): the tile counts of iterations 5 and 6 are shared, iteration 4 is not
        assert _lib.debug_solve_plan(182, grid=256, ncu=256)["k"] == 3
        assert _lib.debug_solve_plan(139, grid=256, ncu=256)["k"] == 2
        assert _lib.debug_solve_plan(225, grid=256, ncu=256)["regime"] == "none"


def test_plan_options():
    """GANQ_SOLVE_SHARE=0 is the rule as it stood; GANQ_SOLVE_SHARE_K forces one k or no helpers; GANQ_SOLVE_DUO=0 switches every
    helper off; GANQ_SOLVE_CUS plans for a smaller chip."""
    from ganq_amd import _lib

    try:
        assert _lib.debug_solve_plan(182, ncu=256)["regime"] == "shared"
        _lib.debug_option("GANQ_SOLVE_SHARE_K", 2)
        assert _lib.debug_solve_plan(182, ncu=256)["regime"] == "none"  # 182 + 94 workgroups do not fit
        assert _lib.debug_solve_plan(144, ncu=256)["k"] == 2
        _lib.debug_option("GANQ_SOLVE_SHARE_K", 4)
        assert _lib.debug_solve_plan(144, ncu=256)["k"] == 4
        _lib.debug_option("GANQ_SOLVE_SHARE_K", None)
        _lib.debug_option("GANQ_SOLVE_SHARE", 0)
        for A in range(1, 300):
            p = _lib.debug_solve_plan(A, ncu=256)
            assert p["grid"] == old_grid(A, 256) and p["regime"] == old_rule(A, p["grid"], 256)
        _lib.debug_option("GANQ_SOLVE_SHARE", None)
        _lib.debug_option("GANQ_SOLVE_CUS", 32)
        assert _lib.debug_solve_plan(20, ncu=256) == _lib.debug_solve_plan(20, ncu=32)
        assert _lib.debug_solve_plan(20, ncu=256)["regime"] == "shared"
        _lib.debug_option("GANQ_SOLVE_CUS", None)
        _lib.debug_option("GANQ_SOLVE_DUO", 0)
        assert all(_lib.debug_solve_plan(A, ncu=256)["regime"] == "none" for A in (10, 100, 150, 200))
    finally:
        for name in ("GANQ_SOLVE_SHARE_K", "GANQ_SOLVE_SHARE", "GANQ_SOLVE_CUS", "GANQ_SOLVE_DUO"):
            _lib.debug_option(name, None)
