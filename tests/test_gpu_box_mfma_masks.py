"""The matrix-pipe box kernel's edge masks (bm_box_mfma.hip) against oracle.box_disp / box_keys_slice
and against the VALU kernels forced with set_box_kernel(1): maps and keys bit-exact, with the harness of
test_gpu_box_mfma_pairs.py.  Each wave runs the disparities below d_m, the tile's first one that needs a mask, in
the unmasked loop in whole passes and the rest in the masked loop, where AD = 0 comes from the AND of abs_diff and
"no key" from +inf in the stage-2 C operand.  Frames are 50 rows high and at most 320 wide, and each test first
asserts, from the kernel's own arithmetic (test_box_mfma_masks_model.py, checked there by brute force), that its
shape still hits the case it is named for."""
import numpy as np
import pytest

from test_box_mfma_masks_model import T, WAVES, geometry, loop_passes, wave_split
from test_gpu_box_mfma_pairs import _check, _check_slice, _pair, env  # noqa: F401  (env is the fixture)

pytestmark = pytest.mark.gpu
H = 50


def _tiles(W, r, d_lo, d_hi):
    """One row of tiles: x0, the first disparity that needs the AD mask (`ad_from`) and the key mask (`key_from`),
    whether the staged tile has columns past W, the tile's d_end, and every wave's (dw_lo, dw_m, dw_hi, d_m)."""
    NP, TOX = geometry(r, d_lo, d_hi)
    return [dict(x0=x0, NP=NP, ad_from=x0 - r + 1, key_from=W - (min(x0 + TOX, W) - 1) + 1, past=x0 - r + T > W,
                 d_end=min(d_hi, W - x0 + 1), waves=[wave_split(W, r, d_lo, d_hi, x0, w) for w in range(WAVES)])
            for x0 in range(0, W, TOX)]


def _cases(W, r, d_lo, d_hi):
    """The names of the split's cases that (W, r, [d_lo, d_hi)) runs."""
    c = set()
    for t in _tiles(W, r, d_lo, d_hi):
        whole_free = whole_masked = False
        for lo, m, hi, d_m in t["waves"]:
            if hi - lo >= 2:
                if lo < d_m < hi:
                    c.add("d_m even" if (d_m - lo) % 2 == 0 else "d_m odd")
                c |= {name for name, v in (("d_m = lo", lo), ("d_m = lo + 1", lo + 1), ("d_m = hi - 1", hi - 1),
                                           ("d_m = hi", hi)) if d_m == v}
                whole_free |= m == hi
                whole_masked |= m == lo
            if not t["past"] and t["key_from"] < t["ad_from"]:      # the key mask decides d_m; d_free = key_from - 1
                for p in loop_passes(lo, m, t["NP"]) + loop_passes(m, hi, t["NP"]):
                    if len(p) == 2 and p[1] == p[0] + 1 and t["key_from"] - 1 in p:
                        c.add("d_free first" if p[0] == t["key_from"] - 1 else "d_free second")
        if whole_free and whole_masked:
            c.add("free beside masked")
        if t["d_end"] > max(t["ad_from"], t["key_from"], d_lo) and t["x0"] == 0:
            c.add("both masks")
        if t["past"] and t["d_end"] > d_lo:
            c.add("past W")
        if not t["past"] and d_lo < t["d_end"]:
            raw = min(t["ad_from"], t["key_from"])
            if raw < t["d_end"]:
                c.add("slice below d_m" if d_lo < raw else "slice at d_m" if d_lo == raw else "slice above d_m")
    return c


@pytest.mark.parametrize("W,want", [
    (230, {"d_m even", "d_m odd", "d_m = lo", "d_m = hi - 1", "free beside masked", "d_free first", "d_free second"}),
    (232, {"d_m = lo + 1", "d_m even", "d_m odd"}),
    (256, {"d_m = hi", "free beside masked"})])
def test_where_d_m_falls_in_a_wave(env, W, want):
    """r = 5, D = 128: d_m at both ends of a wave's range and one inside either end, at both parities; a wave that
    never enters the masked loop beside one that never leaves it; d_free on either disparity of a pair."""
    assert want <= _cases(W, 5, 0, 128), want - _cases(W, 5, 0, 128)
    L, R = _pair(env, 71, W, H, 64)
    _check(env, L, R, 5, 128)


@pytest.mark.parametrize("d_lo,d_hi,want", [(40, 90, "slice below d_m"), (50, 100, "slice at d_m"),
                                            (60, 110, "slice above d_m"), (17, 81, "slice above d_m")])
def test_slices_around_d_m(env, d_lo, d_hi, want):
    """230 wide, r = 5: the tiles at x0 = 54, 108 and 162 need their first mask at d = 50, 70 and 16."""
    firsts = [min(t["ad_from"], t["key_from"]) for t in _tiles(230, 5, d_lo, d_hi) if not t["past"]]
    assert firsts[1:] == [50, 70, 16]
    assert want in _cases(230, 5, d_lo, d_hi)
    if want == "slice at d_m":
        assert d_lo in firsts
    L, R = _pair(env, 72, 230, H, 64)
    _check_slice(env, L, R, 5, d_lo, d_hi)


def test_both_masks_in_one_tile(env):
    """80 wide (a tile and a half), D = 128 > W: the tile at x0 = 0 has columns left of d and outputs right of
    W - d in the same passes, and the second tile has columns past W."""
    assert {"both masks", "past W"} <= _cases(80, 5, 0, 128)
    L, R = _pair(env, 73, 80, H, 40)
    _check(env, L, R, 5, 128)
    _check_slice(env, L, R, 5, 30, 75)


@pytest.mark.parametrize("W,D", [(217, 256), (159, 128)])
def test_r7_48_column_tiles(env, W, D):
    want = {"d_m even", "d_m odd", "d_m = lo", "free beside masked", "past W", "both masks"}
    assert want <= _cases(W, 7, 0, D), want - _cases(W, 7, 0, D)
    assert geometry(7, 0, D) == (2, 48)
    L, R = _pair(env, 74, W, H, 64)
    _check(env, L, R, 7, D)


@pytest.mark.parametrize("r,W,D", [(2, 127, 32), (2, 133, 32), (1, 129, 24)])
def test_one_d_per_pass_takes_the_same_masks(env, r, W, D):
    """r <= 2, D <= 32: the NP = 1 loop on 64 - 2r columns, split at d_m with no pairing."""
    assert geometry(r, 0, D) == (1, T - 2 * r)
    cases = _cases(W, r, 0, D)
    assert {"past W", "free beside masked"} <= cases and cases & {"d_m = lo + 1", "d_m = hi - 1"}
    L, R = _pair(env, 75 + r, W, H, 24)
    _check(env, L, R, r, D)
    _check_slice(env, L, R, r, 3, 3 + D)


def test_d256_on_300_columns(env):
    """D = 256 on 300 columns: five left-edge tiles, the right-hand ones also cut by d <= W - x."""
    cases = _cases(300, 5, 0, 256)
    assert {"d_m even", "d_m odd", "free beside masked", "past W", "d_free first"} <= cases, cases
    L, R = _pair(env, 79, 300, H, 128)
    _check(env, L, R, 5, 256)
