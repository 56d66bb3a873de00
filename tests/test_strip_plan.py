"""csrc/bm_strip_plan.h on the CPU: the strip kernel's launch geometry.  The header is built with g++ alone
(tests/native/strip_plan_shim.cpp) and compared with the rules restated here: the exhaustive (nb, nbe) search the
launcher ran before the header had it, the kernel's own interior test and LDS offsets (bm_strip.hip keeps both
written out, this test ties them to the header), and the staging's items per thread."""
import ctypes
import itertools
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SC = 128            # input columns per strip
EDGE_COST = 150     # an edge strip's row step, in percent of an interior one
RADII = (16, 17, 25, 37)
WIDTHS = (4, 54, 55, 96, 130, 400, 1920, 4097)
HEIGHTS = (1, 2, 63, 64, 65, 333, 1080, 5000)
SLICES = ((0, 1), (0, 64), (20, 64), (64, 200), (0, 256))
FRAMES = (1, 3, 8, 70000)
RESIDENT = (1, 7, 256, 1024, 4096)


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    if not shutil.which("g++"):
        pytest.skip("g++ absent")
    out = str(tmp_path_factory.mktemp("plan") / "libstrip_plan_shim.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-o", out,
                    os.path.join(ROOT, "tests", "native", "strip_plan_shim.cpp")], check=True)
    lib = ctypes.CDLL(out)
    lib.strip_grid.argtypes = [ctypes.c_int] * 8 + [ctypes.POINTER(ctypes.c_int)]
    lib.strip_grid.restype = None
    lib.strip_lds_all.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_void_p]
    return lib


def grid(lib, W, H, r, d_lo, d_hi, vm, frames, resident):
    o = (ctypes.c_int * 5)()
    lib.strip_grid(W, H, r, d_lo, d_hi, vm, frames, resident, o)
    return tuple(o)


def kernel_interior(x0, r, W, d_hi, vm):
    """strip_kernel's col_ok && out_ok (bm_strip.hip)."""
    sw, cs0 = SC - 2 * r, x0 - r
    col_ok = cs0 >= d_hi - 1 and cs0 + SC <= W
    out_ok = x0 + sw <= W and ((d_hi - 1) <= W - (x0 + sw - 1) if vm == 0 else (d_hi - 1) <= x0)
    return col_ok and out_ok


def split(W, r, d_hi, vm):
    """EL, NI, ER as the launcher counted them: the leading strips that are not interior, the run of interior
    strips behind them, the rest."""
    sw = SC - 2 * r
    strips = -(-W // sw)
    el = 0
    while el < strips and not kernel_interior(el * sw, r, W, d_hi, vm):
        el += 1
    ni = 0
    while el + ni < strips and kernel_interior((el + ni) * sw, r, W, d_hi, vm):
        ni += 1
    return el, ni, strips - el - ni


def search(ni, ne, H, r, frames, resident):
    """The exhaustive search: every nb <= H / 4r and nbe <= H / 2r whose workgroups fit `resident` ((1, 1) always
    counts), the first minimum of the longer band walk in nb-major order.  Returns (nb, nbe, (1, 1) fits)."""
    nb = np.arange(1, (max(1, H // (4 * r)) if ni else 1) + 1, dtype=np.int64)[:, None]
    nbe = np.arange(1, (max(1, H // (2 * r)) if ne else 1) + 1, dtype=np.int64)[None, :]
    fits = (ne * nbe + ni * nb) * frames <= resident
    fallback = not fits[0, 0]
    fits[0, 0] = True
    ti = (-(-H // nb) + 2 * r) * 100 if ni else 0 * nb
    te = (-(-H // nbe) + 2 * r) * EDGE_COST if ne else 0 * nbe
    t = np.where(fits, np.maximum(ti, te), np.iinfo(np.int64).max)
    i, j = np.unravel_index(np.argmin(t), t.shape)   # argmin: the first minimum, row-major
    return int(nb[i, 0]), int(nbe[0, j]), fallback


def test_grid_equals_the_exhaustive_search(lib):
    known = {}
    fallbacks = no_interior = 0
    for r, W, (d_lo, d_hi), vm in itertools.product(RADII, WIDTHS, SLICES, (0, 1)):
        el, ni, er = split(W, r, d_hi, vm)
        no_interior += ni == 0
        assert el >= 1   # strip 0's left halo lies outside the frame: no frame is without an edge strip
        for H, frames, resident in itertools.product(HEIGHTS, FRAMES, RESIDENT):
            key = (ni, el + er, H, r, frames, resident)
            if key not in known:
                known[key] = search(*key)
            nb, nbe, fallback = known[key]
            fallbacks += fallback
            assert grid(lib, W, H, r, d_lo, d_hi, vm, frames, resident) == (el, ni, er, nb, nbe), \
                (W, H, r, d_lo, d_hi, vm, frames, resident)
    assert fallbacks > 0 and no_interior > 0


def test_bands_equal_the_exhaustive_search(lib):
    """The band search alone, over strip counts no frame gives as well: no edge strips (EL + ER = 0, which
    strip_grid never passes), no interior strips, up to 40 of either."""
    fallbacks = 0
    o = (ctypes.c_int * 2)()
    for (ni, ne), r, H, frames, resident in itertools.product(
            ((1, 0), (22, 0), (0, 1), (0, 40), (1, 1), (18, 4), (40, 2), (3, 37)), RADII, HEIGHTS, FRAMES, RESIDENT):
        nb, nbe, fallback = search(ni, ne, H, r, frames, resident)
        fallbacks += fallback
        lib.strip_bands(ni, ne, H, r, frames, resident, o)
        assert tuple(o) == (nb, nbe), (ni, ne, H, r, frames, resident)
    assert fallbacks > 0


def test_interior_strips_are_one_run(lib):
    """strip_interior is the kernel's test; the strips it accepts are contiguous, and the three counts add up to
    the frame's strips."""
    for r, W, (d_lo, d_hi), vm in itertools.product(RADII, WIDTHS + (700, 1000), SLICES, (0, 1)):
        sw = SC - 2 * r
        strips = -(-W // sw)
        flags = [bool(lib.strip_interior(st * sw, r, W, d_hi, vm)) for st in range(strips)]
        assert flags == [kernel_interior(st * sw, r, W, d_hi, vm) for st in range(strips)]
        el, ni, er, _, _ = grid(lib, W, 100, r, d_lo, d_hi, vm, 1, 1024)
        assert el + ni + er == strips
        assert flags == [False] * el + [True] * ni + [False] * er, (r, W, d_hi, vm)


@pytest.mark.parametrize("right", (0, 1))
def test_lds_and_staging(lib, right):
    """Every slice 0 <= d_lo < d_hi <= 256 at every radius."""
    d_lo, d_hi = np.array([(a, b) for a in range(256) for b in range(a + 1, 257)]).T
    per_thread = lib.strip_stage_items_per_thread()
    assert per_thread == 3
    worst = 0.0
    for r in range(16, 38):
        o = np.zeros((len(d_lo), 8), np.int32)
        assert lib.strip_lds_all(r, right, o.ctypes.data) == len(d_lo) == 32896
        DP, RW, RS, nw, wmin_off, rrow_off, total, stage = o.T
        sw = SC - 2 * r
        assert np.array_equal(nw, (d_hi - d_lo + 63) // 64)
        assert np.all(RW % 2 == 0) and np.all(RS % 32 == 16) and np.all(RS >= RW)
        assert np.all(DP >= d_hi - 1) and np.all(DP % 4 == 0)
        # a lane's reads end inside its copy: staged columns DP - d .. DP - d + 127, d >= d_lo
        assert np.all(2 * RW >= DP - d_lo + SC)
        # the kernel's nItems: 4-column groups of the L rows (in, out) and of the R rows (in, out), kPF per thread
        items = 2 * 32 + 2 * (RW // 2)
        assert np.all(items <= per_thread * 64 * nw)
        worst = max(worst, float(np.max(items / (64 * nw))))
        # the kernel's offsets (bm_strip.hip: wmin = lds + 2 BUF, rrow = wmin + 2 nw NG 8 words) and the sum of the parts
        assert np.array_equal(stage, 2 * (SC // 2) * 4 + 2 * 2 * RS * 4)
        wmin_bytes = 2 * nw * ((sw + 7) // 8) * 8 * 4
        assert np.array_equal(wmin_off, 2 * stage) and np.array_equal(rrow_off, wmin_off + wmin_bytes)
        assert np.array_equal(total, 2 * stage + wmin_bytes + (2 * (sw + DP) * 4 if right else 0))
        assert np.all(total <= 160 * 1024)
    assert 2.5 < worst < 2.6   # 2.56 items per thread at the worst slice


def test_pinned_grid_1080p(lib):
    """1080p, D = 128, r = 20, 8 frames.  Strips of 88 outputs: 22.  Strip st starts at x0 = 88 st and is interior
    when x0 - 20 >= 127 (st >= 2), x0 - 20 + 128 <= 1920 (st <= 20) and 127 <= 1920 - (x0 + 87) (st <= 19): 2 left
    edge, 18 interior, 2 right edge.  nb <= 1080 / 80 = 13, nbe <= 1080 / 40 = 27; walks (ceil(1080 / n) + 40) x 100
    interior, x 150 edge.
    1024 resident workgroups, 128 per frame: 18 nb + 4 nbe <= 128.  The best of each nb (at the most nbe that fit):
    nb 1: 112000, 2: 58000, 3: 40000, 4: 31000, 5 (nbe <= 9): max(25600, 24000) = 25600, 6 (nbe <= 5):
    max(22000, 38400) = 38400; nb = 7 leaves room for no edge band.  nb = 5, and the first nbe whose walk is within
    25600: nbe = 8 walks 175 x 150 = 26250, nbe = 9 walks 160 x 150 = 24000: (5, 9), 1008 workgroups.
    512 resident, 64 per frame: nb 1: 112000, 2 (nbe <= 7): 58000, 3 (nbe <= 2): max(40000, 87000); nb = 4 does
    not fit.  nb = 2, and nbe = 3 walks 400 x 150 = 60000, nbe = 4 walks 310 x 150 = 46500: (2, 4), 416 workgroups."""
    assert grid(lib, 1920, 1080, 20, 0, 128, 0, 8, 1024) == (2, 18, 2, 5, 9)
    assert grid(lib, 1920, 1080, 20, 0, 128, 0, 8, 512) == (2, 18, 2, 2, 4)
    assert search(18, 4, 1080, 20, 8, 1024)[:2] == (5, 9) and search(18, 4, 1080, 20, 8, 512)[:2] == (2, 4)


def test_args_ok(lib):
    ok = lib.strip_args_ok
    assert ok(4, 1, 16, 0, 1, 1, 0) and ok(1920, 1080, 37, 64, 256, 8, 1)
    for bad in ((3, 1, 16, 0, 1, 1, 0), (4, 0, 16, 0, 1, 1, 0), (4, 1, 15, 0, 1, 1, 0), (4, 1, 38, 0, 1, 1, 0),
                (4, 1, 16, 5, 5, 1, 0), (4, 1, 16, 0, 257, 1, 0), (4, 1, 16, 0, 1, 0, 0), (4, 1, 16, 0, 1, 1, 2)):
        assert not ok(*bad), bad
