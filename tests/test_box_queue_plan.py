"""The tile queue's schedule (csrc/bm_box_plan.h: box_queue_grab) on the CPU.  The header is built with g++
alone (tests/native/box_queue_shim.cpp).  For tile grids from 1 x 1 to the headline's 36 x 23 x 128 and 1 to 768
slots the grabs cover every tile exactly once and in order, never grow, end with single tiles, are empty past the
end, and number fewer than 2^31; small grids are also walked grab by grab here, against the rule restated in Python.
And box_queue_workgroups / box_queue_candidate: which launches draw from the queue."""
import ctypes
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SLOTS = (1, 2, 3, 5, 7, 12, 36, 100, 255, 256, 767, 768)
GRIDS = [(1, 1, 1), (1, 2, 1), (2, 1, 1), (2, 2, 1), (3, 2, 1), (4, 3, 1), (4, 3, 3), (5, 2, 3), (1, 23, 2), (36, 1, 1),
         (7, 5, 2), (36, 23, 1), (36, 23, 4), (36, 23, 32), (36, 23, 128), (9, 8, 96), (72, 45, 8), (40, 23, 32)]


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    if not shutil.which("g++"):
        pytest.skip("g++ absent")
    out = str(tmp_path_factory.mktemp("queue") / "libbox_queue_shim.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-o", out,
                    os.path.join(ROOT, "tests", "native", "box_queue_shim.cpp")], check=True)
    lib = ctypes.CDLL(out)
    u = ctypes.c_uint
    lib.box_queue_grab.argtypes = [u, u, u, u, ctypes.POINTER(u)]
    lib.box_queue_grab.restype = None
    lib.box_queue_walk.argtypes = [u, u, u, u, ctypes.POINTER(ctypes.c_ulonglong)]
    lib.box_queue_workgroups.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_longlong] + [ctypes.c_int] * 3
    lib.box_mfma_tiles.argtypes = [ctypes.c_int] * 5
    lib.box_mfma_tiles.restype = ctypes.c_longlong
    lib.box_queue_candidate.argtypes = [ctypes.c_int] * 11
    return lib


def _grab(lib, g, total, tiles_x, slots):
    out = (ctypes.c_uint * 2)()
    lib.box_queue_grab(g, total, tiles_x, slots, out)
    return out[0], out[1]


def _model(total, tiles_x, slots):
    """The rule restated: levels of size tiles_x, tiles_x / 2, .. 2 hand out whole grabs while more than `slots` of
    them remain; what is left goes singly."""
    s, t, out = min(tiles_x, 32768), 0, []
    while s > 1:
        q = (total - t) // s
        for _ in range(max(q - slots, 0)):
            out.append((t, t + s))
            t += s
        s //= 2
    return out + [(i, i + 1) for i in range(t, total)]


@pytest.mark.parametrize("grid", GRIDS)
def test_grabs_cover_in_order_shrink_and_end(lib, grid):
    tiles_x, tiles_y, batch = grid
    total = tiles_x * tiles_y * batch
    for slots in SLOTS:
        out = (ctypes.c_ulonglong * 4)()
        assert lib.box_queue_walk(total, tiles_x, slots, slots + 3, out) == 0, (grid, slots)
        n, first, largest, singles = out
        assert 1 <= n < 2 ** 31 and n <= total
        assert first == largest <= max(tiles_x, 1) and singles >= 1
        # the single tiles at the end are what the last level above them leaves, and its size is 2 or 3
        assert singles <= 3 * slots + 2 or tiles_x == 1


@pytest.mark.parametrize("grid", [g for g in GRIDS if g[0] * g[1] * g[2] <= 1000])
def test_grab_by_grab_against_the_rule(lib, grid):
    tiles_x, tiles_y, batch = grid
    total = tiles_x * tiles_y * batch
    for slots in (1, 2, 5, 36, 768):
        want = _model(total, tiles_x, slots)
        got = [_grab(lib, g, total, tiles_x, slots) for g in range(len(want))]
        assert got == want, (grid, slots)
        for g in (len(want), len(want) + 1, len(want) + slots, 2 ** 31, 2 ** 32 - 1):
            b, e = _grab(lib, g, total, tiles_x, slots)
            assert b == e, (grid, slots, g)


def test_headline_schedule(lib):
    """36 x 23 x 128 tiles on 768 slots: rows first, about nine grabs per slot, and a tail of 2 x 768 single tiles."""
    total = 36 * 23 * 128
    out = (ctypes.c_ulonglong * 4)()
    assert lib.box_queue_walk(total, 36, 768, 768, out) == 0
    n, first, largest, singles = out
    assert first == 36 and singles == 2 * 768
    assert _grab(lib, 0, total, 36, 768) == (0, 36) and _grab(lib, 1, total, 36, 768) == (36, 72)
    assert 8 * 768 <= n <= 10 * 768
    # the largest total the launcher takes
    assert lib.box_queue_walk(2 ** 31 - 1, 36, 768, 4, out) == 0 and out[0] < 2 ** 31


def test_which_launches_draw(lib):
    q = lib.box_queue_workgroups         # np, dspan, tiles, slots, SM_PARAM_BOX_WORKGROUPS, _QUEUE_WORKGROUPS
    assert q(2, 128, 105984, 768, 0, 0) == 768            # the headline: 138 tiles per slot
    assert q(2, 128, 64 * 768, 768, 0, 0) == 768 and q(2, 128, 64 * 768 - 1, 768, 0, 0) == 0
    assert q(2, 128, 26496, 768, 0, 0) == 0 and q(2, 65, 26496, 768, 0, 0) == 0   # 32 frames: 34 tiles per slot, static
    assert q(2, 64, 26496, 768, 0, 0) == 768 and q(2, 8, 26496, 768, 0, 0) == 768  # but the queue for short spans
    assert q(2, 64, 28 * 768, 768, 0, 0) == 768 and q(2, 64, 28 * 768 - 1, 768, 0, 0) == 0
    assert q(2, 64, 6912, 768, 0, 0) == 0                 # 463 x 370 x 96: 9 tiles per slot
    assert q(2, 40, 12, 768, 0, 5) == 5 and q(2, 40, 12, 768, 0, 40) == 40    # an explicit queue size at any launch size
    assert q(2, 128, 105984, 768, 4, 0) == 0 and q(2, 40, 12, 768, 4, 5) == 0  # an explicit range count: static
    assert q(1, 32, 105984, 768, 0, 0) == 0 and q(1, 16, 12, 768, 0, 5) == 0   # one d per pass
    assert q(2, 40, 12, 768, 0, -1) == 0 and q(2, 40, 12, 768, 0, 2 ** 20 + 1) == 0 and q(2, 128, 105984, 0, 0, 0) == 0
    assert lib.box_mfma_tiles(1920, 1080, 5, 128, 128) == 105984
    assert lib.box_mfma_tiles(200, 100, 5, 40, 1) == 12 and lib.box_mfma_tiles(200, 100, 7, 16, 1) == 15
    assert lib.box_mfma_tiles(200, 100, 1, 16, 1) == 4 * 2 and lib.box_mfma_tiles(200, 100, 1, 33, 1) == 4 * 3
    c = lib.box_queue_candidate          # W, H, radius, d_lo, d_hi, batch, valid_mode, cus, box_kernel, n, queue n
    assert c(1920, 1080, 5, 0, 128, 128, 0, 256, 0, 0, 0) == 1
    assert c(1920, 1080, 5, 0, 128, 128, 0, 256, 0, 16, 0) == 0     # explicit ranges
    assert c(1920, 1080, 5, 0, 128, 128, 0, 256, 1, 0, 0) == 0      # the VALU kernels
    assert c(1920, 1080, 5, 0, 128, 1, 0, 256, 0, 0, 0) == 0        # batch 1 stays on the 8-wave tiles
    assert c(200, 100, 5, 0, 40, 1, 0, 256, 2, 0, 0) == 0           # a test frame: static ranges, no counter taken
    assert c(200, 100, 5, 0, 40, 1, 0, 256, 2, 0, 5) == 1           # unless the queue size is explicit
    assert c(200, 100, 1, 0, 16, 1, 0, 256, 2, 0, 5) == 0           # one d per pass
    assert c(200, 100, 8, 0, 40, 1, 0, 256, 2, 0, 5) == 0 and c(200, 100, 5, 0, 40, 1, 1, 256, 2, 0, 5) == 0
