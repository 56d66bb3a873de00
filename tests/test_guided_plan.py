"""csrc/bm_guided_plan.h on the CPU: the guided pass's tile geometry, the right view's workspace size and what the
launcher accepts.  The header is built with g++ alone (tests/native/guided_plan_shim.cpp) and compared with the
formulas restated here: 32-row tiles of 64 - 4r columns, 8 S2H segments per row, a right-key chain of
D + 8 * segment - 1 steps, 4 bytes per step and tile row."""
import ctypes
import itertools
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

RADII = range(8)
HEIGHTS = (1, 32, 33)
DISPS = (1, 32, 33, 256)
BATCHES = (1, 3)
REDUCE_BOUNDS = (4, 6, 8, 10)   # the instantiated guided_right_reduce_kernel<32, MAXT>


@pytest.fixture(scope="module")
def plan(tmp_path_factory):
    if not shutil.which("g++"):
        pytest.skip("g++ absent")
    out = str(tmp_path_factory.mktemp("gplan") / "libguided_plan_shim.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-o", out,
                    os.path.join(ROOT, "tests", "native", "guided_plan_shim.cpp")], check=True)
    lib = ctypes.CDLL(out)
    lib.guided_geometry.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_int)]
    lib.guided_geometry.restype = None
    lib.guided_partial_bytes.argtypes = [ctypes.c_int] * 5
    lib.guided_partial_bytes.restype = ctypes.c_ulonglong
    lib.guided_ok.argtypes = [ctypes.c_int] * 6
    lib.guided_ok.restype = ctypes.c_int
    return lib


def tile_w(r):
    return 64 - 4 * r


def widths(r):
    return (1, tile_w(r) - 1, tile_w(r), tile_w(r) + 1, 4096)


def geometry(r, D):
    tw = tile_w(r)
    sw2 = (tw + 7) // 8
    span = 8 * sw2
    K = D + span - 1
    return [tw, 32, sw2, span, K, (K + tw - 1) // tw + 1]


def partial_bytes(W, H, r, D, batch):
    tw, th, _, _, K, _ = geometry(r, D)
    return -(-W // tw) * -(-H // th) * batch * K * th * 4


def test_geometry_and_bytes_follow_the_formulas(plan):
    seen = set()
    for r, D in itertools.product(RADII, DISPS):
        o = (ctypes.c_int * 6)()
        plan.guided_geometry(r, D, o)
        assert list(o) == geometry(r, D), (r, D)
        assert o[5] <= max(REDUCE_BOUNDS), (r, D)
        seen.add(min(b for b in REDUCE_BOUNDS if o[5] <= b))
        for W, H, batch in itertools.product(widths(r), HEIGHTS, BATCHES):
            assert plan.guided_partial_bytes(W, H, r, D, batch) == partial_bytes(W, H, r, D, batch), (W, H, r, D, batch)
    # every instantiated reduce is some case's
    assert seen == set(REDUCE_BOUNDS)
    o = (ctypes.c_int * 6)()
    plan.guided_geometry(7, 256, o)
    assert o[5] == 10   # the worst case, by hand: K = 256 + 40 - 1 = 295, TW = 36: ceil(295 / 36) + 1


def test_no_workspace_outside_the_kernel_radii(plan):
    for r in (-1, 8):
        assert plan.guided_partial_bytes(1920, 1080, r, 128, 1) == 0


def test_pinned_workspace_sizes(plan):
    # r = 5: TW = 44, segments of 6, K = D + 47
    assert plan.guided_partial_bytes(1920, 1080, 5, 128, 1) == 44 * 34 * 175 * 32 * 4 == 33510400
    assert plan.guided_partial_bytes(3840, 2160, 5, 192, 8) == 88 * 68 * 8 * 239 * 32 * 4 == 1464500224


def test_what_the_launcher_accepts(plan):
    ok = lambda W=64, H=32, r=5, lo=0, hi=64, batch=1: plan.guided_ok(W, H, r, lo, hi, batch) == 1  # noqa: E731
    assert ok()
    assert ok(r=0) and ok(r=7) and not ok(r=-1) and not ok(r=8)
    assert ok(lo=0, hi=1) and ok(lo=255, hi=256) and ok(lo=0, hi=256)
    assert not ok(lo=-1, hi=5) and not ok(lo=5, hi=5) and not ok(lo=6, hi=5) and not ok(lo=0, hi=257)
    assert not ok(lo=256, hi=257) and not ok(lo=0, hi=0)
    assert ok(W=1, H=1) and not ok(W=0) and not ok(H=0) and not ok(batch=0) and not ok(W=-3)
