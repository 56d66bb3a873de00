"""CPU tests of the speckle filter (StereoSGBM's speckleWindowSize / speckleRange): the numpy reference against
the literal flood fill, its invariants, the quality it buys on two Middlebury pairs, the host-only parts of the
C ABI and csrc/bm_speckle_plan.h built with g++ alone (tests/native/speckle_plan_shim.cpp)."""
import ctypes
import itertools
import os
import shutil
import subprocess

import numpy as np
import pytest

import sgm_ref
import speckle_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")


def _random_map(seed, dtype):
    """A seeded map up to 23 x 17 of a few close levels and zeros, so that regions of every size appear."""
    rng = np.random.default_rng(seed)
    H, W = int(rng.integers(1, 18)), int(rng.integers(1, 24))
    base = rng.integers(0, 6, (H, W))            # 0 = invalid
    if dtype == np.uint16:
        v = np.where(base > 0, (base + 7) * 16 + rng.integers(0, 16, (H, W)), 0)
    else:
        v = np.where(base > 0, base + 7, 0)
    return v.astype(dtype)


@pytest.mark.parametrize("seed", range(20))
def test_reference_equals_literal_flood_fill(seed):
    dtype = np.uint16 if seed % 2 else np.uint8
    img = _random_map(seed, dtype)
    mask = np.random.default_rng(seed + 100).integers(0, 2, img.shape).astype(np.uint8)
    for max_diff, max_size in itertools.product((0, 1, 2, 16), (0, 1, 3, img.size)):
        got = speckle_ref.speckle(img, max_size, max_diff, mask)
        want = speckle_ref.speckle_literal(img, max_size, max_diff, mask)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), (seed, max_diff, max_size)
        assert got[0].dtype == img.dtype
        if max_size == 0:
            assert np.array_equal(got[0], img) and np.array_equal(got[1], mask)
        if max_size == img.size:
            assert not got[0].any()


def test_labels_are_the_smallest_index_of_the_region():
    img = np.array([[5, 5, 0, 9],
                    [0, 6, 0, 9],
                    [7, 7, 0, 0]], np.uint8)
    lab = speckle_ref.components(img, 1)
    assert lab.tolist() == [[0, 0, -1, 3], [-1, 0, -1, 3], [0, 0, -1, -1]]
    assert speckle_ref.components(img, 0).tolist() == [[0, 0, -1, 3], [-1, 5, -1, 3], [8, 8, -1, -1]]


def test_idempotent():
    for seed in range(6):
        img = _random_map(seed, np.uint8)
        once, _ = speckle_ref.speckle(img, 3, 1)
        twice, _ = speckle_ref.speckle(once, 3, 1)
        assert np.array_equal(once, twice)


def test_joining_is_transitive_along_a_ramp():
    ramp = (10 + 2 * np.arange(20)).astype(np.uint8)[None, :]     # steps of 2: the ends differ by 38
    assert np.array_equal(speckle_ref.speckle(ramp, 19, 2)[0], ramp)          # one region of 20 pixels: kept
    assert not speckle_ref.speckle(ramp, 20, 2)[0].any()                      # removed as a whole
    assert not speckle_ref.speckle(ramp, 1, 1)[0].any()                       # steps above max_diff: 20 single pixels


def test_differences_do_not_wrap():
    a = np.array([[255, 1]], np.uint8)
    assert not speckle_ref.speckle(a, 1, 2)[0].any()                 # |255 - 1| = 254 > 2: two regions of one pixel
    b = np.array([[65535, 3]], np.uint16)
    assert not speckle_ref.speckle(b, 1, 4)[0].any()
    assert np.array_equal(speckle_ref.speckle(b, 1, 65532)[0], b)    # joined: one region of two pixels


def test_quality_on_books_and_art(oracle, gray):
    """The LR-checked AD-SGM maps of sgm_ref at r = 2, D = 80, auto penalties, then speckle(200, 1); bad = |d - gt| > 1
    over gt > 0 and d > 0 with gt = disp1.png / 3.  Measured: Books 0.2148 (128,608 kept) -> 0.1903, 4,090 pixels
    removed; Art 0.3242 (113,646 kept) -> 0.2664, 10,705 removed."""
    gts = np.load(os.path.join(GOLDEN, "middlebury_gt.npz"))
    for name in ("Books", "Art"):
        gt = gts[name + "/disp1"].astype(np.float64) / 3.0
        L, R = gray[name + "/view1"], gray[name + "/view5"]
        checked = sgm_ref.sgm_lr(oracle, L, R, 2, 80, *sgm_ref.auto_penalties(2))[2]
        filtered, _ = speckle_ref.speckle(checked, 200, 1)

        def rate(d):
            m = (gt > 0) & (d > 0)
            return float((np.abs(d[m] - gt[m]) > 1).mean()), int(m.sum())

        (b0, n0), (b1, n1) = rate(checked), rate(filtered)
        removed = int(((checked != 0) & (filtered == 0)).sum())
        print(f"{name} r=2 D=80 bad-pixel rate: LR-checked {b0:.4f} ({n0} kept), + speckle(200, 1) {b1:.4f} "
              f"({n1} kept), {removed} pixels removed")
        assert b1 < b0 and removed > 0


# ---- the C ABI without a device ----
def test_symbols_and_constants():
    import gpu_stereo_matching_amd as sm
    from gpu_stereo_matching_amd import _capi
    lib = _capi.load()
    names = ("sm_speckle_workspace_bytes", "sm_speckle_filter_device", "sm_speckle_filter_u8", "sm_speckle_filter_u16")
    hdr = open(os.path.join(ROOT, "include", "sm_hip.h")).read()
    for n in names:
        assert hasattr(lib, n) and n in _capi.EXPORTED and n + "(" in hdr, n
    assert _capi.SM_PARAM_SPECKLE_SIZE == 9 and _capi.SM_PARAM_SPECKLE_RANGE == 10
    assert "SM_PARAM_SPECKLE_SIZE = 9" in hdr and "SM_PARAM_SPECKLE_RANGE = 10" in hdr
    for n in ("set_speckle", "speckle_filter", "speckle_filter_device"):
        assert hasattr(sm.BlockMatcher, n), n
    assert hasattr(sm.BlockMatcherGroup, "set_speckle") and "speckle_workspace_bytes" in sm.__all__


def test_invalid_arguments_without_a_device():
    from gpu_stereo_matching_amd import _capi
    lib = _capi.load()
    INVALID = _capi.SM_ERR_INVALID_ARG
    err = lib.sm_last_error_string
    buf = (ctypes.c_uint8 * 4096)()
    m = ctypes.addressof(buf)

    def dev(elem=1, W=8, H=8, pitch=8, batch=1, stride=64, size=1, diff=1, ptr=m):
        return lib.sm_speckle_filter_device(None, ptr, elem, W, H, pitch, batch, stride, size, diff, None, None)

    # the arguments' own rules come first and need no handle; a call that passes them reports the null handle
    assert dev() == INVALID and b"null handle" in err()
    for kw, word in (({"elem": 0}, b"elem_bytes"), ({"elem": 3}, b"elem_bytes"), ({"elem": 4}, b"elem_bytes"),
                     ({"W": 0}, b"frame size"), ({"H": -1}, b"frame size"), ({"batch": 0}, b"batch"),
                     ({"pitch": 7}, b"pitch"), ({"size": -1}, b"max_size"), ({"diff": -1}, b"max_diff"),
                     ({"diff": 256}, b"max_diff"), ({"elem": 2, "diff": 65536}, b"max_diff"), ({"ptr": None}, b"null map"),
                     ({"batch": 2, "stride": 63}, b"strides overlap"), ({"W": 65536, "H": 32768, "pitch": 65536}, b"2^31")):
        assert dev(**kw) == INVALID and word in err() and b"speckle" in err(), kw
    assert dev(diff=255) == INVALID and b"null handle" in err()
    assert dev(elem=2, diff=65535) == INVALID and b"null handle" in err()
    assert dev(size=0) == INVALID and b"null handle" in err()      # max_size 0 is legal, and still needs a handle
    assert dev(batch=2, stride=64) == INVALID and b"null handle" in err()
    for fn, top in ((lib.sm_speckle_filter_u8, 255), (lib.sm_speckle_filter_u16, 65535)):
        host = lambda W=8, H=8, pitch=8, size=1, diff=1, ptr=m, mask=None, mp=8: \
            fn(None, ptr, W, H, pitch, size, diff, mask, mp)   # noqa: E731
        assert host() == INVALID and b"null handle" in err()
        assert host(diff=top) == INVALID and b"null handle" in err()
        for kw, word in (({"W": 0}, b"frame size"), ({"pitch": 7}, b"pitch"), ({"size": -1}, b"max_size"),
                         ({"diff": -1}, b"max_diff"), ({"diff": top + 1}, b"max_diff"), ({"ptr": None}, b"null map"),
                         ({"mask": m, "mp": 7}, b"mask_pitch")):
            assert host(**kw) == INVALID and word in err() and b"speckle" in err(), kw
    for p in (_capi.SM_PARAM_SPECKLE_SIZE, _capi.SM_PARAM_SPECKLE_RANGE):
        assert lib.sm_set_param_f(None, p, 1.0) == INVALID
        assert lib.sm_group_set_param_f(None, p, 1.0) == INVALID
    # the workspace function: host-only
    n = ctypes.c_size_t(7)
    assert lib.sm_speckle_workspace_bytes(8, 8, 1, None) == INVALID
    for W, H, B in ((0, 8, 1), (8, 0, 1), (8, 8, 0), (-1, 8, 1), (65536, 32768, 1)):
        assert lib.sm_speckle_workspace_bytes(W, H, B, ctypes.byref(n)) == INVALID and n.value == 0, (W, H, B)
        assert b"speckle" in err()
    assert lib.sm_speckle_workspace_bytes(46341, 46340, 1, ctypes.byref(n)) == _capi.SM_OK   # < 2^31 pixels


def test_workspace_bytes_follow_the_formula():
    import gpu_stereo_matching_amd as sm
    up = lambda v: (v + 255) // 256 * 256   # noqa: E731
    for W, H, B in ((1, 1, 1), (67, 65, 1), (67, 65, 3), (463, 370, 2), (1920, 1080, 1), (1920, 1080, 8),
                    (1920, 1080, 9), (1920, 1080, 100)):
        assert sm.speckle_workspace_bytes(W, H, B) == 2 * up(4 * W * H * min(B, 8)), (W, H, B)
    assert sm.speckle_workspace_bytes(1920, 1080) == 16588800          # 8 B per pixel
    assert sm.speckle_workspace_bytes(1920, 1080, 100) == 132710400    # groups of 8 frames
    with pytest.raises(sm.SMError, match="speckle"):
        sm.speckle_workspace_bytes(0, 5)


# ---- the plan header ----
@pytest.fixture(scope="module")
def plan(tmp_path_factory):
    if not shutil.which("g++"):
        pytest.skip("g++ absent")
    out = str(tmp_path_factory.mktemp("splan") / "libspeckle_plan_shim.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-shared", "-fPIC", "-o", out,
                    os.path.join(ROOT, "tests", "native", "speckle_plan_shim.cpp")], check=True)
    lib = ctypes.CDLL(out)
    lib.speckle_constants.argtypes = [ctypes.POINTER(ctypes.c_int)]
    lib.speckle_constants.restype = None
    lib.speckle_plan.argtypes = [ctypes.c_int] * 3 + [ctypes.POINTER(ctypes.c_longlong)]
    lib.speckle_plan.restype = None
    lib.speckle_ok.argtypes = [ctypes.c_int] * 3
    lib.speckle_ok.restype = ctypes.c_int
    return lib


def plan_constants(plan):
    o = (ctypes.c_int * 4)()
    plan.speckle_constants(o)
    return list(o)


def plan_of(plan, W, H, batch=1):
    o = (ctypes.c_longlong * 8)()
    plan.speckle_plan(W, H, batch, o)
    return list(o)


def test_plan_sizes(plan):
    TW, TH, T, G = plan_constants(plan)
    assert (TW, TH, T, G) == (32, 32, 256, 8) and (TW * TH) % T == 0
    up = lambda v: (v + 255) // 256 * 256   # noqa: E731
    cases = [(1, 1), (TW, TH), (TW + 1, TH), (TW, TH + 1), (TW + 1, TH + 1), (2 * TW + 3, 2 * TH + 1), (1, 3 * TW + 1),
             (3 * TH + 1, 1), (1920, 1080)]
    for (W, H), B in itertools.product(cases, (1, 3, 8, 9)):
        tx, ty = -(-W // TW), -(-H // TH)
        pairs = (tx - 1) * H + (ty - 1) * W
        g = min(B, G)
        plane = up(4 * W * H * g)
        assert plan_of(plan, W, H, B) == [tx, ty, pairs, -(-pairs // T), -(-W * H // T), g, plane, 2 * plane], (W, H, B)
    # pinned, by hand
    assert plan_of(plan, 1, 1) == [1, 1, 0, 0, 1, 1, 256, 512]
    assert plan_of(plan, 32, 32) == [1, 1, 0, 0, 4, 1, 4096, 8192]                 # one tile exactly: no seam pass
    assert plan_of(plan, 33, 32) == [2, 1, 32, 1, 5, 1, 4352, 8704]                # one tile + 1 column: 32 pairs
    assert plan_of(plan, 1920, 1080) == [60, 34, 59 * 1080 + 33 * 1920, 497, 8100, 1, 8294400, 16588800]
    assert plan_of(plan, 1920, 1080, 20)[5:] == [8, 66355200, 132710400]


def test_plan_accepts(plan):
    ok = lambda W=64, H=32, B=1: plan.speckle_ok(W, H, B) == 1   # noqa: E731
    assert ok() and ok(1, 1, 1) and ok(B=1000)
    assert not ok(W=0) and not ok(H=0) and not ok(B=0) and not ok(W=-3)
    assert ok(46341, 46340) and not ok(46341, 46341)      # 2^31 - 1 pixels at most: labels are 32-bit indices
    assert plan_of(plan, 0, 5) == [0] * 8                 # a refused frame plans nothing


def test_plan_matches_the_library(plan):
    import gpu_stereo_matching_amd as sm
    for W, H, B in ((1, 1, 1), (67, 65, 3), (1920, 1080, 9)):
        assert sm.speckle_workspace_bytes(W, H, B) == plan_of(plan, W, H, B)[7]
