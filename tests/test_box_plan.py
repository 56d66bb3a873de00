"""plan_box_pass (csrc/bm_box_plan.h): which kernels a box-aggregation pass runs and the workspace it takes, on the
CPU.  The header is built with g++ alone (tests/native/box_plan_shim.cpp) and compared with the selection rules
restated here: tile kernels up to r = 15, the strip kernel at r 16..37, the separable wide path, the direct kernel,
and where the right view comes from; and box_tile_kernel, which kernel a left-only tile pass launches."""
import ctypes
import itertools
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NONE, MAP, KEYS = 0, 1, 2                       # RightWant
TILE, STRIP, WIDE, DIRECT = 0, 1, 2, 3          # BoxLeft
R_NONE, FUSED, MIRRORED, UNSUPPORTED = 0, 1, 2, 3   # BoxRight

RADII = (0, 7, 8, 15, 16, 37, 38, 127)
# (W, H, pitch): every width at a small height, a pitch wider than the frame, and 4096-column frames of exactly
# 2^31 bytes (past the wide path's 32-bit offsets) and one row less
FRAMES = [(w, 6, w) for w in (3, 4, 64, 4096, 4097)] + [(64, 6, 80), (4096, 524288, 4096), (4096, 524287, 4096)]
SLICES = ((0, 64), (20, 64), (0, 256))
BATCHES = (1, 3)


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    if not shutil.which("g++"):
        pytest.skip("g++ absent")
    out = str(tmp_path_factory.mktemp("plan") / "libbox_plan_shim.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-o", out,
                    os.path.join(ROOT, "tests", "native", "box_plan_shim.cpp")], check=True)
    lib = ctypes.CDLL(out)
    lib.box_plan.argtypes = [ctypes.c_int] * 8 + [ctypes.POINTER(ctypes.c_ulonglong)]
    lib.box_plan.restype = None
    lib.box_tile_kernel.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_longlong] + [ctypes.c_int] * 3
    return lib


@pytest.fixture(scope="module")
def plan(lib):
    def call(W, H, pitch, radius, d_lo, d_hi, batch, want):
        o = (ctypes.c_ulonglong * 5)()
        lib.box_plan(W, H, pitch, radius, d_lo, d_hi, batch, want, o)
        return dict(left=o[0], right=o[1], rpart=o[2], vol=o[3], mirror=o[4])
    return call


def partial_bytes(W, H, r, D, batch):
    """The fused right view's per-tile right-key partials: 32-row tiles of 64 - 2r columns, rows of
    TW + dmax + 1 keys behind up to 4 pad slots, rounded to 4 entries."""
    dspan = (D + 7) & ~7
    dmax = 64 if dspan <= 64 else 128 if dspan <= 128 else 192 if dspan <= 192 else 256
    tw = 64 - 2 * r
    pwp = (tw + dmax + 1 + 7 + 3) & ~3
    return -(-W // tw) * -(-H // 32) * batch * 32 * pwp * 4


def wide_bytes(W, H, D, batch):
    """The wide path's u16 V planes of one launch group: at most 8 frames, 4.5 GB, and ~8192 row blocks."""
    plane = W * H * D * 2
    group = max(1, min(-(-8192 // H), batch, 8, max(1, (4608 << 20) // max(plane, 1))))
    return group * D * W * H * 2


def expected(W, H, pitch, r, d_lo, d_hi, batch, want):
    D = d_hi - d_lo
    e = dict(left=TILE, right=R_NONE, rpart=0, vol=0, mirror=0)
    if r <= 15:
        if want != NONE:
            e.update(right=FUSED, rpart=partial_bytes(W, H, r, D, batch))
        return e
    strip_ok = 16 <= r <= 37 and W >= 4 and H >= 1 and d_lo < d_hi <= 256
    wide_ok = 4 <= W <= 4096 and pitch * H < 2 ** 31
    if want == NONE and strip_ok:
        e.update(left=STRIP)
    elif want == MAP and wide_ok and strip_ok:
        e.update(left=STRIP, right=FUSED, vol=4 * W * H * batch)
    elif wide_ok:
        e.update(left=WIDE, right=R_NONE if want == NONE else FUSED, vol=wide_bytes(W, H, D, batch))
    elif want == NONE:
        e.update(left=DIRECT)
    elif want == MAP:
        e.update(left=STRIP if strip_ok else DIRECT, right=MIRRORED, mirror=2)
    else:
        e.update(left=None, right=UNSUPPORTED)   # no left pass runs: the callers reject the call
    return e


def cases():
    return itertools.product(RADII, FRAMES, SLICES, BATCHES, (NONE, MAP, KEYS))


def test_plan_follows_the_table(plan):
    seen = set()
    for r, (W, H, pitch), (d_lo, d_hi), batch, want in cases():
        got = plan(W, H, pitch, r, d_lo, d_hi, batch, want)
        want_plan = expected(W, H, pitch, r, d_lo, d_hi, batch, want)
        if want_plan["left"] is None:
            got["left"] = None
        assert got == want_plan, (W, H, pitch, r, d_lo, d_hi, batch, want)
        seen.add((got["left"], got["right"]))
    # every row of the table is reached
    assert seen == {(TILE, R_NONE), (TILE, FUSED), (STRIP, R_NONE), (STRIP, FUSED), (WIDE, R_NONE), (WIDE, FUSED),
                    (DIRECT, R_NONE), (STRIP, MIRRORED), (DIRECT, MIRRORED), (None, UNSUPPORTED)}


def test_strip_without_right_view_takes_no_workspace(plan):
    n = 0
    for r, (W, H, pitch), (d_lo, d_hi), batch, want in cases():
        p = plan(W, H, pitch, r, d_lo, d_hi, batch, want)
        if p["left"] == STRIP and p["right"] == R_NONE:
            assert p["vol"] == 0 and p["rpart"] == 0 and p["mirror"] == 0, (W, H, pitch, r, d_lo, d_hi, batch)
            n += 1
    assert n > 0
    # the d-slice member of ADVICE r6: 1080p, D = 256 over 2 members, r 16..37, no LR
    for r in (16, 20, 37):
        for lo, hi in ((0, 128), (128, 256)):
            p = plan(1920, 1080, 1920, r, lo, hi, 1, NONE)
            assert (p["left"], p["vol"], p["rpart"]) == (STRIP, 0, 0)


def test_pinned_workspace_sizes(plan):
    p = plan(1920, 1080, 1920, 5, 0, 128, 1, MAP)
    assert (p["left"], p["right"]) == (TILE, FUSED)
    assert p["rpart"] == 36 * 34 * 32 * 192 * 4 == 30081024 and p["vol"] == 0
    for want in (NONE, MAP):
        p = plan(1920, 1080, 1920, 40, 0, 128, 8, want)
        assert p["left"] == WIDE
        assert p["vol"] == 8 * 128 * 1920 * 1080 * 2 == 4246732800 and p["rpart"] == 0


PLAIN, MID8, WIDE16, MATRIX = 0, 1, 2, 3        # BoxTileKernel


def tile_kernel(r, span, tiles, cus, box_kernel, scope):
    """Which kernel a left-only tile pass launches: the forced matrix kernel inside its scope first, then 16-wave
    tiles (r <= 7, at most one tile per CU, >= 32 d pairs), 8-wave tiles (r <= 7, at most 8 tiles per CU, >= 16
    pairs), the matrix kernel by itself past 8 tiles per CU, else the 4-wave kernel."""
    npairs = ((span + 7) & ~7) // 2
    if scope and box_kernel == 2:
        return MATRIX
    if r <= 7:
        if tiles <= cus and npairs >= 32:
            return WIDE16
        if tiles <= 8 * cus and npairs >= 16:
            return MID8
    if scope and box_kernel == 0 and tiles > 8 * cus:
        return MATRIX
    return PLAIN


def test_tile_kernel_follows_the_rule(lib):
    seen = set()
    for cus in (256, 7):
        for r, span, tiles, box_kernel, scope in itertools.product(
                (0, 1, 7, 8, 15), (8, 31, 32, 64, 128), (cus - 1, cus, cus + 1, 8 * cus, 8 * cus + 1), (0, 1, 2),
                (0, 1)):
            got = lib.box_tile_kernel(r, span, tiles, cus, box_kernel, scope)
            assert got == tile_kernel(r, span, tiles, cus, box_kernel, scope), (r, span, tiles, cus, box_kernel, scope)
            seen.add(got)
    assert seen == {PLAIN, MID8, WIDE16, MATRIX}
    # the headline (1080p D = 128 r = 5: 36 x 34 tiles of 54 x 32) on 256 CUs: batch 1 on 8-wave tiles, a batch of
    # frames on the matrix kernel unless the VALU kernels are forced; 2^31 - 1 tiles stay in range
    assert lib.box_tile_kernel(5, 128, 36 * 34, 256, 0, 1) == MID8
    assert lib.box_tile_kernel(5, 128, 36 * 34 * 8, 256, 0, 1) == MATRIX
    assert lib.box_tile_kernel(5, 128, 36 * 34 * 8, 256, 1, 1) == PLAIN
    assert lib.box_tile_kernel(5, 128, 2 ** 31 - 1, 256, 0, 1) == MATRIX


def test_matrix_scope(lib):
    """The matrix-pipe kernel takes the left view at r 1..7, valid_mode 0, slices inside [0, 256]."""
    for r, (d_lo, d_hi), vm in itertools.product(range(0, 10), ((0, 1), (0, 256), (20, 64), (0, 257), (5, 5), (-1, 8)),
                                                 (0, 1)):
        want = 1 <= r <= 7 and vm == 0 and 0 <= d_lo < d_hi <= 256
        assert bool(lib.box_mfma_scope(r, d_lo, d_hi, vm)) == want, (r, d_lo, d_hi, vm)
