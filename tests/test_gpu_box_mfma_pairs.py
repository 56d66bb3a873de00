"""The matrix-pipe box kernel's paired loop and 48-row tiles (bm_box_mfma.hip; SM_PARAM_BOX_KERNEL 2)
against oracle.box_disp / box_keys_slice and against the VALU kernels forced with set_box_kernel(1): maps and keys
bit-exact.  Each wave walks its share of the d range two disparities per pass and folds both keys of a pixel with
one min3, so the shapes are the smallest at which that can go wrong: tile seams at 48 rows and 64 - 2r columns (48
at r = 7), wave ranges of 0, 1, 2 and 3 disparities, d-slices, right-edge tiles whose range the d <= W - x rule cuts
to an odd length, a pair whose second disparity is masked for some columns while its first is valid for all,
columns left of d that differ within a pair, ties within a pair, every radius, the r = 7 bounds, and a pitched
batch.  Ranges of at most 32 disparities at r <= 2 take one d per pass on 64 - 2r rows: both sides of that rule
are run."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
LEGACY, MATRIX = 1, 2
TILE_H, WAVES = 48, 4   # bm_box_mfma.hip: MG::TOY, kNW


def _tile_w(r):
    """bm_box_mfma.hip's MG::TOX: four column blocks cut at 64 - 2r, three full ones at r = 7."""
    return 64 - 2 * r if r <= 6 else 48


@pytest.fixture(scope="module")
def env():
    import torch
    import gpu_stereo_matching_amd as sm
    from oracle import oracle as O
    with sm.BlockMatcher(0, 320, 100, 256) as m:
        yield sm, torch, O, m


def _maps(env, L, R, r, D, kernel):
    sm, torch, O, m = env
    m.set_box_kernel(kernel)
    try:
        out = m.match_device(torch.from_numpy(L).cuda(), torch.from_numpy(R).cuda(), r, D)
        torch.cuda.synchronize()
    finally:
        m.set_box_kernel(0)
    return out.cpu().numpy()


def _keys(env, L, R, r, d_lo, d_hi, kernel):
    sm, torch, O, m = env
    m.set_box_kernel(kernel)
    try:
        k = m.slice_keys_device(torch.from_numpy(L).cuda(), torch.from_numpy(R).cuda(), r, d_lo, d_hi)
        torch.cuda.synchronize()
    finally:
        m.set_box_kernel(0)
    return k.cpu().numpy().view(np.uint32)


def _check(env, L, R, r, D):
    O = env[2]
    want, want_keys = O.box_disp(L, R, r, D, want_keys=True)
    got, old = _maps(env, L, R, r, D, MATRIX), _maps(env, L, R, r, D, LEGACY)
    assert np.array_equal(old, want)
    assert np.array_equal(got, want), f"{int((got != want).sum())} pixels differ from the oracle"
    kg = _keys(env, L, R, r, 0, D, MATRIX)
    assert np.array_equal(kg, want_keys), f"{int((kg != want_keys).sum())} keys differ from the oracle"
    return got, kg


def _check_slice(env, L, R, r, d_lo, d_hi):
    want = env[2].box_keys_slice(L, R, r, d_lo, d_hi)
    got = _keys(env, L, R, r, d_lo, d_hi, MATRIX)
    assert np.array_equal(_keys(env, L, R, r, d_lo, d_hi, LEGACY), want), (d_lo, d_hi)
    assert np.array_equal(got, want), (d_lo, d_hi, int((got != want).sum()))
    return got


def _pair(env, seed, W, H, D):
    L, R = env[0].synth_pair(seed, W, H, D)
    return np.ascontiguousarray(L), np.ascontiguousarray(R)


def _wave_passes(W, r, d_lo, d_hi):
    """(x0, d_free, first d, second d or None) of every loop pass of every wave of one row of tiles, by the
    kernel's own arithmetic: the range [d_lo, min(d_hi, W - x0 + 1)) split over the waves, walked in pairs."""
    out = []
    TILE_W = _tile_w(r)
    for x0 in range(0, W, TILE_W):
        d_end = min(d_hi, W - x0 + 1)
        nd = max(d_end - d_lo, 0)
        d_free = W - (min(x0 + TILE_W, W) - 1)
        for w in range(WAVES):
            lo, hi = d_lo + (w * nd) // WAVES, d_lo + ((w + 1) * nd) // WAVES
            out += [(x0, d_free, d, d + 1 if d + 1 < hi else None) for d in range(lo, hi, 2)]
    return out


@pytest.mark.parametrize("r,W,H", [(5, 150, 100), (5, 3 * 54, 2 * TILE_H), (5, 2 * 54 + 1, TILE_H + 1),
                                   (7, 3 * 48, 2 * TILE_H), (7, 2 * 48 + 1, TILE_H + 1)])
def test_tile_seams(env, r, W, H):
    """D = 40: several tiles each way; partial last tiles, frames that end exactly on a seam of 48 rows and of 54
    (r = 5) or 48 (r = 7) columns, and frames one pixel past it."""
    assert W <= 150 or W % _tile_w(r) in (0, 1)
    L, R = _pair(env, 11, W, H, 40)
    got, _ = _check(env, L, R, r, 40)
    assert len(np.unique(got)) > 8    # a textured pair: the map is not all threshold zeros


@pytest.mark.parametrize("r", [1, 2])
@pytest.mark.parametrize("D", [32, 33])
def test_small_radius_both_loops(env, r, D):
    """r <= 2 on 130 x 100: D = 32 is the longest range on the 64 - 2r-row tiles with one d per pass (two tiles each
    way), D = 33 the shortest on the 48-row tiles of the paired loop (62 / 60 columns); a slice on either side."""
    L, R = _pair(env, 80 + r, 130, 100, 32)
    _check(env, L, R, r, D)
    _check_slice(env, L, R, r, 3, D + 2)
    _check_slice(env, L, R, r, 5, 5 + D)


@pytest.mark.parametrize("D", [1, 2, 3, 5, 6, 7, 9, 13, 40])
def test_wave_ranges_odd_single_empty(env, D):
    """r = 3 on 100 x 50: with four waves these D give waves that own 0, 1, 2 and 3 disparities."""
    L, R = _pair(env, 41, 100, 50, max(D, 2))
    _check(env, L, R, 3, D)


def test_wave_range_sizes_covered():
    sizes = set()
    for D in (1, 2, 3, 5, 6, 7, 9, 13, 40):
        sizes |= {((w + 1) * D) // WAVES - (w * D) // WAVES for w in range(WAVES)}
    assert {0, 1, 2, 3} <= sizes


@pytest.mark.parametrize("d_lo,d_hi", [(7, 8), (3, 20), (16, 40), (100, 141)])
def test_d_slices(env, d_lo, d_hi):
    L, R = _pair(env, 61, 200, 60, 40)
    _check_slice(env, L, R, 5, d_lo, d_hi)


@pytest.mark.parametrize("D", [128, 256])
@pytest.mark.parametrize("W", [200, 201, 300])
def test_right_edge_cuts_the_range(env, W, D):
    """d <= W - x cuts the range of the right-hand tiles: odd per-tile and per-wave lengths, partly valid d."""
    passes = _wave_passes(W, 5, 0, D)
    assert any(b is None for _, _, _, b in passes), "no wave ends on a single disparity"
    # a pair whose first d is valid for every output of its tile and whose second is masked for some columns
    assert any(b is not None and a == d_free for _, d_free, a, b in passes)
    L, R = _pair(env, 31, W, 50, 64)
    _check(env, L, R, 5, D)


def test_columns_left_of_d(env):
    """The tile at x0 = 0 with D past the tile width: c >= d selects differ for the two disparities of a pair."""
    L, R = _pair(env, 43, 100, 50, 64)
    _check(env, L, R, 3, 70)
    _check_slice(env, L, R, 3, 33, 70)


def test_ties_within_a_pair(env):
    """Constant frames (every d ties at 0) and frames a constant apart (every d ties at 10 * (2r+1)^2 where no
    column is left of d): the smaller d of a pair wins (Device.cu:57), also in slices with d_lo > 0."""
    r, W, H = 4, 120, 50
    L = np.full((H, W), 77, np.uint8)
    got, _ = _check(env, L, L.copy(), r, 32)
    assert not got.any()
    k = _check_slice(env, L, L.copy(), r, 3, 20)
    assert (k[:, :W - 3] == 3).all()
    R = np.full((H, W), 67, np.uint8)
    for d_lo, d_hi in ((0, 32), (3, 20), (4, 21)):
        k = _check_slice(env, L, R, r, d_lo, d_hi)
        # windows wholly inside the image and right of every d of the slice: all d tie, d_lo wins
        inner = k[r:H - r, d_hi + r:W - d_hi - r]
        assert (inner == ((10 * (2 * r + 1) ** 2) << 8 | d_lo)).all()


@pytest.mark.parametrize("r", range(1, 8))
def test_every_radius(env, r):
    L, R = _pair(env, 20 + r, 130, 100, 24)
    _check(env, L, R, r, 24)


@pytest.mark.parametrize("kind", ["hi_lo", "lo_hi", "checker"])
def test_worst_case_sums_r7(env, kind):
    """The f16 bias bound and the 2^24 key bound on 100 x 100: three 48-row tiles each way."""
    H, W = 100, 100
    if kind == "checker":
        L = (((np.arange(H)[:, None] + np.arange(W)[None, :]) & 1) * 255).astype(np.uint8)
        R = (255 - L).astype(np.uint8)
    else:
        L = np.full((H, W), 255 if kind == "hi_lo" else 0, np.uint8)
        R = np.full((H, W), 0 if kind == "hi_lo" else 255, np.uint8)
    _check(env, L, R, 7, 16)
    _check_slice(env, L, R, 7, 5, 10)


def test_batch_with_pitched_frames(env):
    """3 frames, inputs and outputs slices of larger tensors: pitch != W, frame stride != H * pitch; nothing
    outside the output slices changes."""
    sm, torch, O, m = env
    from gpu_stereo_matching_amd import _capi
    W, H, D, r, B = 150, 98, 41, 5, 3
    PW, PH = W + 10, H + 2
    pairs = [_pair(env, 50 + f, W, H, D) for f in range(B)]
    bigL = torch.zeros((B, PH, PW), dtype=torch.uint8, device="cuda")
    bigR = torch.zeros_like(bigL)
    for f, (L, R) in enumerate(pairs):
        bigL[f, 1:H + 1, 3:W + 3] = torch.from_numpy(L).cuda()
        bigR[f, 1:H + 1, 3:W + 3] = torch.from_numpy(R).cuda()
    out = torch.full((B, PH, PW), 0xAB, dtype=torch.uint8, device="cuda")
    m.set_box_kernel(MATRIX)
    try:
        _capi.check(m._lib.sm_match_device(
            m._h, bigL[0, 1:, 3:].data_ptr(), bigR[0, 1:, 3:].data_ptr(), W, H, PW, B, PH * PW, r, D, 0,
            out[0, 1:, 3:].data_ptr(), PW, PH * PW, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)))
        torch.cuda.synchronize()
    finally:
        m.set_box_kernel(0)
    res = out.cpu().numpy()
    for f, (L, R) in enumerate(pairs):
        assert np.array_equal(res[f, 1:H + 1, 3:W + 3], O.box_disp(L, R, r, D)), f
    res[:, 1:H + 1, 3:W + 3] = 0xAB
    assert (res == 0xAB).all(), "wrote outside the output slices"
