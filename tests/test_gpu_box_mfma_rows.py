"""The matrix-pipe box kernel walking ranges of tiles and keeping the right band along a row (bm_box_mfma.hip,
DESIGN §24; SM_PARAM_BOX_WORKGROUPS) against oracle.box_disp / box_keys_slice, against the VALU kernels forced with
set_box_kernel(1), and against the same matrix kernel with one tile per workgroup (n = T): maps and slice keys bit
for bit, with the harness of test_gpu_box_mfma_pairs.py.  Every frame here has fewer tiles than the GPU has
workgroup slots, so only an explicit n makes a workgroup take more than one tile: each shape runs for n in
(1, 2, 3, 4, 7, T, T + 5).  n = 1 crosses every row and frame boundary in one workgroup, small n cut the ranges
mid-row (a fresh band, then carried ones), n >= T carries nothing.  Frames are at most 320 x 70."""
import ctypes

import numpy as np
import pytest

from test_box_mfma_rows_model import dims, walk
from test_gpu_box_mfma_pairs import LEGACY, MATRIX, _check, _check_slice, _keys, _maps, _pair, env  # noqa: F401

pytestmark = pytest.mark.gpu


def _tile_count(W, H, r, d_lo, d_hi, batch=1):
    _, TOX, TOY = dims(r, d_lo, d_hi)[:3]
    return -(-W // TOX), -(-H // TOY), -(-W // TOX) * -(-H // TOY) * batch


def _ns(T):
    return (1, 2, 3, 4, 7, T, T + 5)


def _with_n(env, n, fn, *args, **kw):
    m = env[3]
    m.set_box_workgroups(n)
    try:
        return fn(env, *args, **kw)
    finally:
        m.set_box_workgroups(0)


def _check_every_n(env, L, R, r, D):
    """One frame: maps and keys of [0, D) at every n against the oracle, the VALU kernels and n = T."""
    H, W = L.shape
    T = _tile_count(W, H, r, 0, D)[2]
    got, kg = _check(env, L, R, r, D)              # oracle, VALU kernels, matrix kernel at auto n (= T here)
    at_T = _with_n(env, T, _maps, L, R, r, D, MATRIX), _with_n(env, T, _keys, L, R, r, 0, D, MATRIX)
    assert np.array_equal(at_T[0], got) and np.array_equal(at_T[1], kg)
    for n in _ns(T):
        a = _with_n(env, n, _maps, L, R, r, D, MATRIX)
        assert np.array_equal(a, got), (n, int((a != got).sum()))
        k = _with_n(env, n, _keys, L, R, r, 0, D, MATRIX)
        assert np.array_equal(k, kg), (n, int((k != kg).sum()))
    return T


def _batch_maps(env, Ls, Rs, r, D, kernel, n):
    sm, torch, O, m = env
    m.set_box_kernel(kernel)
    m.set_box_workgroups(n)
    try:
        out = m.match_device(torch.from_numpy(Ls).cuda(), torch.from_numpy(Rs).cuda(), r, D)
        torch.cuda.synchronize()
    finally:
        m.set_box_kernel(0)
        m.set_box_workgroups(0)
    return out.cpu().numpy()


def test_headline_geometry_batch_of_three(env):
    """r = 5, D = 128, 230 x 50 x 3 frames: 5 x 2 tiles per frame, T = 30.  The band reaches left of column 0 on the
    first three tiles of a row and the last tile reaches past W."""
    W, H, D, r, B = 230, 50, 128, 5, 3
    tiles_x, tiles_y, T = _tile_count(W, H, r, 0, D, B)
    assert (tiles_x, tiles_y, T) == (5, 2, 30)
    assert [tx * 54 - r - 128 < 0 for tx in range(5)] == [True, True, True, False, False] and 4 * 54 - r + 64 > W
    # n = 1 carries across every tile of a row and restages at each of the 5 row and frame changes; n = 4 cuts
    # ranges mid-row
    w1, w4 = walk(tiles_x, tiles_y, B, 1), walk(tiles_x, tiles_y, B, 4)
    assert sum(not t[4] for t in w1[0]) == tiles_y * B and any(mine[0][3] != 0 for mine in w4)
    pairs = [_pair(env, 300 + f, W, H, 64) for f in range(B)]
    Ls, Rs = np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])
    want = np.stack([env[2].box_disp(L, R, r, D) for L, R in pairs])
    assert np.array_equal(_batch_maps(env, Ls, Rs, r, D, LEGACY, 0), want)
    assert np.array_equal(_batch_maps(env, Ls, Rs, r, D, MATRIX, T), want)
    for n in _ns(T):
        got = _batch_maps(env, Ls, Rs, r, D, MATRIX, n)
        assert np.array_equal(got, want), (n, [int((got[f] != want[f]).sum()) for f in range(B)])
    # one frame of it with its keys
    assert _check_every_n(env, pairs[0][0], pairs[0][1], r, D) == 10


@pytest.mark.parametrize("W", [54, 50, 108])
def test_one_tile_rows_and_exact_multiples(env, W):
    """W = 54 and 50: one tile per row, every tile a row start, nothing carried at any n.  W = 108: two tiles that
    end exactly on the frame's edge."""
    r, D, H = 5, 40, 70
    tiles_x, tiles_y, T = _tile_count(W, H, r, 0, D)
    assert tiles_x == (2 if W == 108 else 1) and tiles_y == 2
    L, R = _pair(env, 310 + W, W, H, D)
    _check_every_n(env, L, R, r, D)


@pytest.mark.parametrize("r,D,W,tox", [(7, 256, 217, 48), (4, 64, 230, 56), (3, 192, 230, 58), (1, 24, 200, 62),
                                       (2, 32, 200, 60)])
def test_other_geometries(env, r, D, W, tox):
    """r = 7 D = 256 (TOX = 48, three column blocks, the widest band); r = 4 D = 64 (TOX = 56: the new columns are
    whole groups); r = 3 D = 192; r = 1 / 2 at D = 24 / 32 (one d per pass, 62- / 60-row tiles; at r = 1 the carried
    tile has 128 + 128 = 256 staging elements, every thread stages, at r = 2 120 + 128)."""
    dm = dims(r, 0, D)
    assert dm[1] == tox
    if r <= 2:
        assert dm[0] == 1 and 8 * dm[7] + 128 == (256 if r == 1 else 248)
    if r == 4:
        assert (dm[4] - tox) % 4 == 0
    H = 70
    assert _tile_count(W, H, r, 0, D)[0] >= 4 and _tile_count(W, H, r, 0, D)[1] == 2
    L, R = _pair(env, 320 + r, W, H, min(D, 64))
    _check_every_n(env, L, R, r, D)


@pytest.mark.parametrize("d_lo,d_hi", [(40, 90), (100, 140)])
def test_d_slices_with_d_lo(env, d_lo, d_hi):
    """Slices with d_lo > 0 on 230 x 50: the band starts d_lo further left, and stays left of column 0 for longer."""
    W, H, r = 230, 50, 5
    L, R = _pair(env, 331, W, H, 64)
    want = _check_slice(env, L, R, r, d_lo, d_hi)   # oracle, VALU kernels, matrix kernel at auto n
    T = _tile_count(W, H, r, d_lo, d_hi)[2]
    assert np.array_equal(_with_n(env, T, _keys, L, R, r, d_lo, d_hi, MATRIX), want)
    for n in _ns(T):
        k = _with_n(env, n, _keys, L, R, r, d_lo, d_hi, MATRIX)
        assert np.array_equal(k, want), (n, int((k != want).sum()))


@pytest.mark.parametrize("n", [1, 2])
def test_batch_with_pitched_frames(env, n):
    """150 x 70 inside 160 x 72, 3 frames, a frame stride that is not H x pitch, guard bytes 0xAB: nothing outside
    the output slices is written."""
    sm, torch, O, m = env
    from gpu_stereo_matching_amd import _capi
    W, H, D, r, B = 150, 70, 40, 5, 3
    PW, PH = W + 10, H + 2
    pairs = [_pair(env, 50 + f, W, H, D) for f in range(B)]
    bigL = torch.zeros((B, PH, PW), dtype=torch.uint8, device="cuda")
    bigR = torch.zeros_like(bigL)
    for f, (L, R) in enumerate(pairs):
        bigL[f, 1:H + 1, 3:W + 3] = torch.from_numpy(L).cuda()
        bigR[f, 1:H + 1, 3:W + 3] = torch.from_numpy(R).cuda()
    out = torch.full((B, PH, PW), 0xAB, dtype=torch.uint8, device="cuda")
    m.set_box_kernel(MATRIX)
    m.set_box_workgroups(n)
    try:
        _capi.check(m._lib.sm_match_device(
            m._h, bigL[0, 1:, 3:].data_ptr(), bigR[0, 1:, 3:].data_ptr(), W, H, PW, B, PH * PW, r, D, 0,
            out[0, 1:, 3:].data_ptr(), PW, PH * PW, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)))
        torch.cuda.synchronize()
    finally:
        m.set_box_kernel(0)
        m.set_box_workgroups(0)
    res = out.cpu().numpy()
    for f, (L, R) in enumerate(pairs):
        assert np.array_equal(res[f, 1:H + 1, 3:W + 3], O.box_disp(L, R, r, D)), f
    res[:, 1:H + 1, 3:W + 3] = 0xAB
    assert (res == 0xAB).all(), "wrote outside the output slices"


def test_parameter_values_and_scope(env):
    sm, torch, O, m = env
    from gpu_stereo_matching_amd import _capi
    for bad in (-1, 1.5, float("nan")):
        with pytest.raises(_capi.SMError) as e:
            m.set_box_workgroups(bad)
        assert e.value.code == _capi.SM_ERR_INVALID_ARG
    with pytest.raises(_capi.SMError):
        m.set_box_kernel(3)                          # the box-kernel parameter keeps rejecting 3
    L, R = _pair(env, 71, 150, 70, 24)
    want = O.box_disp(L, R, 5, 24)
    m.set_box_workgroups(2)
    m.set_box_workgroups(0)                          # 0 restores auto
    assert np.array_equal(_maps(env, L, R, 5, 24, MATRIX), want)
    # the VALU kernels, and the passes outside the matrix kernel's scope, give the same maps at any n
    for n in (1, 3, 1000):
        assert np.array_equal(_with_n(env, n, _maps, L, R, 5, 24, LEGACY), want), n
        for r, kw in ((0, {}), (8, {}), (5, {"lr_check": True})):
            a = _with_n(env, n, _maps_kw, L, R, r, 24, MATRIX, **kw)
            assert np.array_equal(a, _maps_kw(env, L, R, r, 24, LEGACY, **kw)), (n, r, kw)


def _maps_kw(env, L, R, r, D, kernel, **kw):
    sm, torch, O, m = env
    m.set_box_kernel(kernel)
    try:
        out = m.match_device(torch.from_numpy(L).cuda(), torch.from_numpy(R).cuda(), r, D, **kw)
        torch.cuda.synchronize()
    finally:
        m.set_box_kernel(0)
    return out.cpu().numpy()
