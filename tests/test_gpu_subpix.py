"""GPU sub-pixel disparities (1/16 px, uint16), the uniqueness filter and the reprojection against the numpy
restatement of their contract (tests/subpix_ref.py).

Integer arithmetic end to end, so every map and mask comparison is bit-exact; the reprojection is compared with a
float64 evaluation at rtol = 1e-5 (the kernel evaluates in double and rounds once to fp32, 2^-24)."""
import ctypes
import functools
import os

import numpy as np
import pytest

import subpix_ref
from conftest import GOLDEN

pytestmark = pytest.mark.gpu

SHAPES = [   # W, H, D, r
    (67, 9, 16, 2),     # odd width, one partial block
    (37, 11, 64, 0),    # W < D: dmax clamps at every pixel, and the right view's pair set bites
    (300, 5, 256, 7),   # a second x-block, q > 255, the widest window
    (64, 8, 1, 2),      # D = 1 and D = 2: no interior d, q == 16 d0 everywhere
    (64, 8, 2, 0),
]
PATHS = [("box", "ad"), ("box", "census"), ("sgm", "ad"), ("sgm", "census")]
TOP = (1 << 24) - 1


@pytest.fixture(scope="module")
def sm_mod():
    import gpu_stereo_matching_amd as sm
    return sm


@pytest.fixture(scope="module")
def matcher(sm_mod):
    m = sm_mod.BlockMatcher(0, 640, 370, 256)
    yield m
    m.close()


@functools.lru_cache(maxsize=None)
def _pair(W, H, D, kind, seed=0):
    """kind 'synth': oracle.synth_pair with +-4 noise on the right image; 'random': a random texture and its copy
    shifted by 3 columns with +-30 noise, so that the AD box threshold splits the frame."""
    from oracle import oracle as O
    seed = seed or (W * 131 + H * 17 + D)
    rng = np.random.default_rng(seed)
    if kind == "synth":
        L, R = O.synth_pair(seed, W, H, D)
        R = np.clip(R.astype(np.int64) + rng.integers(-4, 5, R.shape), 0, 255).astype(np.uint8)
    else:
        L = rng.integers(0, 256, (H, W)).astype(np.uint8)
        R = np.roll(L, -3, axis=1)
        R = np.clip(R.astype(np.int64) + rng.integers(-30, 31, R.shape), 0, 255).astype(np.uint8)
    L.setflags(write=False)
    R.setflags(write=False)
    return L, R


@functools.lru_cache(maxsize=None)
def _volume(W, H, D, r, kind, agg, cost, seed=0):
    """(V, invalid_from, right_pairs) of the reference, computed once per case and shared."""
    from oracle import oracle as O
    O.build()
    L, R = _pair(W, H, D, kind, seed)
    V, inv, pairs = subpix_ref.volume(O, L, R, r, D, agg, cost)
    V.setflags(write=False)
    return V, inv, pairs


def _u16(t):
    return t.cpu().numpy().view(np.uint16)


@pytest.mark.parametrize("agg,cost", PATHS)
@pytest.mark.parametrize("kind", ["random", "synth"])
@pytest.mark.parametrize("W,H,D,r", SHAPES)
def test_paths(matcher, W, H, D, r, kind, agg, cost):
    L, R = _pair(W, H, D, kind)
    V, inv, pairs = _volume(W, H, D, r, kind, agg, cost)
    d8 = matcher.match(L, R, r, D, agg=agg, cost=cost)
    c8, _, m8 = matcher.match_lr(L, R, r, D, agg=agg, cost=cost)
    try:
        for u in (0, 10):
            matcher.set_uniqueness(u)
            for lr in (False, True):
                q, qr, mask = matcher.match_subpix(L, R, r, D, agg=agg, cost=cost, lr_check=lr, return_right=True,
                                                   return_mask=True)
                wq, wqr, wmask = subpix_ref.subpix(V, u, inv, lr, pairs)
                assert np.array_equal(q, wq) and np.array_equal(qr, wqr) and np.array_equal(mask, wmask)
                assert np.array_equal(matcher.match_subpix(L, R, r, D, agg=agg, cost=cost, lr_check=lr), wq)
                # d8 is the unchecked 8-bit map: with u > 0 a right-view pixel that the filter drops counts as
                # d0 = 0 in the check, so a pixel the 8-bit check occludes can pass here
                assert (np.abs(q.astype(np.int64) - 16 * d8.astype(np.int64))[mask == 1] <= 8).all()
                assert not q[mask == 0].any()
                if D <= 2:
                    assert not (q % 16).any() and not (qr % 16).any()
                if u == 0 and lr:
                    assert np.array_equal(mask, m8)
                    assert (np.abs(q.astype(np.int64) - 16 * c8.astype(np.int64)) <= 8).all()
    finally:
        matcher.set_uniqueness(0)


def test_device_pitch_and_strided_batch(matcher):
    """Frames with pitch > width, a batch of 2 whose frames and maps are not dense, and the optional outputs."""
    import torch
    W, H, D, r, B = 67, 9, 16, 2, 2
    pairs = [_pair(W, H, D, "synth", seed=900 + b) for b in range(B)]
    big_l = torch.zeros((B, H + 3, W + 13), dtype=torch.uint8, device="cuda")
    big_r = torch.full((B, H + 3, W + 13), 255, dtype=torch.uint8, device="cuda")
    for b in range(B):
        big_l[b, :H, :W] = torch.from_numpy(pairs[b][0].copy()).cuda()
        big_r[b, :H, :W] = torch.from_numpy(pairs[b][1].copy()).cuda()
    Lt, Rt = big_l[:, :H, :W], big_r[:, :H, :W]
    for agg, cost in PATHS:
        for lr in (False, True):
            big_o = torch.full((B, H + 2, W + 5), -1, dtype=torch.int16, device="cuda")
            out = big_o[:, :H, :W]
            rt = torch.empty((B, H, W), dtype=torch.int16, device="cuda")
            mt = torch.empty((B, H, W), dtype=torch.uint8, device="cuda")
            got = matcher.match_subpix_device(Lt, Rt, r, D, out_t=out, agg=agg, cost=cost, lr_check=lr, right_t16=rt,
                                              mask_t=mt)
            single = matcher.match_subpix_device(Lt[1], Rt[1], r, D, agg=agg, cost=cost, lr_check=lr)
            torch.cuda.synchronize()
            assert got.data_ptr() == out.data_ptr()
            for b in range(B):
                V, inv, rp = _volume(W, H, D, r, "synth", agg, cost, seed=900 + b)
                wq, wqr, wmask = subpix_ref.subpix(V, 0, inv, lr, rp)
                assert np.array_equal(_u16(out[b].contiguous()), wq)
                assert np.array_equal(_u16(rt[b]), wqr) and np.array_equal(mt[b].cpu().numpy(), wmask)
            assert np.array_equal(_u16(single), _u16(out[1].contiguous()))
            pad = big_o.clone()
            pad[:, :H, :W] = -1
            assert bool((pad == -1).all())   # nothing written outside the maps


def _crafted(dtype):
    """A [D, H, W] volume of crafted columns at x = 0 .. 7 (every d exists there) over a random background."""
    D, H, W = 6, 3, 40
    top = TOP if dtype == np.uint32 else 65535
    rng = np.random.default_rng(17)
    V = rng.integers(0, 50, (D, H, W)).astype(np.int64)
    V[:, :, 0] = 7                                            # all equal: q = 0
    V[:, :, 1] = np.array([9, 9, 3, 3, 9, 9])[:, None]        # plateau: delta = +8
    V[:, :, 2] = np.array([top, 1, 0, top, top, top])[:, None]    # a = 1, c = top: -8, the largest numerator
    V[:, :, 3] = np.array([top, top, 0, top, top, top])[:, None]  # den = 2 top
    V[:, :, 4] = np.array([top, top, 0, 0, top, top])[:, None]    # plateau at the top of the range
    V[:, :, 5] = np.array([top, top, top - 1, top, top, top])[:, None]
    V[:, :, 6] = np.array([500, 400, 90, 400, 100, 500])[:, None]   # uniqueness 10: the tie, valid
    V[:, :, 7] = np.array([500, 400, 90, 400, 99, 500])[:, None]    # one less: invalid
    return V


@pytest.mark.parametrize("dtype", [np.uint16, np.uint32])
def test_volume_wta_on_crafted_volumes(matcher, dtype):
    import torch
    V = _crafted(dtype)
    D, H, W = V.shape
    vt = torch.from_numpy(V.astype(dtype).view(np.int16 if dtype == np.uint16 else np.int32)).cuda()
    try:
        for u in (0, 10):
            matcher.set_uniqueness(u)
            for inv in (0, 90, 91):   # the crafted b = 90 on the boundary: b >= 90 invalid, b >= 91 valid
                for lr in (False, True):
                    rt = torch.empty((H, W), dtype=torch.int16, device="cuda")
                    mt = torch.empty((H, W), dtype=torch.uint8, device="cuda")
                    q = _u16(matcher.volume_wta_subpix_device(vt, inv, lr, right_t16=rt, mask_t=mt))
                    wq, wqr, wmask = subpix_ref.subpix(V, u, inv, lr, 1)
                    assert np.array_equal(q, wq) and np.array_equal(_u16(rt), wqr)
                    assert np.array_equal(mt.cpu().numpy(), wmask)
                    if not lr and inv == 0:
                        assert not q[:, 0].any()
                        assert (q[:, 1] == 40).all() and (q[:, 2] == 24).all() and (q[:, 3] == 32).all()
                        assert (q[:, 4] == 40).all() and (q[:, 6] == 32).all()
                        for x in (5, 7):   # rivals within 10 % of the best
                            assert (q[:, x] == (32 if u == 0 else 0)).all()
                            assert (mt.cpu().numpy()[:, x] == (u == 0)).all()
                    if not lr and inv:
                        assert (mt.cpu().numpy()[:, 6] == (inv == 91)).all()
    finally:
        matcher.set_uniqueness(0)


def test_uniqueness_parameter_is_checked(matcher, sm_mod):
    from gpu_stereo_matching_amd import _capi
    for bad in (-1, 100, 2.5):
        assert matcher._lib.sm_set_param_f(matcher._h, _capi.SM_PARAM_UNIQUENESS, float(bad)) == 1
        assert b"uniqueness" in matcher._lib.sm_last_error_string()
    matcher.set_uniqueness(99)
    matcher.set_uniqueness(0)
    with sm_mod.BlockMatcherGroup([0], 64, 64, 16) as g:
        assert g._lib.sm_group_set_param_f(g._g, _capi.SM_PARAM_UNIQUENESS, 10.0) == 0
        assert g._lib.sm_group_set_param_f(g._g, _capi.SM_PARAM_UNIQUENESS, 100.0) == 1
    L, R = _pair(67, 9, 16, "synth")
    q = np.empty(L.shape, np.uint16)
    with pytest.raises(sm_mod.SMError, match="SM_MEDIAN"):
        _capi.check(matcher._lib.sm_block_match_subpix_u16(matcher._h, L.ctypes.data, R.ctypes.data, 67, 9, 67, 2, 16,
                                                           sm_mod.SM_AGG_SGM | sm_mod.SM_MEDIAN, q.ctypes.data, None,
                                                           None, 67))
    for agg in ("guided", "box-staged", "device-cu"):
        with pytest.raises(sm_mod.SMError, match="no cost volume"):
            matcher.match_subpix(L, R, 2, 16, agg=agg)
    with pytest.raises(sm_mod.SMError, match="radius"):
        matcher.match_subpix(L, R, 8, 16)
    with pytest.raises(sm_mod.SMError, match="null"):
        _capi.check(matcher._lib.sm_block_match_subpix_u16(matcher._h, L.ctypes.data, R.ctypes.data, 67, 9, 67, 2, 16,
                                                           0, None, None, None, 67))


def test_reproject(matcher, sm_mod):
    import torch
    from gpu_stereo_matching_amd import calib
    K1, K2, d1, d2, R, T = calib.load_data_batch(os.path.join(GOLDEN, "Calib_Data_OpenCV.yml"))
    Q = np.asarray(calib.stereo_rectify(K1, d1, K2, d2, (320, 200), R, T)[4], np.float64).reshape(4, 4)
    W, H = 300, 7   # a second x-block
    rng = np.random.default_rng(4)
    q = rng.integers(1, 4089, (H, W)).astype(np.uint16)
    q[rng.random((H, W)) < 0.2] = 0
    q[0, 0], q[H - 1, W - 1], q[1, 255], q[1, 256] = 0, 4088, 1, 0
    xs, ys = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64))
    vec = np.stack([xs, ys, q.astype(np.float64) / 16.0, np.ones_like(xs)], axis=-1) @ Q.T
    assert (vec[..., 3][q > 0] != 0).all()
    want = np.where((q > 0)[..., None], vec[..., :3] / np.where(vec[..., 3:] == 0, 1.0, vec[..., 3:]), 0.0)
    got = matcher.reproject(q, Q)
    assert got.dtype == np.float32 and got.shape == (H, W, 3)
    assert np.allclose(got, want, rtol=1e-5, atol=0.0)
    assert not got[q == 0].any()
    # device form, a map with pitch > width
    big = torch.zeros((H, W + 9), dtype=torch.int16, device="cuda")
    big[:, :W] = torch.from_numpy(q.view(np.int16)).cuda()
    pts = matcher.reproject_device(big[:, :W], Q)
    torch.cuda.synchronize()
    assert np.array_equal(pts.cpu().numpy(), got)
    f = sm_mod.to_float(big[:, :W])
    assert np.array_equal(f.cpu().numpy(), sm_mod.to_float(q))


def test_non_default_stream_and_stream_sync(matcher):
    import torch
    W, H, D, r = 67, 9, 16, 2
    L, R = _pair(W, H, D, "synth")
    V, inv, rp = _volume(W, H, D, r, "synth", "sgm", "ad")
    want = subpix_ref.subpix(V, 0, inv, True, rp)
    Lt, Rt = torch.from_numpy(L.copy()).cuda(), torch.from_numpy(R.copy()).cuda()
    torch.cuda.synchronize()
    st = torch.cuda.Stream()
    mt = torch.empty((H, W), dtype=torch.uint8, device="cuda")
    out = matcher.match_subpix_device(Lt, Rt, r, D, agg="sgm", lr_check=True, mask_t=mt, stream=st)
    assert matcher._lib.sm_stream_sync(matcher._h, ctypes.c_void_p(st.cuda_stream)) == 0
    assert np.array_equal(_u16(out), want[0]) and np.array_equal(mt.cpu().numpy(), want[2])
