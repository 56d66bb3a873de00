"""The matrix-pipe box kernel (bm_box_mfma.hip, SM_PARAM_BOX_KERNEL 2) against oracle.box_disp (Device.cu:34-64,
BlockMatching.cpp:111-189) and against the VALU kernels forced with set_box_kernel(1): maps and keys bit-exact.
Shapes are the smallest at which it can go wrong: several 64 - 2r tiles each way with partial last tiles, columns
left of d, D not a multiple of 8, right-edge tiles whose d range the d <= W - x rule cuts, worst-case sums at
r = 7 (the f16 bias bound and the 2^24 key bound), all-tie frames, pitched batches and d-slices with d_lo > 0."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
LEGACY, MATRIX = 1, 2


@pytest.fixture(scope="module")
def env():
    import torch
    import gpu_stereo_matching_amd as sm
    from oracle import oracle as O
    with sm.BlockMatcher(0, 320, 96, 256) as m:
        yield sm, torch, O, m


def _maps(env, L, R, r, D, kernel, **kw):
    sm, torch, O, m = env
    m.set_box_kernel(kernel)
    try:
        out = m.match_device(torch.from_numpy(L).cuda(), torch.from_numpy(R).cuda(), r, D, **kw)
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
    kg, ko = _keys(env, L, R, r, 0, D, MATRIX), _keys(env, L, R, r, 0, D, LEGACY)
    assert np.array_equal(ko, want_keys)
    assert np.array_equal(kg, want_keys), f"{int((kg != want_keys).sum())} keys differ from the oracle"
    return got


def _pair(env, seed, W, H, D):
    L, R = env[0].synth_pair(seed, W, H, D)
    return np.ascontiguousarray(L), np.ascontiguousarray(R)


def test_several_tiles_partial_edges(env):
    """150 x 70, D = 40, r = 5: 3 x 2 tiles of 54, partial right and bottom tiles, columns c < d, D % 8 != 0."""
    L, R = _pair(env, 11, 150, 70, 40)
    got = _check(env, L, R, 5, 40)
    assert len(np.unique(got)) > 8    # a textured pair: the map is not all threshold zeros


@pytest.mark.parametrize("r", range(1, 8))
def test_every_radius(env, r):
    L, R = _pair(env, 20 + r, 130, 70, 24)
    _check(env, L, R, r, 24)


@pytest.mark.parametrize("W,D", [(200, 128), (300, 256)])
def test_validity_rule_cuts_the_range(env, W, D):
    """d <= W - x cuts most disparities; the right-edge tiles skip the d that no output of theirs can take."""
    L, R = _pair(env, 31, W, 40, min(D, 64))
    _check(env, L, R, 5, D)


@pytest.mark.parametrize("D", [1, 9])
def test_tiny_ranges(env, D):
    L, R = _pair(env, 41, 100, 50, max(D, 2))
    _check(env, L, R, 3, D)


@pytest.mark.parametrize("kind", ["hi_lo", "lo_hi", "checker"])
def test_worst_case_sums_r7(env, kind):
    H, W = 60, 80
    if kind == "checker":
        L = (((np.arange(H)[:, None] + np.arange(W)[None, :]) & 1) * 255).astype(np.uint8)
        R = (255 - L).astype(np.uint8)
    else:
        L = np.full((H, W), 255 if kind == "hi_lo" else 0, np.uint8)
        R = np.full((H, W), 0 if kind == "hi_lo" else 255, np.uint8)
    _check(env, L, R, 7, 16)
    # the same sums through d-slices that start past 0 (the c < d columns widen, the keys carry d >= d_lo)
    O = env[2]
    for d_lo, d_hi in ((1, 16), (5, 9)):
        want = O.box_keys_slice(L, R, 7, d_lo, d_hi)
        assert np.array_equal(_keys(env, L, R, 7, d_lo, d_hi, MATRIX), want)


def test_constant_frames_all_ties(env):
    """Every d ties at cost 0: the smallest valid d wins (Device.cu:57), here and in a slice with d_lo > 0."""
    L = np.full((50, 120), 77, np.uint8)
    got = _check(env, L, L.copy(), 4, 32)
    assert not got.any()
    k = _keys(env, L, L.copy(), 4, 3, 20, MATRIX)
    assert np.array_equal(k, env[2].box_keys_slice(L, L.copy(), 4, 3, 20))
    assert (k[:, :120 - 3] == 3).all()


def test_batch_with_pitched_frames(env):
    """3 frames, inputs and outputs slices of larger tensors: pitch != W, frame stride != H * pitch."""
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
    res = {}
    for kernel in (LEGACY, MATRIX):
        out = torch.full((B, PH, PW), 0xAB, dtype=torch.uint8, device="cuda")
        m.set_box_kernel(kernel)
        try:
            _capi.check(m._lib.sm_match_device(
                m._h, bigL[0, 1:, 3:].data_ptr(), bigR[0, 1:, 3:].data_ptr(), W, H, PW, B, PH * PW, r, D, 0,
                out[0, 1:, 3:].data_ptr(), PW, PH * PW, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)))
            torch.cuda.synchronize()
        finally:
            m.set_box_kernel(0)
        res[kernel] = out.cpu().numpy()
    for f, (L, R) in enumerate(pairs):
        want = O.box_disp(L, R, r, D)
        for kernel in (LEGACY, MATRIX):
            assert np.array_equal(res[kernel][f, 1:H + 1, 3:W + 3], want), (kernel, f)
    guard = res[MATRIX].copy()
    guard[:, 1:H + 1, 3:W + 3] = 0xAB
    assert (guard == 0xAB).all(), "wrote outside the output slices"


def test_slice_keys_with_d_lo(env):
    L, R = _pair(env, 61, 150, 70, 40)
    for d_lo, d_hi in ((16, 40), (7, 8), (100, 140)):
        a, b = _keys(env, L, R, 5, d_lo, d_hi, MATRIX), _keys(env, L, R, 5, d_lo, d_hi, LEGACY)
        assert np.array_equal(a, b), (d_lo, d_hi)
        assert np.array_equal(a, env[2].box_keys_slice(L, R, 5, d_lo, d_hi))


def test_parameter_values_and_scope(env):
    sm, torch, O, m = env
    from gpu_stereo_matching_amd import _capi
    for bad in (3, -1, 1.5):
        with pytest.raises(_capi.SMError) as e:
            m.set_box_kernel(bad)
        assert e.value.code == _capi.SM_ERR_INVALID_ARG
    L, R = _pair(env, 71, 150, 70, 24)
    # outside the matrix kernel's scope the VALU kernels answer
    for r, kw in ((0, {}), (8, {}), (5, {"lr_check": True})):
        assert np.array_equal(_maps(env, L, R, r, 24, MATRIX, **kw), _maps(env, L, R, r, 24, LEGACY, **kw)), (r, kw)
    assert np.array_equal(_maps(env, L, R, 0, 24, MATRIX), O.box_disp(L, R, 0, 24))
    assert np.array_equal(_maps(env, L, R, 8, 24, MATRIX), O.box_disp(L, R, 8, 24))
