"""CPU tests of semi-global matching (SM_AGG_SGM): the numpy reference against the literal definition, its
invariants, the host-only parts of the C ABI and the quality the definition buys on a Middlebury pair."""
import ctypes
import os

import numpy as np
import pytest

import sgm_ref

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _noisy_pair(oracle, seed, W, H, D):
    """oracle.synth_pair with +-4 noise on the right image, so that costs are not degenerate."""
    L, R = oracle.synth_pair(seed, W, H, D)
    noise = np.random.default_rng(seed).integers(-4, 5, R.shape)
    return L, np.clip(R.astype(np.int64) + noise, 0, 255).astype(np.uint8)


@pytest.mark.parametrize("radius", [0, 1])
def test_scans_equal_literal_triple_loop(oracle, radius):
    W, H, D = 13, 7, 6
    L, R = _noisy_pair(oracle, 5 + radius, W, H, D)
    C = oracle.box_cost(L, R, radius, D).astype(np.int64)
    P1, P2 = 3 * (radius + 1), 11 * (radius + 1)   # small against the costs, so every term of the min is taken somewhere
    for rho in sgm_ref.DIRECTIONS:
        assert np.array_equal(sgm_ref.path(C, rho, P1, P2), sgm_ref.path_literal(C, rho, P1, P2)), rho
    S, disp = sgm_ref.aggregate(C, P1, P2)
    S2, disp2 = sgm_ref.aggregate(C, P1, P2, path_fn=sgm_ref.path_literal)
    assert np.array_equal(S, S2) and np.array_equal(disp, disp2)


def test_zero_penalties_give_four_times_the_cost(oracle):
    W, H, D, r = 41, 19, 12, 1
    L, R = _noisy_pair(oracle, 11, W, H, D)
    C = oracle.box_cost(L, R, r, D).astype(np.int64)
    S, disp = sgm_ref.aggregate(C, 0, 0)
    E = np.broadcast_to(sgm_ref.exists(D, W)[:, None, :], C.shape)
    assert np.array_equal(S[E], 4 * C[E])
    assert np.all(S[~E] == sgm_ref.SENTINEL)
    box = np.argmin(np.where(E, C, sgm_ref.SENTINEL), axis=0)   # the thresholdless box argmin
    assert np.array_equal(disp, box)


def test_path_cost_is_bounded_by_cost_plus_p2(oracle):
    W, H, D, r = 37, 23, 16, 2
    L, R = _noisy_pair(oracle, 3, W, H, D)
    C = oracle.box_cost(L, R, r, D).astype(np.int64)
    P1, P2 = sgm_ref.auto_penalties(r)
    E = np.broadcast_to(sgm_ref.exists(D, W)[:, None, :], C.shape)
    for rho in sgm_ref.DIRECTIONS:
        Lr = sgm_ref.path(C, rho, P1, P2)
        assert np.all(Lr[E] <= C[E] + P2) and np.all(Lr[E] >= C[E])
        assert np.all(Lr[~E] == sgm_ref._INF)


def test_symbols_and_constants():
    import gpu_stereo_matching_amd as sm
    from gpu_stereo_matching_amd import _capi
    lib = _capi.load()
    assert hasattr(lib, "sm_sgm_workspace_bytes") and hasattr(lib, "sm_sgm_check")
    assert _capi.SM_AGG_SGM == 32 and _capi.SM_PARAM_SGM_P1 == 4 and _capi.SM_PARAM_SGM_P2 == 5
    assert sm._flags("sgm", True, True) == sm.SM_AGG_SGM | sm.SM_LR_CHECK | sm.SM_MEDIAN
    hdr = open(os.path.join(os.path.dirname(GOLDEN), "..", "include", "sm_hip.h")).read()
    assert "SM_AGG_SGM = 32u" in hdr and "SM_PARAM_SGM_P1 = 4" in hdr and "SM_PARAM_SGM_P2 = 5" in hdr


def test_workspace_bytes():
    import gpu_stereo_matching_amd as sm
    W, H, D = 1920, 1080, 128
    P = W * H
    n = sm.sgm_workspace_bytes(W, H, D, 2)
    assert 6 * P * D + 4 * P <= n <= 6 * P * D + 4 * P + 3 * 256   # S u32 + SAD u16 + right keys, 256-B aligned
    assert sm.sgm_workspace_bytes(W, H, D, 2, p2=0) == sm.sgm_workspace_bytes(W, H, D, 2, p2=800)
    with pytest.raises(sm.SMError):
        sm.sgm_workspace_bytes(W, H, D, 7, p2=8161)
    with pytest.raises(sm.SMError):
        sm.sgm_workspace_bytes(W, H, 257, 2)
    assert _rc_ws(64, 64, 16, 2, 0, None) == 1   # null output pointer


def _up(n):
    return (n + 255) // 256 * 256


@pytest.mark.parametrize("W,H,D,sgm,census_box,census_sgm", [
    (37, 5, 3, 4352, 5888, 7424),                           # every part a non-multiple of 256
    (320, 256, 64, 31784960, 17367040, 33095680),
    (1920, 1080, 128, 1600819200, 837734400, 1633996800),
])
def test_workspace_layout_totals(W, H, D, sgm, census_box, census_sgm):
    """The volume workspace's one layout (volume_layout, csrc/sm_handle.h) through the exported functions, no
    device needed: the totals are the sums of their 256-B aligned parts, and equal the values the library gave
    before the SGM and census layouts were merged (the literals)."""
    import gpu_stereo_matching_amd as sm
    P = W * H
    assert sm.sgm_workspace_bytes(W, H, D, 2) == _up(4 * P * D) + _up(2 * P * D) + _up(4 * P) == sgm
    assert sm.census_workspace_bytes(W, H, D, 2) == \
        _up(P * D) + _up(2 * P * D) + _up(4 * P) + 2 * _up(8 * P) == census_box
    assert sm.census_workspace_bytes(W, H, D, 2, agg="sgm") == sgm + 2 * _up(8 * P) == census_sgm


def _rc_ws(W, H, D, r, p2, out):
    from gpu_stereo_matching_amd import _capi
    return _capi.load().sm_sgm_workspace_bytes(W, H, D, r, p2, out)


@pytest.mark.parametrize("radius", range(8))
def test_auto_penalties(radius):
    import gpu_stereo_matching_amd as sm
    win2 = (2 * radius + 1) ** 2
    assert sm.sgm_penalties(radius) == (8 * win2, 32 * win2) == sgm_ref.auto_penalties(radius)
    assert sm.sgm_penalties(radius, 5, 0) == (5, 32 * win2)
    assert sm.sgm_penalties(radius, 0, 8 * win2) == (8 * win2, 8 * win2)
    assert sm.sgm_penalties(radius, 7, 9) == (7, 9)


def test_invalid_arguments_without_a_device():
    from gpu_stereo_matching_amd import _capi
    lib = _capi.load()
    SGM, INVALID = _capi.SM_AGG_SGM, _capi.SM_ERR_INVALID_ARG

    def rc(width, radius, flags, p1, p2):
        return lib.sm_sgm_check(width, radius, flags, p1, p2, None, None)

    assert rc(640, 2, SGM, 0, 0) == _capi.SM_OK
    assert rc(640, 2, SGM, 900, 800) == INVALID and b"P1" in lib.sm_last_error_string()
    assert rc(640, 2, SGM, 0, 100) == INVALID            # the auto P1 = 200 exceeds P2 = 100
    assert rc(640, 2, SGM, -1, 800) == INVALID and b"negative" in lib.sm_last_error_string()
    assert rc(640, 7, SGM, 0, 8160) == _capi.SM_OK       # 255 * 225 + 8160 = 65535
    assert rc(640, 7, SGM, 0, 8161) == INVALID and b"65535" in lib.sm_last_error_string()
    assert rc(640, 2, SGM, 0, 65535 - 255 * 25) == _capi.SM_OK
    assert rc(640, 2, SGM, 0, 65536 - 255 * 25) == INVALID
    assert rc(640, 8, SGM, 0, 0) == INVALID and b"radius" in lib.sm_last_error_string()
    assert rc(4096, 2, SGM, 0, 0) == _capi.SM_OK
    assert rc(4097, 2, SGM, 0, 0) == INVALID and b"width" in lib.sm_last_error_string()
    for other in (_capi.SM_AGG_GUIDED, _capi.SM_STAGED, _capi.SM_DEVICE_CU_GRID):
        assert rc(640, 2, SGM | other, 0, 0) == INVALID
        assert b"does not combine" in lib.sm_last_error_string()
    # the entry points themselves, on the null-handle path the other argument tests use
    assert lib.sm_block_match_u8(None, None, None, 10, 10, 10, 1, 8, SGM, None, 10) == INVALID
    assert lib.sm_set_param_f(None, _capi.SM_PARAM_SGM_P1, 8.0) == INVALID
    # the calls that cannot honour the flag say why before they touch a device
    assert lib.sm_group_block_match_u8(None, None, None, 8, 8, 8, 1, 8, SGM, None, 8) == INVALID
    p1 = ctypes.c_int()
    assert lib.sm_sgm_check(640, 3, SGM, 0, 0, ctypes.byref(p1), None) == _capi.SM_OK and p1.value == 8 * 49


def test_python_layers_accept_and_reject_sgm():
    import torch
    import gpu_stereo_matching_amd as sm
    from gpu_stereo_matching_amd import sharding
    assert sm._flags("sgm", False) == sm.SM_AGG_SGM
    a = torch.zeros((64, 32), dtype=torch.uint8)
    with pytest.raises(ValueError, match="sgm"):
        sharding.band_disparity(None, a, a, 2, 16, 0, 32, agg="sgm")
    with pytest.raises(ValueError, match="agg must be"):
        sharding._match_dslice_lr(None, a, a, 2, 16, 0, 2, None, None, None, None, "rs_ag", "sgm", None)


def test_quality_on_books(oracle, gray):
    """Books 463x370, r = 2, D = 80, auto penalties (P1 = 200, P2 = 800), bad = |d - gt| > 1 over gt > 0 with gt =
    disp1.png / 3: the reference's SGM bad-pixel rate must be below the thresholdless box rate.
    Measured: box 0.5615, SGM 0.3971."""
    gt = np.load(os.path.join(GOLDEN, "middlebury_gt.npz"))["Books/disp1"].astype(np.float64) / 3.0
    L, R = gray["Books/view1"], gray["Books/view5"]
    r, D = 2, 80
    C = oracle.box_cost(L, R, r, D).astype(np.int64)
    E = np.broadcast_to(sgm_ref.exists(D, C.shape[2])[:, None, :], C.shape)
    box = np.argmin(np.where(E, C, sgm_ref.SENTINEL), axis=0)
    _, disp = sgm_ref.aggregate(C, *sgm_ref.auto_penalties(r))
    b, s = sgm_ref.bad_rate(box, gt), sgm_ref.bad_rate(disp, gt)
    print(f"Books r=2 D=80 bad-pixel rate: box {b:.4f}, SGM {s:.4f}")
    assert s < b
