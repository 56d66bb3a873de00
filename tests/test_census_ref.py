"""CPU tests of the census matching cost (SM_COST_CENSUS): the numpy reference against the literal definition, its
invariants, the host-only parts of the C ABI and the quality the cost buys on two Middlebury pairs."""
import ctypes
import os

import numpy as np
import pytest

import census_ref
import sgm_ref

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _noisy_pair(oracle, seed, W, H, D):
    """oracle.synth_pair with +-4 noise on the right image, so that costs are not degenerate."""
    L, R = oracle.synth_pair(seed, W, H, D)
    noise = np.random.default_rng(seed).integers(-4, 5, R.shape)
    return L, np.clip(R.astype(np.int64) + noise, 0, 255).astype(np.uint8)


@pytest.mark.parametrize("W,H", [(11, 8), (5, 3)])   # 5 x 3 lies inside the 9 x 7 window
def test_census_and_hamming_equal_the_literal_loops(W, H):
    D = 5
    rng = np.random.default_rng(W * 100 + H)
    L = rng.integers(0, 256, (H, W)).astype(np.uint8)
    R = rng.integers(0, 256, (H, W)).astype(np.uint8)
    L[0, :3] = L[0, 0]   # ties: the compare is strict
    assert len(census_ref.OFFSETS) == 62 and census_ref.OFFSETS[0] == (-3, -4) and census_ref.OFFSETS[31] == (0, 1)
    assert np.array_equal(census_ref.census(L), census_ref.census_literal(L))
    assert np.array_equal(census_ref.census(R), census_ref.census_literal(R))
    assert np.array_equal(census_ref.hamming_volume(L, R, D), census_ref.hamming_volume_literal(L, R, D))


@pytest.mark.parametrize("radius", [0, 1, 3])
def test_box_sum_of_the_ad_volume_is_the_box_cost(oracle, radius):
    W, H, D = 23, 14, 9
    L, R = _noisy_pair(oracle, 7, W, H, D)
    assert np.array_equal(census_ref.box_sum(oracle.precal(L, R, D), radius), oracle.box_cost(L, R, radius, D))


def test_invariants(oracle):
    W, H, D = 37, 23, 12
    L, R = _noisy_pair(oracle, 3, W, H, D)
    assert not census_ref.census(np.full((H, W), 97, np.uint8)).any()
    for img in (L, R):
        assert not (census_ref.census(img) >> np.uint64(62)).any()
    assert not census_ref.hamming_volume(L, L, D)[0].any()
    ham = census_ref.hamming_volume(L, R, D)
    assert ham.max() <= census_ref.MAX_HAM == 62
    for d in range(D):
        assert not ham[d][:, :d].any()
    assert census_ref.cost(L, R, 2, D).max() <= 62 * 25


def test_symbols_and_constants():
    import gpu_stereo_matching_amd as sm
    from gpu_stereo_matching_amd import _capi
    lib = _capi.load()
    for name in ("sm_census_device", "sm_census_volume_device", "sm_census_volume_u8", "sm_census_workspace_bytes"):
        assert hasattr(lib, name) and name in _capi.EXPORTED
    assert _capi.SM_COST_CENSUS == 64 == sm.SM_COST_CENSUS
    assert sm._flags("sgm", True, True) == sm.SM_AGG_SGM | sm.SM_LR_CHECK | sm.SM_MEDIAN
    assert sm._flags("sgm", True, True, "census") == sm.SM_AGG_SGM | sm.SM_LR_CHECK | sm.SM_MEDIAN | 64
    assert sm._flags("box", False, False, "census") == 64 and sm._flags("box", False, False, "ad") == 0
    with pytest.raises(ValueError, match="cost must be"):
        sm._flags("box", False, False, "hamming")
    hdr = open(os.path.join(os.path.dirname(GOLDEN), "..", "include", "sm_hip.h")).read()
    assert "SM_COST_CENSUS = 64u" in hdr


@pytest.mark.parametrize("radius", range(8))
def test_auto_penalties(radius):
    import gpu_stereo_matching_amd as sm
    win2 = (2 * radius + 1) ** 2
    assert sm.sgm_penalties(radius, cost="census") == (10 * win2, 120 * win2) == census_ref.auto_penalties(radius)
    assert sm.sgm_penalties(radius, 5, 0, cost="census") == (5, 120 * win2)
    assert sm.sgm_penalties(radius, 7, 9, cost="census") == (7, 9)
    # without the bit: the AD answers, unchanged
    assert sm.sgm_penalties(radius) == sm.sgm_penalties(radius, cost="ad") == (8 * win2, 32 * win2)


def test_sgm_check_with_the_census_bit():
    from gpu_stereo_matching_amd import _capi
    lib = _capi.load()
    SGM, CEN, INVALID = _capi.SM_AGG_SGM, _capi.SM_COST_CENSUS, _capi.SM_ERR_INVALID_ARG

    def rc(width, radius, flags, p1, p2):
        return lib.sm_sgm_check(width, radius, flags, p1, p2, None, None)

    for r in range(8):
        win2 = (2 * r + 1) ** 2
        assert rc(640, r, SGM | CEN, 0, 65535 - 62 * win2) == _capi.SM_OK
        assert rc(640, r, SGM | CEN, 0, 65536 - 62 * win2) == INVALID and b"65535" in lib.sm_last_error_string()
    assert rc(640, 7, SGM | CEN, 0, 0) == _capi.SM_OK            # 62 * 225 + 120 * 225 = 40950
    # the AD bound without the bit, as before
    assert rc(640, 7, SGM, 0, 8160) == _capi.SM_OK
    assert rc(640, 7, SGM, 0, 8161) == INVALID and b"65535" in lib.sm_last_error_string()
    assert rc(640, 7, SGM | CEN, 0, 8161) == _capi.SM_OK
    assert rc(640, 2, SGM | CEN, 3001, 0) == INVALID and b"P1" in lib.sm_last_error_string()   # auto P2 = 3000
    p1, p2 = ctypes.c_int(), ctypes.c_int()
    assert lib.sm_sgm_check(640, 3, SGM | CEN, 0, 0, ctypes.byref(p1), ctypes.byref(p2)) == _capi.SM_OK
    assert (p1.value, p2.value) == (490, 5880)


def test_rejections_without_a_device():
    from gpu_stereo_matching_amd import _capi
    lib = _capi.load()
    SGM, CEN, INVALID = _capi.SM_AGG_SGM, _capi.SM_COST_CENSUS, _capi.SM_ERR_INVALID_ARG
    n = ctypes.c_size_t()

    def ws(width, radius, flags):   # census_check / sgm_check, as the matching entry points apply them
        return lib.sm_census_workspace_bytes(width, 64, 16, radius, flags, ctypes.byref(n))

    for agg in (0, SGM):
        assert ws(640, 2, agg | CEN) == _capi.SM_OK and n.value > 0
        for other in (_capi.SM_AGG_GUIDED, _capi.SM_STAGED, _capi.SM_DEVICE_CU_GRID):
            assert ws(640, 2, agg | CEN | other) == INVALID and n.value == 0
            assert b"SM_COST_CENSUS does not combine" in lib.sm_last_error_string()
            assert lib.sm_sgm_check(640, 2, agg | CEN | other, 0, 0, None, None) == INVALID
            assert b"SM_COST_CENSUS does not combine" in lib.sm_last_error_string()
        assert ws(640, 8, agg | CEN) == INVALID and b"radius" in lib.sm_last_error_string()
        assert ws(640, -1, agg | CEN) == INVALID and b"radius" in lib.sm_last_error_string()
        assert ws(640, 7, agg | CEN) == _capi.SM_OK
        assert ws(4096, 2, agg | CEN) == _capi.SM_OK
        assert ws(4097, 2, agg | CEN) == INVALID and b"width" in lib.sm_last_error_string()
        assert ws(0, 2, agg | CEN) == INVALID and b"width" in lib.sm_last_error_string()
    # the entry points themselves, on the null-handle path the other argument tests use
    assert lib.sm_block_match_u8(None, None, None, 10, 10, 10, 1, 8, CEN, None, 10) == INVALID
    assert lib.sm_match_device(None, None, None, 10, 10, 10, 1, 100, 1, 8, SGM | CEN, None, 10, 100, None) == INVALID
    assert lib.sm_census_device(None, None, 10, 10, 10, None, None) == INVALID
    assert lib.sm_census_volume_device(None, None, None, 10, 10, 10, 4, None, None) == INVALID
    assert lib.sm_census_volume_u8(None, None, None, 10, 10, 10, 4, None) == INVALID
    # the calls that cannot honour the flag
    assert lib.sm_group_block_match_u8(None, None, None, 8, 8, 8, 1, 8, CEN, None, 8) == INVALID
    assert lib.sm_group_dslice_block_match_u8(None, None, None, 8, 8, 8, 1, 8, CEN, None, 8) == INVALID
    assert lib.sm_dslice_rehearse_u8(None, None, None, 8, 8, 8, 1, 8, CEN, 2, None, 8) == INVALID
    assert lib.sm_slice_keys_lr_device(None, None, None, 8, 8, 8, 1, 0, 8, CEN, None, None, None) == INVALID


def test_workspace_bytes():
    import gpu_stereo_matching_amd as sm
    W, H, D = 1920, 1080, 128
    P = W * H
    box = sm.census_workspace_bytes(W, H, D, 2)
    assert 3 * P * D + 20 * P <= box <= 3 * P * D + 20 * P + 5 * 256   # Hamming u8, cost u16, keys, two census images
    sgm = sm.census_workspace_bytes(W, H, D, 2, agg="sgm")
    assert sgm == sm.sgm_workspace_bytes(W, H, D, 2) + 16 * P          # 8 P is a multiple of 256 here
    assert 6 * P * D + 20 * P <= sgm <= 6 * P * D + 20 * P + 5 * 256
    with pytest.raises(sm.SMError):
        sm.census_workspace_bytes(W, H, 257, 2)
    with pytest.raises(sm.SMError):
        sm.census_workspace_bytes(W, H, D, 8)
    with pytest.raises(ValueError):
        sm.census_workspace_bytes(W, H, D, 2, agg="guided")
    from gpu_stereo_matching_amd import _capi
    assert _capi.load().sm_census_workspace_bytes(64, 64, 16, 2, 0, None) == _capi.SM_ERR_INVALID_ARG


@pytest.mark.parametrize("name", ["Books", "Art"])
def test_quality(oracle, gray, name):
    """463x370, r = 2, D = 80, auto penalties, bad = |d - gt| > 1 over gt > 0 with gt = disp1.png / 3: on the
    reference implementation the census cost must beat the AD cost under both aggregations.
    Measured: Books AD box 0.5615, AD SGM 0.3971, census box 0.3942, census SGM 0.3285;
              Art   AD box 0.6277, AD SGM 0.5309, census box 0.4717, census SGM 0.4398."""
    gt = np.load(os.path.join(GOLDEN, "middlebury_gt.npz"))[f"{name}/disp1"].astype(np.float64) / 3.0
    L, R = gray[f"{name}/view1"], gray[f"{name}/view5"]
    r, D = 2, 80
    Cad = oracle.box_cost(L, R, r, D).astype(np.int64)
    Ccen = census_ref.cost(L, R, r, D)
    ad_box = sgm_ref.bad_rate(census_ref.box_wta(Cad)[1], gt)
    cen_box = sgm_ref.bad_rate(census_ref.box_wta(Ccen)[1], gt)
    ad_sgm = sgm_ref.bad_rate(sgm_ref.aggregate(Cad, *sgm_ref.auto_penalties(r))[1], gt)
    cen_sgm = sgm_ref.bad_rate(sgm_ref.aggregate(Ccen, *census_ref.auto_penalties(r))[1], gt)
    print(f"{name} r=2 D=80 bad-pixel rate: AD box {ad_box:.4f}, AD SGM {ad_sgm:.4f}, "
          f"census box {cen_box:.4f}, census SGM {cen_sgm:.4f}")
    assert cen_sgm < ad_sgm
    assert cen_box < ad_box
