"""CPU tests of the sub-pixel disparity contract: the numpy reference (tests/subpix_ref.py) against the literal
per-pixel definition, its invariants, the host-only parts of the C ABI and the accuracy the 1/16-px maps buy on
two Middlebury pairs."""
import ctypes
import os

import numpy as np
import pytest

import sgm_ref
import subpix_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")

NEW_SYMBOLS = ("sm_match_subpix_device", "sm_block_match_subpix_u16", "sm_volume_wta_subpix_device",
               "sm_reproject_device", "sm_reproject_u16")


def _column(costs, W=1):
    """A [D, 1, W] volume whose pixel x = 0 has the given costs (W large enough for every d to exist there)."""
    V = np.full((len(costs), 1, W), 1000, np.int64)
    V[:, 0, 0] = costs
    return V


@pytest.mark.parametrize("u,invalid_from,right_pairs", [(0, 0, 1), (10, 0, 1), (0, 40, 2), (25, 40, 2)])
def test_vectorised_reference_equals_the_literal_loop(u, invalid_from, right_pairs):
    rng = np.random.default_rng(11 + u)
    D, H, W = 9, 4, 13
    V = rng.integers(0, 60, (D, H, W))   # a small range: ties, plateaus and near-minima are common
    for lr in (False, True):
        got = subpix_ref.subpix(V, u, invalid_from, lr, right_pairs)
        want = subpix_ref.subpix(V, u, invalid_from, lr, right_pairs, view_fn=subpix_ref.view_literal)
        for g, w in zip(got, want):
            assert np.array_equal(g, w)
    assert got[2].any() and not got[2].all()


def test_invariants():
    rng = np.random.default_rng(5)
    D, H, W = 12, 5, 21
    V = rng.integers(0, 200, (D, H, W))
    E = subpix_ref.left_exists(D, H, W)
    q, d0, valid = subpix_ref.view(V, E)
    assert valid.all()
    assert np.array_equal(d0, np.argmin(np.where(E, V, subpix_ref.SENTINEL), axis=0))   # the 8-bit d
    assert (np.abs(q.astype(np.int64) - 16 * d0.astype(np.int64)) <= 8).all()
    assert (q[d0 == 0] == 0).all()
    dmax = np.minimum(D - 1, W - np.arange(W))
    assert (q[d0 == dmax[None, :]] == 16 * d0[d0 == dmax[None, :]]).all()            # no neighbour above: delta 0
    assert q.max() <= 16 * 255 + 8
    # D = 1 and D = 2 have no interior d
    for D2 in (1, 2):
        q2, d2, _ = subpix_ref.view(V[:D2], E[:D2])
        assert np.array_equal(q2, 16 * d2.astype(np.uint16))
    # all-equal costs: the first minimum is d = 0
    q3, _, _ = subpix_ref.view(np.full((D, H, W), 7), E)
    assert not q3.any()


def test_crafted_plateau_and_both_ends_of_delta():
    W = 16
    E = subpix_ref.left_exists(5, 1, W)
    # a two-wide plateau, c == b: delta = floor((16 (a - b) + (a - b)) / (2 (a - b))) = 8
    q, d0, _ = subpix_ref.view(_column([9, 9, 3, 3, 9], W), E)
    assert (d0[0, 0], q[0, 0]) == (2, 16 * 2 + 8)
    # a = b + 1, c huge: 8 (a - c) / den = -7.98, which rounds to -8
    q, d0, _ = subpix_ref.view(_column([50, 11, 10, 1000, 50], W), E)
    assert (d0[0, 0], q[0, 0]) == (2, 16 * 2 - 8)
    # symmetric neighbours: delta 0; exactly half way rounds up
    q, _, _ = subpix_ref.view(_column([50, 20, 10, 20, 50], W), E)
    assert q[0, 0] == 32
    q, _, _ = subpix_ref.view(_column([50, 13, 10, 12, 50], W), E)   # 8 * 1 / 5 = 1.6 -> 2
    assert q[0, 0] == 34
    q, _, _ = subpix_ref.view(_column([50, 14, 10, 13, 50], W), E)   # 8 * 1 / 7 = 1.14 -> 1
    assert q[0, 0] == 33
    q, _, _ = subpix_ref.view(_column([50, 12, 10, 13, 50], W), E)   # -8 / 5 = -1.6 -> -2 (floor, not truncation)
    assert q[0, 0] == 30
    # -0.5 exactly rounds half up to 0: 8 (a - c) / den = -1/2 <=> den = 16 (c - a), e.g. a - b = 15, c - b = 17
    q, _, _ = subpix_ref.view(_column([90, 10 + 15, 10, 10 + 17, 90], W), E)
    assert q[0, 0] == 32
    # +0.5 exactly rounds up to 1
    q, _, _ = subpix_ref.view(_column([90, 10 + 17, 10, 10 + 15, 90], W), E)
    assert q[0, 0] == 33


def test_the_kernels_unsigned_division_is_the_floor_division_below_2_24():
    """subpix_wta_kernel divides the non-negative numerator 16 (a - c) + 33 den by 2 den in uint32 and takes 16 off
    (bm_subpix.hip): equal to the floor division for every a > b <= c below 2^24, without overflow."""
    rng = np.random.default_rng(1)
    top = (1 << 24) - 1
    b = np.concatenate([rng.integers(0, top, 4000), [0, 0, 0, top - 1, 0]])
    a = np.concatenate([rng.integers(0, top, 4000), [top, 1, top, top, 1]])
    c = np.concatenate([rng.integers(0, top, 4000), [top, top, 0, top - 1, 0]])
    b = np.minimum(b, np.minimum(a - 1, c))
    keep = b >= 0
    a, b, c = a[keep], b[keep], c[keep]
    den = a + c - 2 * b
    assert (den >= 1).all()
    want = (16 * (a - c) + den) // (2 * den)
    num = 16 * a - 16 * c + 33 * den
    assert (num >= 0).all() and (num < 1 << 31).all()
    a32, b32, c32 = (v.astype(np.uint32) for v in (a, b, c))
    den32 = a32 + c32 - np.uint32(2) * b32
    got = ((np.uint32(16) * a32 - np.uint32(16) * c32 + np.uint32(33) * den32) // (np.uint32(2) * den32)).astype(np.int64) - 16
    assert np.array_equal(got, want) and want.min() == -8 and want.max() == 8


def test_uniqueness_boundary():
    W, u = 16, 10
    E = subpix_ref.left_exists(6, 1, W)
    b = 90   # b * 100 = 9000 = 100 * (100 - u): a rival at exactly 100 ties the strict comparison
    for rival, ok in ((100, True), (99, False)):
        q, d0, valid = subpix_ref.view(_column([500, 400, b, 400, rival, 500], W), E, u)
        assert bool(valid[0, 0]) is ok and bool(q[0, 0] != 0) is ok and d0[0, 0] == (2 if ok else 0)
    # an adjacent d never counts, however close
    _, _, valid = subpix_ref.view(_column([500, b + 1, b, b, 500, 500], W), E, u)
    assert valid[0, 0]
    # u = 0 is off
    _, _, valid = subpix_ref.view(_column([b, 400, 400, 400, b, 500], W), E, 0)
    assert valid[0, 0]
    # the threshold: invalid from b == invalid_from on
    for inv, ok in ((b + 1, True), (b, False)):
        _, _, valid = subpix_ref.view(_column([500, 400, b, 400, 500, 500], W), E, 0, inv)
        assert bool(valid[0, 0]) is ok


def test_lr_check_and_invalid_views():
    """The check runs on d0 with invalid pixels counted as d0 = 0, and matches oracle-free launch_lr_check rules."""
    dl = np.array([[0, 1, 2, 5, 2, 3]], np.uint8)
    dr = np.array([[9, 0, 2, 1, 2, 0]], np.uint8)
    # x=0: d == 0; x=1: dR(0) = 9; x=2: dR(0) = 9; x=3: x - d < 0; x=4: dR(2) = 2 ok; x=5: dR(2) = 2, |3 - 2| = 1 ok
    assert subpix_ref.lr_occluded(dl, dr).tolist() == [[True, True, True, True, False, False]]
    rng = np.random.default_rng(3)
    V = rng.integers(0, 50, (6, 3, 17))
    q, qr, mask = subpix_ref.subpix(V, 30, 0, True)
    assert not q[mask == 0].any() and mask.any() and not mask.all()
    # with nothing invalidated the mask is the integer check of the two argmin maps
    q0, _, mask0 = subpix_ref.subpix(V, 0, 0, True)
    E = subpix_ref.left_exists(*V.shape)
    dl = np.argmin(np.where(E, V, subpix_ref.SENTINEL), axis=0).astype(np.uint8)
    VR, ER = subpix_ref.right_view(V)
    dr = np.argmin(np.where(ER, VR, subpix_ref.SENTINEL), axis=0).astype(np.uint8)
    assert np.array_equal(mask0, (~subpix_ref.lr_occluded(dl, dr)).astype(np.uint8))
    assert (np.abs(q0.astype(np.int64) - 16 * dl)[mask0 == 1] <= 8).all()


@pytest.mark.parametrize("name", ["Books", "Art"])
def test_quality(oracle, gray, name):
    """463x370, r = 2, D = 80, AD cost, auto penalties, four-path SGM: the mean absolute error against gt = disp1 / 3
    over the pixels with gt > 0 whose integer disparity is within 1 of gt must drop with the 1/16-px values.
    Measured: Books 0.3426 -> 0.2956, Art 0.3840 -> 0.3381."""
    gt = np.load(os.path.join(GOLDEN, "middlebury_gt.npz"))[f"{name}/disp1"].astype(np.float64) / 3.0
    L, R = gray[f"{name}/view1"], gray[f"{name}/view5"]
    r, D = 2, 80
    S, d_int = sgm_ref.aggregate(oracle.box_cost(L, R, r, D), *sgm_ref.auto_penalties(r))
    q, d0, _ = subpix_ref.view(S, subpix_ref.left_exists(*S.shape))
    assert np.array_equal(d0, d_int)
    mae_int = subpix_ref.mae(d_int, d_int, gt)
    mae_sub = subpix_ref.mae(q.astype(np.float64) / 16.0, d_int, gt)
    print(f"{name} r=2 D=80 AD SGM mean |d - gt|: integer {mae_int:.4f}, 1/16 px {mae_sub:.4f}")
    assert mae_sub < mae_int


def test_symbols_and_constants():
    import gpu_stereo_matching_amd as sm
    from gpu_stereo_matching_amd import _capi
    lib = _capi.load()
    hdr = open(os.path.join(ROOT, "include", "sm_hip.h")).read()
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name) and name in _capi.EXPORTED and name + "(" in hdr
    assert _capi.SM_PARAM_UNIQUENESS == 7 and "SM_PARAM_UNIQUENESS = 7" in hdr
    for name in ("match_subpix", "match_subpix_device", "volume_wta_subpix_device", "set_uniqueness", "reproject",
                 "reproject_device"):
        assert callable(getattr(sm.BlockMatcher, name))
    f = sm.to_float(np.array([[0, 8, 4088]], np.uint16))
    assert f.dtype == np.float32 and f.tolist() == [[0.0, 0.5, 255.5]]


def test_refusals_without_a_device():
    from gpu_stereo_matching_amd import _capi
    lib = _capi.load()
    INVALID = _capi.SM_ERR_INVALID_ARG
    SGM, CEN, LR = _capi.SM_AGG_SGM, _capi.SM_COST_CENSUS, _capi.SM_LR_CHECK

    def dev(flags, width=64, radius=2):
        return lib.sm_match_subpix_device(None, None, None, width, 8, width, 1, 8 * width, radius, 16, flags, None,
                                          width, 8 * width, None, None, None)

    def host(flags, width=64, radius=2):
        return lib.sm_block_match_subpix_u16(None, None, None, width, 8, width, radius, 16, flags, None, None, None,
                                             width)

    for call in (dev, host):
        for agg in (0, SGM, SGM | CEN, CEN | LR):
            assert call(agg | _capi.SM_MEDIAN) == INVALID
            assert b"SM_MEDIAN" in lib.sm_last_error_string() and b"8-bit" in lib.sm_last_error_string()
            for other in (_capi.SM_AGG_GUIDED, _capi.SM_STAGED, _capi.SM_DEVICE_CU_GRID):
                assert call(agg | other) == INVALID and b"no cost volume" in lib.sm_last_error_string()
            assert call(agg, radius=8) == INVALID and b"radius 8" in lib.sm_last_error_string()
            assert call(agg, width=4097) == INVALID and b"width 4097" in lib.sm_last_error_string()
            assert call(agg) == INVALID and b"null handle" in lib.sm_last_error_string()
    q = (ctypes.c_double * 16)()
    assert lib.sm_volume_wta_subpix_device(None, None, 2, 8, 8, 4, 0, 0, None, 8, None, None, None) == INVALID
    assert b"null handle" in lib.sm_last_error_string()
    assert lib.sm_reproject_device(None, None, 8, 8, 8, q, None, 24, None) == INVALID
    assert b"null handle" in lib.sm_last_error_string()
    assert lib.sm_reproject_u16(None, None, 8, 8, 8, q, None, 24) == INVALID
    assert b"null handle" in lib.sm_last_error_string()
    assert lib.sm_set_param_f(None, _capi.SM_PARAM_UNIQUENESS, 10.0) == INVALID
    assert b"null handle" in lib.sm_last_error_string()
    assert lib.sm_group_set_param_f(None, _capi.SM_PARAM_UNIQUENESS, 10.0) == INVALID
