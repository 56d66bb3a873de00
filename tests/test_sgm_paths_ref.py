"""CPU tests of SM_PARAM_SGM_PATHS: the numpy diagonal scan against the literal definition, the invariants of the
eight-path sum, the host-only parts of the C ABI and what the diagonals buy on a Middlebury pair."""
import os

import numpy as np
import pytest

import sgm_paths_ref
import sgm_ref

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

LITERAL_SHAPES = [(13, 7, 6), (7, 13, 6), (5, 9, 8), (1, 5, 3), (9, 1, 4)]   # W, H, D


def _random_cost(oracle, seed, W, H, D, r):
    rng = np.random.default_rng(seed)
    L = rng.integers(0, 256, (H, W)).astype(np.uint8)
    R = rng.integers(0, 256, (H, W)).astype(np.uint8)
    return oracle.box_cost(L, R, r, D).astype(np.int64)


@pytest.mark.parametrize("W,H,D", LITERAL_SHAPES)
def test_diagonal_scan_equals_literal_triple_loop(oracle, W, H, D):
    """Wide, tall, W < D, a single column (every step restarts) and a single row (every path is C).  The second
    volume holds costs of the penalties' size, so that every term of the min is taken somewhere."""
    P1, P2 = 3, 11
    small = np.random.default_rng(W * 100 + H).integers(0, 24, (D, H, W)).astype(np.int64)
    for C in (_random_cost(oracle, 7 + W, W, H, D, 0), small):
        for rho in sgm_paths_ref.DIAGONALS:
            assert np.array_equal(sgm_paths_ref.diagonal_path(C, rho, P1, P2), sgm_ref.path_literal(C, rho, P1, P2)), rho
        S, disp = sgm_paths_ref.aggregate(C, P1, P2, 8)
        S2, disp2 = sgm_paths_ref.aggregate(C, P1, P2, 8, path_fn=sgm_ref.path_literal)
        assert np.array_equal(S, S2) and np.array_equal(disp, disp2)


def test_zero_penalties_give_eight_times_the_cost(oracle):
    W, H, D, r = 41, 19, 12, 1
    C = _random_cost(oracle, 11, W, H, D, r)
    S, disp = sgm_paths_ref.aggregate(C, 0, 0, 8)
    E = np.broadcast_to(sgm_ref.exists(D, W)[:, None, :], C.shape)
    assert np.array_equal(S[E], 8 * C[E])
    assert np.all(S[~E] == sgm_ref.SENTINEL)
    assert np.array_equal(disp, np.argmin(np.where(E, C, sgm_ref.SENTINEL), axis=0))


def test_diagonal_path_cost_is_bounded_by_cost_plus_p2(oracle):
    W, H, D, r = 37, 23, 16, 2
    C = _random_cost(oracle, 3, W, H, D, r)
    P1, P2 = sgm_ref.auto_penalties(r)
    E = np.broadcast_to(sgm_ref.exists(D, W)[:, None, :], C.shape)
    for rho in sgm_paths_ref.DIAGONALS:
        Lr = sgm_paths_ref.diagonal_path(C, rho, P1, P2)
        assert np.all(Lr[E] <= C[E] + P2) and np.all(Lr[E] >= C[E])
        assert np.all(Lr[~E] == sgm_ref._INF)
    S, _ = sgm_paths_ref.aggregate(C, P1, P2, 8)
    assert S[E].max() <= 8 * 65535 < 1 << 19


def test_four_paths_are_sgm_ref(oracle):
    W, H, D, r = 37, 23, 16, 1
    C = _random_cost(oracle, 5, W, H, D, r)
    P1, P2 = sgm_ref.auto_penalties(r)
    S, disp = sgm_paths_ref.aggregate(C, P1, P2, 4)
    S0, disp0 = sgm_ref.aggregate(C, P1, P2)
    assert np.array_equal(S, S0) and np.array_equal(disp, disp0)
    assert np.array_equal(sgm_paths_ref.aggregate(C, P1, P2)[0], S0)   # the default count
    assert sgm_paths_ref.directions(4) == sgm_ref.DIRECTIONS
    S8, _ = sgm_paths_ref.aggregate(C, P1, P2, 8)
    assert not np.array_equal(S8, S0)
    with pytest.raises(ValueError):
        sgm_paths_ref.directions(5)
    rng = np.random.default_rng(1)
    L = rng.integers(0, 256, (H, W)).astype(np.uint8)
    R = rng.integers(0, 256, (H, W)).astype(np.uint8)
    for a, b in zip(sgm_paths_ref.sgm_lr(oracle, L, R, r, D, P1, P2, median=True),
                    sgm_ref.sgm_lr(oracle, L, R, r, D, P1, P2, median=True)):
        assert np.array_equal(a, b)


def test_constant_and_null_handle():
    from gpu_stereo_matching_amd import _capi
    lib = _capi.load()
    assert _capi.SM_PARAM_SGM_PATHS == 13
    hdr = open(os.path.join(os.path.dirname(GOLDEN), "..", "include", "sm_hip.h")).read()
    assert "SM_PARAM_SGM_PATHS = 13" in hdr
    assert lib.sm_set_param_f(None, _capi.SM_PARAM_SGM_PATHS, 8.0) == _capi.SM_ERR_INVALID_ARG
    assert b"null handle" in lib.sm_last_error_string()


def test_python_layers_have_the_setter():
    import gpu_stereo_matching_amd as sm
    assert callable(sm.BlockMatcher.set_sgm_paths) and callable(sm.BlockMatcherGroup.set_sgm_paths)


def test_quality_on_books(oracle, gray):
    """Books 463x370, D = 80, auto penalties, bad = |d - gt| > 1 over gt > 0 with gt = disp1.png / 3, on the raw left
    map: at r = 0, where SGM works on per-pixel costs, the eight-path bad-pixel rate must be below the four-path one.
    Measured: r = 0: 4 paths 0.4480, 8 paths 0.4267; r = 2: 0.3971, 0.3961 (printed, not asserted: the box window has
    smoothed the volume already)."""
    gt = np.load(os.path.join(GOLDEN, "middlebury_gt.npz"))["Books/disp1"].astype(np.float64) / 3.0
    L, R = gray["Books/view1"], gray["Books/view5"]
    D = 80
    rate = {}
    for r in (0, 2):
        C = oracle.box_cost(L, R, r, D).astype(np.int64)
        for paths in (4, 8):
            _, disp = sgm_paths_ref.aggregate(C, *sgm_ref.auto_penalties(r), paths)
            rate[r, paths] = sgm_ref.bad_rate(disp, gt)
        print(f"Books r={r} D=80 bad-pixel rate: 4 paths {rate[r, 4]:.4f}, 8 paths {rate[r, 8]:.4f}")
    assert rate[0, 8] < rate[0, 4]
