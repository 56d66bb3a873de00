"""CPU tests of SM_PAIRS_IN_VIEW and SM_PARAM_MIN_DISP: the numpy restatement (tests/pairs_ref.py) against the older
references under the reference's rule and against a literal per-pixel loop under the in-view rule, what the rule buys
on the Middlebury pairs, and the host-only parts of the C ABI."""
import ctypes
import os

import numpy as np
import pytest

import census_ref
import pairs_ref
import sgm_paths_ref
import sgm_ref
import subpix_ref

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

REFERENCE_SHAPES = [(13, 7, 6, 1), (7, 13, 9, 0), (24, 5, 8, 2), (1, 5, 3, 0), (9, 1, 4, 1)]   # W, H, D, r
# W, H, D, d0: plain; a minimum disparity with columns that have no candidate; a single column (only d = 0 exists); a
# single row; d0 = W, where no pixel has a candidate
IN_VIEW_SHAPES = [(7, 5, 4, 0), (9, 4, 6, 3), (1, 6, 2, 0), (6, 1, 5, 2), (5, 5, 3, 5)]


def _pair(seed, W, H):
    rng = np.random.default_rng(seed)
    return rng.integers(0, 256, (H, W)).astype(np.uint8), rng.integers(0, 256, (H, W)).astype(np.uint8)


# ---- 1. the reference's rule: pairs_ref is the older references ----
@pytest.mark.parametrize("W,H,D,r", REFERENCE_SHAPES)
def test_reference_rule_equals_the_older_references(oracle, W, H, D, r):
    L, R = _pair(W * 31 + H, W, H)
    assert np.array_equal(pairs_ref.exists("reference", D, W), sgm_ref.exists(D, W))
    assert np.array_equal(pairs_ref.ad_volume(L, R, D), oracle.precal(L, R, D).reshape(D, H, W))
    assert np.array_equal(pairs_ref.hamming_volume(L, R, D), census_ref.hamming_volume(L, R, D))
    C = {"ad": oracle.box_cost(L, R, r, D).astype(np.int64), "census": census_ref.cost(L, R, r, D).astype(np.int64)}
    ref = pairs_ref.Reference(L, R, r, D)
    for kind in ("ad", "census"):
        assert np.array_equal(ref.cost(kind), C[kind]), kind
        P1, P2 = ref.penalties(kind)
        E = pairs_ref.exists("reference", D, W)
        for rho in sgm_paths_ref.directions(8):
            want = sgm_paths_ref.path(C[kind], rho, P1, P2)
            assert np.array_equal(pairs_ref.path(C[kind], rho, P1, P2, E), want), rho
        for paths in (4, 8):
            S, dl = sgm_paths_ref.aggregate(C[kind], P1, P2, paths)
            assert np.array_equal(ref.volume("sgm", kind, paths)[0], S)
            want = sgm_paths_ref.maps(oracle, S, dl)
            for a, b in zip(ref.maps("sgm", kind, paths), want):
                assert np.array_equal(a, b), (kind, paths)
            for u, lr in ((0, False), (10, True), (0, True)):
                for a, b in zip(ref.subpix("sgm", kind, u, lr, paths), subpix_ref.subpix(S, u, 0, lr, 1)):
                    assert np.array_equal(a, b), (kind, paths, u, lr)
    # the census box WTA and the AD box volume of the sub-pixel calls
    for a, b in zip(ref.maps("box", "census"), census_ref.census_lr(oracle, L, R, r, D, "box")):
        assert np.array_equal(a, b)
    for agg, kind in (("box", "census"), ("box", "ad")):
        V, inv, rp = subpix_ref.volume(oracle, L, R, r, D, agg, kind)
        for u, lr in ((0, False), (10, True)):
            for a, b in zip(ref.subpix(agg, kind, u, lr), subpix_ref.subpix(V, u, inv, lr, rp)):
                assert np.array_equal(a, b), (agg, kind, u, lr)


# ---- 2. the in-view rule: pairs_ref is the literal loop of the contract ----
def _literal_maps(V, rule, d0):
    """The 8-bit rule per pixel, both views and the check: (left, right, checked, mask)."""
    D, H, W = V.shape
    dl, dr = np.zeros((H, W), np.uint8), np.zeros((H, W), np.uint8)
    for y in range(H):
        for x in range(W):
            ks = [k for k in range(D) if x - (d0 + k) >= 0]
            if ks:
                v = [int(V[k, y, x]) for k in ks]
                dl[y, x] = d0 + v.index(min(v))
            ks = [k for k in range(D) if x + d0 + k <= W - 1]
            if ks:
                v = [int(V[k, y, x + d0 + k]) for k in ks]
                dr[y, x] = d0 + v.index(min(v))
    checked, mask = np.zeros((H, W), np.uint8), np.zeros((H, W), np.uint8)
    for y in range(H):
        for x in range(W):
            d = int(dl[y, x])
            if d != 0 and x - d >= 0 and abs(d - int(dr[y, x - d])) <= 1:
                checked[y, x], mask[y, x] = d, 1
    return dl, dr, checked, mask


@pytest.mark.parametrize("paths", [4, 8])
@pytest.mark.parametrize("W,H,D,d0", IN_VIEW_SHAPES)
def test_in_view_rule_equals_literal_triple_loop(W, H, D, d0, paths):
    P1, P2 = 3, 11
    L, R = _pair(W * 7 + H + d0, W, H)
    # (costs of the penalties' size, so that every term of the min is taken somewhere)
    small = np.random.default_rng(W * 100 + H).integers(0, 24, (D, H, W)).astype(np.int64)
    E = pairs_ref.exists("in-view", D, W, d0)
    assert np.array_equal(E, np.array([[x - (d0 + k) >= 0 for x in range(W)] for k in range(D)]))
    ER = pairs_ref.right_exists("in-view", D, W, d0)
    assert np.array_equal(ER, np.array([[u + d0 + k <= W - 1 for u in range(W)] for k in range(D)]))
    if d0 >= W:
        assert not E.any() and not ER.any()
    for C in (pairs_ref.cost(L, R, 1, D, "ad", d0), pairs_ref.cost(L, R, 0, D, "census", d0), small):
        for rho in sgm_paths_ref.directions(paths):
            assert np.array_equal(pairs_ref.path(C, rho, P1, P2, E),
                                  pairs_ref.path_literal(C, rho, P1, P2, "in-view", d0)), rho
        S = pairs_ref.aggregate(C, P1, P2, paths, "in-view", d0)
        S2 = pairs_ref.aggregate(C, P1, P2, paths, "in-view", d0,
                                 path_fn=lambda C_, rho: pairs_ref.path_literal(C_, rho, P1, P2, "in-view", d0))
        assert np.array_equal(S, S2)
        assert np.all(S[~np.broadcast_to(E[:, None, :], S.shape)] == sgm_ref.SENTINEL)
        for V in (S, pairs_ref.box_volume(C, "in-view", d0)):   # SGM's sums and the census box WTA
            for a, b in zip(pairs_ref.maps8(V, "in-view", d0), _literal_maps(V, "in-view", d0)):
                assert np.array_equal(a, b)
            for u, inv, lr in ((0, 0, False), (10, 0, True), (0, 40, True)):
                got = pairs_ref.subpix(V, "in-view", d0, u, inv, lr)
                want = pairs_ref.subpix(V, "in-view", d0, u, inv, lr, view_fn=pairs_ref.view16_literal)
                for a, b in zip(got, want):
                    assert np.array_equal(a, b), (u, inv, lr)
        # a pixel with no candidate: 0 in both maps and the mask, in either view
        none_l, none_r = ~E.any(axis=0), ~ER.any(axis=0)
        dl, dr, checked, mask = pairs_ref.maps8(S, "in-view", d0)
        q, qr, qm = pairs_ref.subpix(S, "in-view", d0)
        assert not dl[:, none_l].any() and not q[:, none_l].any() and not qm[:, none_l].any()
        assert not dr[:, none_r].any() and not qr[:, none_r].any()
        assert not checked[:, none_l].any() and not mask[:, none_l].any()
        if d0 and not none_l.all():
            assert dl[:, ~none_l].min() >= d0 and q[:, ~none_l].min() >= 16 * d0 - 8


def test_cost_planes_are_the_reference_planes_shifted():
    """Plane k under a minimum disparity d0 is plane d0 + k of the d0 = 0 volume: the costs keep their zero rule."""
    W, H, D, d0 = 19, 6, 5, 4
    L, R = _pair(5, W, H)
    assert np.array_equal(pairs_ref.ad_volume(L, R, D, d0), pairs_ref.ad_volume(L, R, D + d0)[d0:])
    assert np.array_equal(pairs_ref.hamming_volume(L, R, D, d0), pairs_ref.hamming_volume(L, R, D + d0)[d0:])
    assert np.array_equal(pairs_ref.cost(L, R, 2, D, "ad", d0), pairs_ref.cost(L, R, 2, D + d0, "ad")[d0:])
    with pytest.raises(ValueError):
        pairs_ref.exists("reference", D, W, 1)
    with pytest.raises(ValueError):
        pairs_ref.exists("other", D, W)


# ---- 3. what the rule buys ----
def test_quality_on_books(gray):
    """Books 463x370, r = 2, D = 80, 4 paths, auto penalties, bad = |d - gt| > 1 over gt > 0 with gt = disp1.png / 3 on
    the raw left map: the in-view bad-pixel rate must be below the reference rule's by at least 0.05, half the gain
    measured with sgm_paths_ref's existence rule replaced (0.3971 against 0.2882).  The other figures are printed:
    Art, r = 0, eight paths, the borders, and d0 = 20 with D = 60."""
    gts = np.load(os.path.join(GOLDEN, "middlebury_gt.npz"))
    rate = {}
    for name in ("Books", "Art"):
        gt = gts[f"{name}/disp1"].astype(np.float64) / 3.0
        L, R = gray[f"{name}/view1"], gray[f"{name}/view5"]
        W = L.shape[1]
        for r in (2, 0):
            for rule in pairs_ref.RULES:
                ref = pairs_ref.Reference(L, R, r, 80, rule)
                for paths in (4, 8) if name == "Books" else (4,):
                    dl = ref.maps("sgm", "ad", paths)[0]
                    rate[name, r, rule, paths] = pairs_ref.bad_rate(dl, gt)
                    parts = [pairs_ref.bad_rate(dl, gt, c) for c in (slice(0, 80), slice(W - 80, W), slice(80, W - 80))]
                    print(f"{name} r={r} D=80 {paths} paths {rule}: bad {rate[name, r, rule, paths]:.4f} "
                          f"(left 80 cols {parts[0]:.3f}, right 80 cols {parts[1]:.3f}, middle {parts[2]:.3f})")
        if name == "Books":
            for d0, D in ((16, 64), (20, 60)):
                dl = pairs_ref.Reference(L, R, 2, D, "in-view", d0).maps("sgm", "ad")[0]
                print(f"Books r=2 d0={d0} D={D} 4 paths in-view: bad {pairs_ref.bad_rate(dl, gt):.4f}")
    assert rate["Books", 2, "in-view", 4] <= rate["Books", 2, "reference", 4] - 0.05


# ---- 4. the host-only parts of the C ABI ----
def test_constants_and_host_refusals():
    import gpu_stereo_matching_amd as sm
    from gpu_stereo_matching_amd import _capi
    lib = _capi.load()
    assert _capi.SM_PAIRS_IN_VIEW == 128 == sm.SM_PAIRS_IN_VIEW and _capi.SM_PARAM_MIN_DISP == 14
    hdr = open(os.path.join(os.path.dirname(GOLDEN), "..", "include", "sm_hip.h")).read()
    assert "SM_PAIRS_IN_VIEW = 128u" in hdr and "SM_PARAM_MIN_DISP = 14" in hdr
    assert sm._flags("sgm", True, pairs="in-view") == sm.SM_AGG_SGM | sm.SM_LR_CHECK | sm.SM_PAIRS_IN_VIEW
    assert sm._flags("sgm", True) == sm.SM_AGG_SGM | sm.SM_LR_CHECK
    with pytest.raises(ValueError, match="pairs"):
        sm._flags("sgm", False, pairs="all")
    assert callable(sm.BlockMatcher.set_min_disp) and callable(sm.BlockMatcherGroup.set_min_disp)
    # sm_sgm_check takes the bit with SGM (and the census cost), with the penalties it gives without it
    a, b = ctypes.c_int(), ctypes.c_int()
    for extra in (0, _capi.SM_COST_CENSUS):
        f = _capi.SM_AGG_SGM | extra
        f |= _capi.SM_PAIRS_IN_VIEW
        assert lib.sm_sgm_check(640, 2, f, 0, 0, ctypes.byref(a), ctypes.byref(b)) == _capi.SM_OK
        assert (a.value, b.value) == sm.sgm_penalties(2, width=640, cost="census" if extra else "ad")
    assert sm.sgm_penalties(2, pairs="in-view") == sm.sgm_penalties(2)
    for other in (_capi.SM_AGG_GUIDED, _capi.SM_STAGED, _capi.SM_DEVICE_CU_GRID):
        f = _capi.SM_AGG_SGM | _capi.SM_PAIRS_IN_VIEW | other
        assert lib.sm_sgm_check(640, 2, f, 0, 0, None, None) == _capi.SM_ERR_INVALID_ARG
    # the workspace sizes do not know the rule, and the parameter needs a handle
    assert lib.sm_set_param_f(None, _capi.SM_PARAM_MIN_DISP, 3.0) == _capi.SM_ERR_INVALID_ARG
    assert b"null handle" in lib.sm_last_error_string()
