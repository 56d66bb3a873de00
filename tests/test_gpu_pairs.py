"""GPU tests of SM_PAIRS_IN_VIEW and SM_PARAM_MIN_DISP against the numpy restatement (tests/pairs_ref.py).

Every shape runs the AD and the census cost through SGM with four and eight paths, the census box WTA and the AD box
volume of the sub-pixel calls, each through match, match_lr, match_subpix and match_subpix with the LR check and
uniqueness 10.  Integer arithmetic end to end: every comparison is np.array_equal.
"""
import functools

import numpy as np
import pytest

import fill_ref
import pairs_ref
import sgm_paths_ref
import speckle_ref
from fuzz_util import fuzz_pair
from test_volume_variants_model import BOUND_SHAPE, bound_input, bound_p2

pytestmark = pytest.mark.gpu

COSTS = ("ad", "census")
SUBPIX_COMBOS = [(0, False), (10, True)]   # uniqueness, lr_check
WIDE = 640
IV = "in-view"

# W, H, D, r, d0
CASES = [
    (75, 9, 129, 2, 0),     # sgm_h<3, false>, a partial last lane; kmax = x would reach D - 1 at x = 128 > W: never full
    (33, 7, 65, 1, 0),      # a lone d in the last lane / chunk; one column past a tile
    (40, 6, 193, 0, 0),     # W < D: no column reaches D - 1
    (67, 35, 16, 2, 0),     # three tiles with a partial last one on the diagonals
    (67, 35, 16, 2, 3),
    (32, 3, 8, 0, 3),       # one tile, H < prefetch depth, the first three columns without a candidate
    (9, 40, 5, 7, 4),       # H >> W, every lane wraps
    (9, 40, 5, 7, 9),       # d0 = W: the all-zero map and mask
    (1, 9, 2, 0, 0),        # a single column: only d = 0 exists
    (64, 1, 8, 0, 2),       # a single row
    (96, 5, 256, 3, 0),     # 32 chunks of 8
    (300, 4, 6, 1, 250),    # the 8-bit bound, d0 + D - 1 = 255
    (4096, 2, 20, 0, 0),    # the width limit
]
SUBPIX_ONLY_CASES = [(4096, 2, 96, 0, 4000)]   # q up to 16 * 4095 + 8
DIFFERS_FROM_REFERENCE_RULE = [(67, 35, 16, 2, 0), (67, 35, 16, 2, 3)]


def _oracle():
    from oracle import oracle as O
    O.build()
    return O


@pytest.fixture(scope="module")
def sm_mod():
    import gpu_stereo_matching_amd as sm
    return sm


@pytest.fixture(scope="module")
def matcher(sm_mod):
    m = sm_mod.BlockMatcher(0, 640, 370, 256)
    yield m
    m.close()


@pytest.fixture(scope="module")
def wide_matcher(sm_mod):
    m = sm_mod.BlockMatcher(0, 4096, 8, 96)
    yield m
    m.close()


@functools.lru_cache(maxsize=None)
def _pair(W, H, D):
    L, R = fuzz_pair(np.random.default_rng(W * 131 + H * 17 + D), W, H)
    L.setflags(write=False)
    R.setflags(write=False)
    return L, R


@functools.lru_cache(maxsize=None)
def _case(case, rule=IV):
    """(L, R, reference) of a shape, computed once and shared by its costs and path counts."""
    W, H, D, r, d0 = case
    L, R = _pair(W, H, D)
    return L, R, pairs_ref.Reference(L, R, r, D, rule, d0 if rule == IV else 0)


def _check_subpix(m, L, R, r, D, agg, cost, ref, paths, combos, tag):
    try:
        for u, lr in combos:
            m.set_uniqueness(u)
            q, qr, qm = m.match_subpix(L, R, r, D, agg=agg, cost=cost, lr_check=lr, return_right=True, return_mask=True,
                                       pairs=IV)
            wq, wqr, wqm = ref.subpix(agg, cost, u, lr, paths)
            assert np.array_equal(q, wq), f"{tag} u={u} lr={lr}: q"
            assert np.array_equal(qr, wqr), f"{tag} u={u} lr={lr}: right-view q"
            assert np.array_equal(qm, wqm), f"{tag} u={u} lr={lr}: mask"
    finally:
        m.set_uniqueness(0)


def _check_8bit(m, L, R, r, D, agg, cost, ref, paths, tag):
    dl, dr, checked, mask = ref.maps(agg, cost, paths)
    assert np.array_equal(m.match(L, R, r, D, agg=agg, cost=cost, pairs=IV), dl), f"{tag}: left map"
    c, rr, mm = m.match_lr(L, R, r, D, agg=agg, cost=cost, pairs=IV)
    assert np.array_equal(rr, dr), f"{tag}: right map"
    assert np.array_equal(c, checked), f"{tag}: checked map"
    assert np.array_equal(mm, mask), f"{tag}: mask"


def _check(m, L, R, r, D, d0, ref, tag, combos=SUBPIX_COMBOS, eight_bit=True, paths_list=(4, 8)):
    """Every path of one pair under the in-view rule and the minimum disparity d0."""
    m.set_min_disp(d0)
    try:
        for paths in paths_list:
            m.set_sgm_paths(paths)
            for cost in COSTS:
                t = f"{tag} sgm+{cost}, {paths} paths"
                if eight_bit:
                    _check_8bit(m, L, R, r, D, "sgm", cost, ref, paths, t)
                _check_subpix(m, L, R, r, D, "sgm", cost, ref, paths, combos, t)
        if eight_bit:
            _check_8bit(m, L, R, r, D, "box", "census", ref, None, f"{tag} box+census")
        for cost in COSTS:   # the census box WTA, and the AD box volume that the sub-pixel calls alone keep
            _check_subpix(m, L, R, r, D, "box", cost, ref, None, combos, f"{tag} box+{cost}")
    finally:
        m.set_sgm_paths(4)
        m.set_min_disp(0)


# ---- 1. the shapes ----
@pytest.mark.parametrize("case", CASES + SUBPIX_ONLY_CASES, ids=lambda c: "x".join(map(str, c)))
def test_shapes(matcher, wide_matcher, case):
    W, H, D, r, d0 = case
    L, R, ref = _case(case)
    if case in DIFFERS_FROM_REFERENCE_RULE:
        other = _case(case, "reference")[2].maps("sgm", "ad")[0]
        assert not np.array_equal(other, ref.maps("sgm", "ad")[0]), "the case no longer tells the two rules apart"
    if d0 >= W:
        assert all(not a.any() for a in ref.maps("sgm", "ad")) and not any(a.any() for a in ref.subpix("sgm", "ad"))
    if case in SUBPIX_ONLY_CASES:
        assert int(ref.subpix("sgm", "ad")[0].max()) > 16 * 4000 and d0 + D - 1 == 4095
    _check(wide_matcher if W > WIDE else matcher, L, R, r, D, d0, ref, str(case),
           eight_bit=case not in SUBPIX_ONLY_CASES)


def test_eight_bit_bound(matcher, sm_mod):
    """300 x 4, D = 6: d0 = 250 is the last minimum disparity of the 8-bit calls; 251 is refused by them, naming the
    parameter and leaving the output alone, and taken by the sub-pixel call."""
    W, H, D, r = 300, 4, 6, 1
    L, R = _pair(W, H, D)
    ref = pairs_ref.Reference(L, R, r, D, IV, 251)
    matcher.set_min_disp(251)
    try:
        out = np.full((H, W), 0xAB, np.uint8)
        for agg, cost in (("sgm", "ad"), ("sgm", "census"), ("box", "census")):
            with pytest.raises(sm_mod.SMError, match="SM_PARAM_MIN_DISP"):
                matcher.match(L, R, r, D, agg=agg, cost=cost, pairs=IV, out=out)
            with pytest.raises(sm_mod.SMError, match="SM_PARAM_MIN_DISP"):
                matcher.match_lr(L, R, r, D, agg=agg, cost=cost, pairs=IV)
        assert (out == 0xAB).all()
        for cost in COSTS:
            _check_subpix(matcher, L, R, r, D, "sgm", cost, ref, None, SUBPIX_COMBOS, f"d0=251 sgm+{cost}")
    finally:
        matcher.set_min_disp(0)


# ---- 2. the 16-bit bound ----
def test_path_costs_at_65535(matcher):
    """The largest P2 that sgm_check admits at r = 2 on the two 0 / 255 pairs of test_gpu_volume_variants.py, under the
    in-view rule with eight paths: some path cost of the reference reaches 65535 exactly (asserted here), so a
    saturating or 15-bit L would change S, which the sub-pixel maps read.  It is the tied pair that reaches it, in
    every direction; the plain pair's largest L under this rule is 64005 (it lost the d > x pairs that held its
    65535 under the reference's rule), and it runs all the same."""
    r = 2
    W, H, D = BOUND_SHAPE
    p2 = bound_p2(r, "ad")
    assert p2 == 65535 - 255 * (2 * r + 1) ** 2
    E = pairs_ref.exists(IV, D, W)
    E3 = np.broadcast_to(E[:, None, :], (D, H, W))
    tops = {}
    refs = {}
    for kind in ("plain", "tied"):
        L, R = bound_input(kind, r)
        refs[kind] = ref = pairs_ref.Reference(L, R, r, D, IV, 0, 0, p2)
        tops[kind] = max(int(pairs_ref.path(ref.cost("ad"), rho, *ref.penalties("ad"), E)[E3].max())
                         for rho in sgm_paths_ref.directions(8))
    print("largest in-view path cost:", tops)
    assert tops["tied"] == 65535 and max(tops.values()) == 65535, tops
    matcher.set_sgm_penalties(0, p2)
    try:
        for kind in ("plain", "tied"):
            L, R = bound_input(kind, r)
            matcher.set_min_disp(0)
            for paths in (4, 8):
                matcher.set_sgm_paths(paths)
                _check_8bit(matcher, L, R, r, D, "sgm", "ad", refs[kind], paths, f"bound {kind} {paths} paths")
                _check_subpix(matcher, L, R, r, D, "sgm", "ad", refs[kind], paths,
                              [(0, False), (0, True), (10, False), (10, True)], f"bound {kind} {paths} paths")
    finally:
        matcher.set_sgm_paths(4)
        matcher.set_sgm_penalties()


# ---- 3. seeded fuzz ----
FUZZ_SEEDS = 12
_EDGE_D = (33, 63, 64, 65, 97, 127, 128, 129, 191, 192, 193, 201, 255, 256)


def fuzz_case(seed):
    """(W, H, D, r, d0, L, R, lr, u, paths) of one seed; the order of the draws is part of the case."""
    rng = np.random.default_rng(9900 + seed)
    W, H, r = int(rng.integers(1, 321)), int(rng.integers(1, 49)), int(rng.integers(0, 8))
    D = int(rng.integers(1, 257)) if rng.random() < 0.5 else int(rng.choice(_EDGE_D))
    d0 = (0, 1, W // 3, W - 1)[seed % 4]
    L, R = fuzz_pair(rng, W, H)
    lr, u, paths = bool(rng.integers(0, 2)), int(rng.choice((0, 10))), int(rng.choice((4, 8)))
    return W, H, D, r, d0, L, R, lr, u, paths


@pytest.mark.parametrize("seed", range(FUZZ_SEEDS))
def test_fuzz(matcher, seed):
    W, H, D, r, d0, L, R, lr, u, paths = fuzz_case(seed)
    ref = pairs_ref.Reference(L, R, r, D, IV, d0)
    _check(matcher, L, R, r, D, d0, ref, f"(seed, W, H, D, r, d0, paths) = {(seed, W, H, D, r, d0, paths)}",
           combos=[(u, lr)], eight_bit=d0 + D - 1 <= 255, paths_list=(paths,))


# ---- 4. around the flag and the parameter ----
def test_pipeline_order_median_lr_speckle_fill(matcher):
    """S -> both views' WTA on absolute disparities -> 7x7 median of both maps -> LR check -> speckle filter on the
    checked map and the mask -> row fill on the map alone, with d0 = 3."""
    case = (67, 35, 16, 2, 3)
    W, H, D, r, d0 = case
    L, R, ref = _case(case)
    O = _oracle()
    dl, dr, checked, mask = pairs_ref.maps8(ref.volume("sgm", "ad")[0], IV, d0, median=lambda a: O.median(a, 3))
    spk, spk_mask = speckle_ref.speckle(checked, 20, 1, mask)
    want = fill_ref.fill(spk, 12)
    assert not np.array_equal(checked, spk) and not np.array_equal(spk, want)   # both steps do something here
    matcher.set_min_disp(d0)
    matcher.set_speckle(20, 1)
    matcher.set_fill(12)
    try:
        c, rr, mm = matcher.match_lr(L, R, r, D, agg="sgm", median=True, pairs=IV)
    finally:
        matcher.set_fill(0)
        matcher.set_speckle()
        matcher.set_min_disp(0)
    assert np.array_equal(rr, dr) and np.array_equal(c, want) and np.array_equal(mm, spk_mask)


@pytest.mark.parametrize("dtype", ["int16", "int32"])
def test_caller_volume(matcher, dtype):
    """sm_volume_wta_subpix_device on a caller's volume: plane k is d0 + k, both views, the threshold, the check."""
    import torch
    D, H, W, d0 = 11, 9, 70, 5
    rng = np.random.default_rng(77)
    V = rng.integers(0, 3000, (D, H, W)).astype(dtype)
    vt = torch.from_numpy(V).cuda()
    matcher.set_min_disp(d0)
    try:
        for u, inv, lr in ((0, 0, False), (10, 0, True), (0, 400, True)):
            matcher.set_uniqueness(u)
            rt = torch.empty((H, W), dtype=torch.int16, device="cuda")
            mt = torch.empty((H, W), dtype=torch.uint8, device="cuda")
            qt = matcher.volume_wta_subpix_device(vt, inv, lr, right_t16=rt, mask_t=mt, pairs=IV)
            torch.cuda.synchronize()
            wq, wqr, wqm = pairs_ref.subpix(V, IV, d0, u, inv, lr)
            assert np.array_equal(qt.cpu().numpy().view(np.uint16), wq), (u, inv, lr)
            assert np.array_equal(rt.cpu().numpy().view(np.uint16), wqr), (u, inv, lr)
            assert np.array_equal(mt.cpu().numpy(), wqm), (u, inv, lr)
    finally:
        matcher.set_uniqueness(0)
        matcher.set_min_disp(0)


def test_device_calls_on_sub_frames(matcher):
    """match_device on a batch that starts inside a larger tensor, and match_subpix_device on frames cut out of a
    larger tensor (row and frame strides passed on)."""
    import torch
    case = (67, 35, 16, 2, 3)
    W, H, D, r, d0 = case
    L, R, ref = _case(case)
    big_l = torch.zeros((4, H, W), dtype=torch.uint8, device="cuda")
    big_r = torch.zeros_like(big_l)
    Lt, Rt = torch.tensor(L, device="cuda"), torch.tensor(R, device="cuda")   # (the cached pair is read-only)
    big_l[1:3] = Lt
    big_r[1:3] = Rt
    pad_l = torch.zeros((2, H + 6, W + 10), dtype=torch.uint8, device="cuda")
    pad_r = torch.zeros_like(pad_l)
    pad_l[:, 2:2 + H, 7:7 + W] = Lt
    pad_r[:, 2:2 + H, 7:7 + W] = Rt
    matcher.set_min_disp(d0)
    try:
        for cost in COSTS:
            out = matcher.match_device(big_l[1:3], big_r[1:3], r, D, agg="sgm", cost=cost, pairs=IV)
            lr_out = matcher.match_device(big_l[1:3], big_r[1:3], r, D, agg="sgm", cost=cost, lr_check=True, pairs=IV)
            q = matcher.match_subpix_device(pad_l[:, 2:2 + H, 7:7 + W], pad_r[:, 2:2 + H, 7:7 + W], r, D, agg="sgm",
                                            cost=cost, pairs=IV)
            torch.cuda.synchronize()
            dl, _, checked, _ = ref.maps("sgm", cost)
            for f in range(2):
                assert np.array_equal(out[f].cpu().numpy(), dl), cost
                assert np.array_equal(lr_out[f].cpu().numpy(), checked), cost
                assert np.array_equal(q[f].cpu().numpy().view(np.uint16), ref.subpix("sgm", cost)[0]), cost
    finally:
        matcher.set_min_disp(0)


def test_switching_back_restores_the_default(sm_mod):
    case = (67, 35, 16, 2, 3)
    W, H, D, r, d0 = case
    L, R, ref = _case(case)
    default = _case(case, "reference")[2]
    with sm_mod.BlockMatcher(0, 96, 40, 16) as m:
        for agg, cost in (("sgm", "ad"), ("box", "census")):
            want = default.maps(agg, cost)[0]
            assert np.array_equal(m.match(L, R, r, D, agg=agg, cost=cost), want)
            m.set_min_disp(d0)
            assert np.array_equal(m.match(L, R, r, D, agg=agg, cost=cost, pairs=IV), ref.maps(agg, cost)[0])
            m.set_min_disp(0)
            at_zero = _case(case[:4] + (0,))[2].maps(agg, cost)[0]
            assert np.array_equal(m.match(L, R, r, D, agg=agg, cost=cost, pairs=IV), at_zero)
            assert np.array_equal(m.match(L, R, r, D, agg=agg, cost=cost), want)           # flag off again
            assert np.array_equal(m.match(L, R, r, D, agg=agg, cost=cost, pairs="reference"), want)
            q = m.match_subpix(L, R, r, D, agg=agg, cost=cost)
            assert np.array_equal(q, default.subpix(agg, cost)[0])
        m.set_min_disp(d0)
        m.set_min_disp()
        assert np.array_equal(m.match(L, R, r, D, agg="sgm"), default.maps("sgm", "ad")[0])


@pytest.mark.parametrize("d0", [-1, 4096, 2.5, float("nan")])
def test_other_minimum_disparities_are_refused(sm_mod, d0):
    with sm_mod.BlockMatcher(0, 96, 40, 16) as m:
        with pytest.raises(sm_mod.SMError, match="minimum disparity"):
            m.set_min_disp(d0)
    with sm_mod.BlockMatcherGroup([0], 96, 40, 16) as g:
        with pytest.raises(sm_mod.SMError, match="minimum disparity"):
            g.set_min_disp(d0)


def test_calls_that_refuse_the_flag(sm_mod):
    """Each refusal comes before any device work: the output buffer keeps its bytes and the message names the flag."""
    import torch
    W, H, D, r = 320, 256, 16, 2          # the smallest frame SM_DEVICE_CU_GRID takes
    L, R = _pair(W, H, D)
    Lt, Rt = torch.tensor(L, device="cuda"), torch.tensor(R, device="cuda")
    with sm_mod.BlockMatcher(0, W, H, D) as m:
        out = np.full((H, W), 0xAB, np.uint8)
        for agg in ("box", "guided", "box-staged", "device-cu"):
            with pytest.raises(sm_mod.SMError, match="SM_PAIRS_IN_VIEW"):
                m.match(L, R, r, D, agg=agg, pairs=IV, out=out)
        assert (out == 0xAB).all()
        with pytest.raises(sm_mod.SMError, match="SM_PAIRS_IN_VIEW"):
            m.match_lr(L, R, r, D, pairs=IV)
        with pytest.raises(sm_mod.SMError, match="SM_PAIRS_IN_VIEW"):
            m.match_bgr(np.dstack([L] * 3), np.dstack([R] * 3), r, D, pairs=IV)
        out_t = torch.full((H, W), 0xAB, dtype=torch.uint8, device="cuda")
        for agg in ("box", "guided", "box-staged"):
            with pytest.raises(sm_mod.SMError, match="SM_PAIRS_IN_VIEW"):
                m.match_device(Lt, Rt, r, D, out_t=out_t, agg=agg, pairs=IV)
        with pytest.raises(sm_mod.SMError, match="SM_PAIRS_IN_VIEW"):
            m.match_device(Lt, Rt, r, D, out_t=out_t, agg="guided", cost="census", pairs=IV)
        torch.cuda.synchronize()
        assert bool((out_t == 0xAB).all())
        with pytest.raises(sm_mod.SMError, match="SM_PAIRS_IN_VIEW"):
            m.dslice_rehearse(L, R, r, D, 2, pairs=IV)
        with pytest.raises(sm_mod.SMError, match="SM_PAIRS_IN_VIEW"):
            m.slice_keys_lr_device(Lt, Rt, r, 0, D, pairs=IV)
    with sm_mod.BlockMatcherGroup([0], W, H, D) as g:
        for agg, cost in (("box", "ad"), ("sgm", "ad"), ("box", "census")):
            with pytest.raises(sm_mod.SMError, match="SM_PAIRS_IN_VIEW"):
                g.match(L, R, r, D, agg=agg, cost=cost, pairs=IV)
        with pytest.raises(sm_mod.SMError, match="SM_PAIRS_IN_VIEW"):
            g.match_lr(L, R, r, D, pairs=IV)
        with pytest.raises(sm_mod.SMError, match="SM_PAIRS_IN_VIEW"):
            g.match_dslice(L, R, r, D, pairs=IV)
        with pytest.raises(sm_mod.SMError, match="SM_PAIRS_IN_VIEW"):
            g.match_batch([L], [R], r, D, pairs=IV)            # the 8-bit AD box call


def test_minimum_disparity_needs_the_flag(sm_mod):
    """With d0 > 0 every matching call without SM_PAIRS_IN_VIEW is refused, naming the parameter, before any device
    work."""
    import torch
    W, H, D, r = 67, 35, 16, 2
    L, R = _pair(W, H, D)
    Lt, Rt = torch.tensor(L, device="cuda"), torch.tensor(R, device="cuda")
    name = "SM_PARAM_MIN_DISP"
    with sm_mod.BlockMatcher(0, 96, 40, 16) as m:
        m.set_min_disp(3)
        out = np.full((H, W), 0xAB, np.uint8)
        for agg, cost in (("box", "ad"), ("guided", "ad"), ("box-staged", "ad"), ("sgm", "ad"), ("sgm", "census"),
                          ("box", "census")):
            with pytest.raises(sm_mod.SMError, match=name):
                m.match(L, R, r, D, agg=agg, cost=cost, out=out)
        assert (out == 0xAB).all()
        with pytest.raises(sm_mod.SMError, match=name):
            m.match_lr(L, R, r, D)
        with pytest.raises(sm_mod.SMError, match=name):
            m.match_bgr(np.dstack([L] * 3), np.dstack([R] * 3), r, D)
        with pytest.raises(sm_mod.SMError, match=name):
            m.match_device(Lt, Rt, r, D)
        for agg in ("box", "sgm"):
            with pytest.raises(sm_mod.SMError, match=name):
                m.match_subpix(L, R, r, D, agg=agg)
            with pytest.raises(sm_mod.SMError, match=name):
                m.match_subpix_device(Lt, Rt, r, D, agg=agg)
        with pytest.raises(sm_mod.SMError, match=name):
            m.volume_wta_subpix_device(torch.zeros((D, H, W), dtype=torch.int16, device="cuda"))
        with pytest.raises(sm_mod.SMError, match=name):
            m.slice_keys_device(Lt, Rt, r, 0, D)
        with pytest.raises(sm_mod.SMError, match=name):
            m.guided_slice_keys_device(Lt, Rt, r, 0, D)
        with pytest.raises(sm_mod.SMError, match=name):
            m.slice_keys_lr_device(Lt, Rt, r, 0, D)
        with pytest.raises(sm_mod.SMError, match=name):
            m.dslice_rehearse(L, R, r, D, 2)
        m.set_min_disp(0)
        m.match(L, R, r, D)   # and the handle is back to normal
    with sm_mod.BlockMatcherGroup([0], 96, 40, 16) as g:
        g.set_min_disp(3)
        with pytest.raises(sm_mod.SMError, match=name):
            g.match(L, R, r, D)
        with pytest.raises(sm_mod.SMError, match=name):
            g.match_lr(L, R, r, D)
        with pytest.raises(sm_mod.SMError, match=name):
            g.match_dslice(L, R, r, D)
        with pytest.raises(sm_mod.SMError, match=name):
            g.match_batch([L], [R], r, D, agg="sgm")


def test_group_batch(matcher, sm_mod):
    """A one-member group forwards the flag and the parameter: its match_batch equals the single handle's maps."""
    case = (67, 35, 16, 2, 3)
    W, H, D, r, d0 = case
    L, R, ref = _case(case)
    with sm_mod.BlockMatcherGroup([0], W, H, D) as g:
        g.set_min_disp(d0)
        for agg, cost in (("sgm", "ad"), ("sgm", "census"), ("box", "census")):
            outs = g.match_batch([L, L], [R, R], r, D, agg=agg, cost=cost, pairs=IV)
            assert all(np.array_equal(o, ref.maps(agg, cost)[0]) for o in outs), (agg, cost)
            outs = g.match_batch([L], [R], r, D, agg=agg, cost=cost, lr_check=True, pairs=IV)
            assert np.array_equal(outs[0], ref.maps(agg, cost)[2]), (agg, cost)
        g.set_min_disp(0)
        default = _case(case, "reference")[2]
        assert np.array_equal(g.match_batch([L], [R], r, D, agg="sgm")[0], default.maps("sgm", "ad")[0])
