"""GPU SGM with eight paths (SM_PARAM_SGM_PATHS 8) against the numpy restatement (tests/sgm_paths_ref.py).

Every shape runs through match, match_lr, match_subpix and match_subpix with the LR check and uniqueness 10, on the
AD and the census cost; the shapes of test_shapes run with four paths as well, through the same kernel's vertical
form.  The sub-pixel maps matter: they depend on S itself, where the 8-bit maps can agree between
four and eight paths.  Integer arithmetic end to end: every comparison is np.array_equal.
"""
import functools

import numpy as np
import pytest

import fill_ref
import sgm_paths_ref
import sgm_ref
import speckle_ref
import subpix_ref
from fuzz_util import fuzz_pair
from test_volume_variants_model import BOUND_RADII, BOUND_SHAPE, Reference, bound_input, bound_p2

pytestmark = pytest.mark.gpu

COSTS = ("ad", "census")
SUBPIX_COMBOS = [(0, False), (10, True)]   # uniqueness, lr_check
WIDE = 640

# W, H, D, r: where a sliding, wrapping, chunked scan can go wrong (32-column tiles, kPF = 4 rows in flight, chunks of
# 2 / 4 / 8 disparities up to D = 64 / 128 / 256)
CASES = [
    (67, 35, 16, 2),     # three tiles, the last partial: the wrap goes through the padding
    (32, 3, 8, 0),       # exactly one tile: the wrap with no padding; fewer rows than the prefetch holds
    (31, 6, 8, 1),       # one column short of a tile
    (33, 7, 65, 1),      # one column past a tile; a lone d in the last chunk of 4
    (40, 33, 64, 0),     # W < D: the existing d grow and shrink along every diagonal
    (96, 5, 256, 3),     # full D, 32 chunks of 8; H = kPF + 1
    (64, 4, 8, 0),       # H = kPF
    (64, 1, 8, 0),       # a single row: every path is C
    (9, 40, 5, 7),       # H >> W: every lane wraps and restarts several times
    (1, 9, 2, 0),        # a single column: every step restarts
    (130, 9, 70, 1),     # D crosses into the chunks of 4
    (4096, 2, 20, 0),    # the width limit: 128 tiles
]
DIFFERS_FROM_FOUR_PATHS = [(67, 35, 16, 2), (40, 33, 64, 0)]   # a kernel that ran four paths fails the 8-bit map here


class PathsReference(Reference):
    """test_volume_variants_model.Reference with the path count: the costs, penalties, WTA, LR check and the
    sub-pixel maps are its own; S comes from sgm_paths_ref."""

    def __init__(self, oracle, L, R, r, D, p1=0, p2=0, paths=8):
        super().__init__(oracle, L, R, r, D, p1, p2)
        self.paths = paths

    @functools.lru_cache(maxsize=None)
    def _wta(self, agg, cost):
        assert agg == "sgm"
        return sgm_paths_ref.aggregate(self.cost(cost), *self.penalties(cost), self.paths)


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
    m.set_sgm_paths(8)
    yield m
    m.close()


@pytest.fixture(scope="module")
def wide_matcher(sm_mod):
    m = sm_mod.BlockMatcher(0, 4096, 8, 64)
    m.set_sgm_paths(8)
    yield m
    m.close()


@functools.lru_cache(maxsize=None)
def _case(case, paths=8):
    """(L, R, reference) of a shape and a path count, computed once and shared by its costs."""
    W, H, D, r = case
    L, R = fuzz_pair(np.random.default_rng(W * 131 + H * 17 + D), W, H)
    L.setflags(write=False)
    R.setflags(write=False)
    return L, R, PathsReference(_oracle(), L, R, r, D, paths=paths)


def _check(m, L, R, r, D, cost, ref, combos, tag):
    """The four calls of one (pair, cost) against the reference."""
    dl, dr, checked, mask = ref.maps("sgm", cost)
    assert np.array_equal(m.match(L, R, r, D, agg="sgm", cost=cost), dl), f"{tag}: left map"
    c, rr, mm = m.match_lr(L, R, r, D, agg="sgm", cost=cost)
    assert np.array_equal(rr, dr), f"{tag}: right map"
    assert np.array_equal(c, checked), f"{tag}: checked map"
    assert np.array_equal(mm, mask), f"{tag}: mask"
    try:
        for u, lr in combos:
            m.set_uniqueness(u)
            q, qr, qm = m.match_subpix(L, R, r, D, agg="sgm", cost=cost, lr_check=lr, return_right=True,
                                       return_mask=True)
            wq, wqr, wqm = ref.subpix("sgm", cost, u, lr)
            assert np.array_equal(q, wq), f"{tag} u={u} lr={lr}: q"
            assert np.array_equal(qr, wqr), f"{tag} u={u} lr={lr}: right-view q"
            assert np.array_equal(qm, wqm), f"{tag} u={u} lr={lr}: mask"
    finally:
        m.set_uniqueness(0)


# ---- 1. the shapes ----
# With four paths too: the vertical walk is the diagonal one's code (sgm_col_kernel), and only these shapes put few
# rows, one column and the width limit to it.  The eight-path cases keep their ids.
@pytest.mark.parametrize("cost", COSTS)
@pytest.mark.parametrize("case, paths", [
    pytest.param(c, p, id="x".join(map(str, c)) + ("" if p == 8 else "-4paths")) for p in (8, 4) for c in CASES])
def test_shapes(matcher, wide_matcher, case, paths, cost):
    W, H, D, r = case
    L, R, ref = _case(case, paths)
    if paths == 8 and case in DIFFERS_FROM_FOUR_PATHS:
        four = _case(case, 4)[2].maps("sgm", cost)[0]
        assert not np.array_equal(four, ref.maps("sgm", cost)[0]), "the case no longer tells 4 paths from 8"
    m = wide_matcher if W > WIDE else matcher
    m.set_sgm_paths(paths)
    try:
        _check(m, L, R, r, D, cost, ref, SUBPIX_COMBOS, f"{case} sgm+{cost}, {paths} paths")
    finally:
        m.set_sgm_paths(8)


# ---- 2. the 16-bit bound ----
@pytest.mark.parametrize("r", BOUND_RADII)
@pytest.mark.parametrize("kind", ["plain", "tied"])
def test_diagonal_path_costs_at_65535(matcher, kind, r):
    """The largest P2 that sgm_check admits on the 0 / 255 pairs of test_gpu_volume_variants.py: the reference's
    diagonal path costs reach 65535 exactly (asserted here), so a saturating or 15-bit L would change S, which the
    sub-pixel maps read."""
    W, H, D = BOUND_SHAPE
    L, R = bound_input(kind, r)
    p2 = bound_p2(r, "ad")
    assert p2 == 65535 - 255 * (2 * r + 1) ** 2
    ref = PathsReference(_oracle(), L, R, r, D, 0, p2)
    E = subpix_ref.left_exists(D, H, W)
    top = [int(sgm_paths_ref.diagonal_path(ref.cost("ad"), rho, *ref.penalties("ad"))[E].max())
           for rho in sgm_paths_ref.DIAGONALS]
    assert max(top) == 65535, top
    matcher.set_sgm_penalties(0, p2)
    try:
        _check(matcher, L, R, r, D, "ad", ref, [(0, False), (0, True), (10, False), (10, True)], f"bound {kind} r={r}")
    finally:
        matcher.set_sgm_penalties()


# ---- 3. seeded fuzz ----
FUZZ_SEEDS = 16
# 64 k +- 1 (a half wave's worth of chunks more or less) and the chunk boundaries: a lone d in the last chunk of
# 2 / 4 / 8, and the last D of each chunk size
_EDGE_D = (33, 63, 64, 65, 97, 127, 128, 129, 191, 192, 193, 201, 255, 256)


def fuzz_case(seed):
    """(W, H, D, r, L, R, lr, u) of one seed; the order of the draws is part of the case."""
    rng = np.random.default_rng(8800 + seed)
    W, H, r = int(rng.integers(1, 321)), int(rng.integers(1, 49)), int(rng.integers(0, 8))
    D = int(rng.integers(1, 257)) if rng.random() < 0.5 else int(rng.choice(_EDGE_D))
    L, R = fuzz_pair(rng, W, H)
    lr, u = bool(rng.integers(0, 2)), int(rng.choice((0, 10)))
    return W, H, D, r, L, R, lr, u


@pytest.mark.parametrize("seed", range(FUZZ_SEEDS))
def test_fuzz(matcher, seed):
    W, H, D, r, L, R, lr, u = fuzz_case(seed)
    ref = PathsReference(_oracle(), L, R, r, D)
    for cost in COSTS:
        _check(matcher, L, R, r, D, cost, ref, [(u, lr)], f"(seed, W, H, D, r, cost) = {(seed, W, H, D, r, cost)}")


# ---- 4. around the parameter ----
def test_pipeline_order_median_lr_speckle_fill(matcher):
    """S of eight paths -> both views' WTA -> 7x7 median of both maps -> LR check -> speckle filter on the checked
    map and the mask -> row fill on the map alone."""
    case = (67, 35, 16, 2)
    W, H, D, r = case
    L, R, ref = _case(case)
    O = _oracle()
    dl, dr, checked, mask = sgm_paths_ref.maps(O, *ref._wta("sgm", "ad"), median=True)
    spk, spk_mask = speckle_ref.speckle(checked, 20, 1, mask)
    want = fill_ref.fill(spk, 12)
    assert not np.array_equal(checked, spk) and not np.array_equal(spk, want)   # both steps do something here
    matcher.set_speckle(20, 1)
    matcher.set_fill(12)
    try:
        c, rr, mm = matcher.match_lr(L, R, r, D, agg="sgm", median=True)
    finally:
        matcher.set_fill(0)
        matcher.set_speckle()
    assert np.array_equal(rr, dr) and np.array_equal(c, want) and np.array_equal(mm, spk_mask)


def test_back_to_four_paths(sm_mod):
    case = (67, 35, 16, 2)
    W, H, D, r = case
    L, R, ref = _case(case)
    four = sgm_ref.sgm_lr(_oracle(), L, R, r, D, *sgm_ref.auto_penalties(r))[0]
    with sm_mod.BlockMatcher(0, 96, 40, 16) as m:
        assert np.array_equal(m.match(L, R, r, D, agg="sgm"), four)   # the default
        m.set_sgm_paths(8)
        assert np.array_equal(m.match(L, R, r, D, agg="sgm"), ref.maps("sgm", "ad")[0])
        m.set_sgm_paths(4)
        assert np.array_equal(m.match(L, R, r, D, agg="sgm"), four)
        m.set_sgm_paths(8)
        m.set_sgm_paths()
        assert np.array_equal(m.match(L, R, r, D, agg="sgm"), four)


@pytest.mark.parametrize("paths", [5, 0, 16, 4.5, -8])
def test_other_path_counts_are_refused(sm_mod, paths):
    with sm_mod.BlockMatcher(0, 96, 40, 16) as m:
        with pytest.raises(sm_mod.SMError, match="paths"):
            m.set_sgm_paths(paths)
    with sm_mod.BlockMatcherGroup([0], 96, 40, 16) as g:
        with pytest.raises(sm_mod.SMError, match="paths"):
            g.set_sgm_paths(paths)


def test_group_batch(matcher, sm_mod):
    """A one-member group forwards the parameter: its match_batch equals the single handle's maps."""
    case = (67, 35, 16, 2)
    W, H, D, r = case
    L, R, ref = _case(case)
    single = matcher.match(L, R, r, D, agg="sgm")
    assert np.array_equal(single, ref.maps("sgm", "ad")[0])
    with sm_mod.BlockMatcherGroup([0], W, H, D) as g:
        g.set_sgm_paths(8)
        outs = g.match_batch([L, L], [R, R], r, D, agg="sgm")
        assert all(np.array_equal(o, single) for o in outs)
        g.set_sgm_paths(4)
        four = sgm_ref.sgm_lr(_oracle(), L, R, r, D, *sgm_ref.auto_penalties(r))[0]
        assert all(np.array_equal(o, four) for o in g.match_batch([L, L], [R, R], r, D, agg="sgm"))
