"""CPU part of the cost-volume variant tests (tests/test_gpu_volume_variants.py): the cases and inputs the GPU file
runs, and what can be shown about them without a GPU.

  * the launchers' selection rules restated in Python, and the assertion that the variant table plus the shapes of
    the older SGM / census / sub-pixel tests reach every compiled variant of the path;
  * the 16-bit bound inputs reach L = 65535 exactly on the reference (AD), and the census cost passes 32767 at r = 7;
  * the cases discriminate: wrong variants of the recursion, written here on the numpy side, change the expected
    maps of the cases aimed at them;
  * the reference with shared cost volumes that the GPU file uses equals sgm_ref / census_ref / subpix_ref.

Integer arithmetic end to end: every comparison is np.array_equal.
"""
import functools

import numpy as np
import pytest

import census_ref
import sgm_ref
import subpix_ref
from fuzz_util import fuzz_pair

PATHS8 = [("box", "census"), ("sgm", "ad"), ("sgm", "census")]   # box + ad is the fused kernel, not a volume path
PATHS16 = [("box", "ad")] + PATHS8                               # the sub-pixel calls keep a volume for it too

# ---- the variant table: (W, H, D, r), the fuzz_pair seed, and what the launchers select for it ----
# h: sgm_h_kernel<NJ, VEC>; v: sgm_col_kernel<DPT, DIAG> with (d chunks, threads); cv: census_volume_kernel<VEC> with the rows
# per block that the width leaves; ad: ad_volume_kernel<KF>.  test_table_selects_what_it_says holds these to `select`.
VARIANT_CASES = [
    # three registers per lane, scalar staging: lanes 0..42 are full (d = 128 is lane 42's third register), lane 43
    # would start at d = 129 = D and holds nothing; 17 chunks = 544 threads, rounded to 576
    ((75, 9, 129, 2), 101, dict(h=(3, False), v=(8, 17, 576), cv=(False, 2), ad=1)),
    # three registers, 16-B staging: three full 64-column tiles and one of 8 columns; 24 chunks
    ((200, 6, 192, 1), 103, dict(h=(3, True), v=(8, 24, 768), cv=(False, 2), ad=1)),
    # D no multiple of 3: the last lane is partial; W < D
    ((72, 5, 191, 0), 110, dict(h=(3, True), v=(8, 24, 768), cv=(False, 2), ad=1)),
    # two registers per lane with a lone d = 64 in lane 32; 17 chunks of 4, the last holding that one d
    ((33, 7, 65, 1), 104, dict(h=(2, False), v=(4, 17, 576), cv=(False, 2), ad=1)),
    # four registers per lane with a lone d = 192 in lane 48; 25 chunks of 8, the last holding that one d; W < D
    ((40, 6, 193, 0), 105, dict(h=(4, True), v=(8, 25, 832), cv=(False, 2), ad=1)),
    # the widest frame with two rows per census-volume block: 2 * 128 segments = 256 threads, one d group
    ((2048, 2, 16, 1), 106, dict(h=(1, True), v=(2, 8, 256), cv=(True, 2), ad=1)),
    # one row per block, 16-B stores, three bands; the AD volume's two segments per thread with a one-row last band
    ((2064, 3, 40, 1), 107, dict(h=(1, True), v=(2, 20, 640), cv=(True, 1), ad=2)),
    # one row per block, scalar stores (W % 16 = 4); the horizontal scan walks 33 tiles with scalar staging
    ((2100, 2, 24, 2), 108, dict(h=(1, False), v=(2, 12, 384), cv=(False, 1), ad=2)),
    # the width limit: 256 segments, the padded LDS index reaches 4095 + 255
    ((4096, 2, 20, 0), 109, dict(h=(1, True), v=(2, 10, 320), cv=(True, 1), ad=2)),
]
WIDE = 640   # the cases wider than the suite's usual handle take one of their own

# Shapes (W, H, D) that the older GPU tests run through the same path: test_gpu_sgm.CASES and test_multi_tile_640x360,
# test_gpu_census.CASES and test_multi_tile, test_gpu_subpix.SHAPES.
EXISTING_SHAPES = [(67, 35, 16), (130, 9, 70), (40, 33, 64), (96, 5, 256), (64, 1, 8), (9, 40, 5), (33, 17, 1),
                   (5, 3, 4), (640, 360, 128), (637, 33, 128), (67, 9, 16), (37, 11, 64), (300, 5, 256), (64, 8, 1),
                   (64, 8, 2)]


def select(W, H, D):
    """What launch_sgm_paths, launch_census_volume and launch_ad_volume choose for a frame, as run_volume calls them
    (every volume starts 256-B aligned in the workspace, so the alignment halves of the VEC tests always hold).
    A restatement of those three launchers: it must be updated with them."""
    nj = (D + 63) // 64
    dpt = 2 if D <= 64 else (4 if D <= 128 else 8)
    chunks = (D + dpt - 1) // dpt
    nseg = (W + 15) // 16
    rb_w = 2 if 2 * nseg <= 256 else 1                  # census volume: rows per block that the width leaves
    ad_rb = min(2, H)                                   # AD volume: SM_ADV_ROWS = 2 while 2 * nseg <= 1024
    return dict(h=(nj, W % 8 == 0), v=(dpt, chunks, (32 * chunks + 63) // 64 * 64), cv=(W % 16 == 0, rb_w),
                cv_nflat=min(rb_w, H) * nseg, cv_lds_last=(W - 1) + ((W - 1) >> 4),
                ad=(ad_rb * nseg + 255) // 256)


def case_pair(case, seed):
    W, H, D, r = case
    L, R = fuzz_pair(np.random.default_rng(seed), W, H)
    L.setflags(write=False)
    R.setflags(write=False)
    return L, R


# ---- the 16-bit bound input ----
BOUND_SHAPE = (72, 20, 24)   # W, H, D
BOUND_RADII = (2, 7)


def bound_pair():
    """0 / 255 only: the left third flat, the left half of the right image the inverse of the left one (every pixel
    of a window costs 255), the right half a copy shifted by 3 (a zero-cost d next to saturated ones)."""
    W, H, D = BOUND_SHAPE
    rng = np.random.default_rng(5)
    L = np.where(rng.random((H, W)) < 0.5, 0, 255).astype(np.uint8)
    L[:, :W // 3] = 0
    R = (255 - L).astype(np.uint8)
    R[:, W // 2:] = np.roll(L, -3, axis=1)[:, W // 2:]
    L.setflags(write=False)
    R.setflags(write=False)
    return L, R


# On bound_pair a d that holds a 65535 in one direction is far from every winner, so a store that saturates one below
# the top changes no map there (400 seeds of the same construction: none does).  The second input puts such entries
# next to ties: a sparse texture (5 % zeros) matched at two shifts left and right of a band where the left image is
# 255 and the right one 0.  (seed, band start, band end, left shift, right shift) per radius, found by search on the
# reference; test_saturating_store_fault_changes_the_tied_bound_input holds them to their purpose.
TIED_BOUND = {2: (64374, 19, 47, 2, 6), 7: (240397, 12, 44, 0, 2)}


def tied_bound_pair(r):
    W, H, D = BOUND_SHAPE
    seed, a, b, s1, s2 = TIED_BOUND[r]
    rng = np.random.default_rng(seed)
    L = np.where(rng.random((H, W)) < 0.05, 0, 255).astype(np.uint8)
    R = (255 - L).astype(np.uint8)
    R[:, :a] = np.roll(L, -s1, axis=1)[:, :a]
    R[:, b:] = np.roll(L, -s2, axis=1)[:, b:]
    L[:, a:b] = 255
    R[:, a:b] = 0
    L.setflags(write=False)
    R.setflags(write=False)
    return L, R


def bound_input(kind, r):
    return bound_pair() if kind == "plain" else tied_bound_pair(r)


def bound_p2(r, cost):
    """The largest P2 sgm_check admits at this radius."""
    return 65535 - (255 if cost == "ad" else 62) * (2 * r + 1) ** 2


# ---- the seeded fuzz ----
FUZZ_SEEDS = 24
_EDGE_D = (63, 64, 65, 127, 128, 129, 191, 192, 193, 255, 256)


def fuzz_case(seed):
    """(W, H, D, r, L, R, lr, u) of one seed; the order of the draws is part of the case."""
    rng = np.random.default_rng(7000 + seed)
    W, H, r = int(rng.integers(1, 321)), int(rng.integers(1, 49)), int(rng.integers(0, 8))
    D = int(rng.integers(1, 257)) if rng.random() < 0.5 else int(rng.choice(_EDGE_D))
    L, R = fuzz_pair(rng, W, H)
    lr, u = bool(rng.integers(0, 2)), int(rng.choice((0, 10)))
    return W, H, D, r, L, R, lr, u


# ---- the reference with shared volumes ----
class Reference:
    """The expected results of every path on one pair, from the building blocks of sgm_ref.sgm_lr,
    census_ref.census_lr and subpix_ref.volume, with the AD cost, the census cost and SGM's sums computed once each
    (test_shared_reference_equals_the_references holds it to those three).  p1 / p2: 0 = auto, per cost."""

    def __init__(self, oracle, L, R, r, D, p1=0, p2=0):
        self.O, self.L, self.R, self.r, self.D, self.p1, self.p2 = oracle, L, R, r, D, p1, p2

    @functools.lru_cache(maxsize=None)
    def cost(self, cost):
        if cost == "census":
            return census_ref.cost(self.L, self.R, self.r, self.D).astype(np.int64)
        return self.O.box_cost(self.L, self.R, self.r, self.D).astype(np.int64)

    def penalties(self, cost):
        a1, a2 = (census_ref if cost == "census" else sgm_ref).auto_penalties(self.r)
        return self.p1 or a1, self.p2 or a2

    @functools.lru_cache(maxsize=None)
    def _wta(self, agg, cost):
        """(S with SENTINEL where the pair does not exist, left map)."""
        if agg == "sgm":
            return sgm_ref.aggregate(self.cost(cost), *self.penalties(cost))
        return census_ref.box_wta(self.cost(cost))

    @functools.lru_cache(maxsize=None)
    def maps(self, agg, cost):
        """(left, right, checked, mask) of the 8-bit calls."""
        S, dl = self._wta(agg, cost)
        dr = self.O.right_wta(S.astype(np.int32))
        checked, mask = self.O.lr_check(dl, dr)
        return dl, dr, checked, mask

    def volume(self, agg, cost):
        """(V, invalid_from, right_pairs), as subpix_ref.volume."""
        if agg == "sgm":
            return self._wta(agg, cost)[0], 0, 1
        if cost == "census":
            return self.cost(cost), 0, 1
        return self.cost(cost), 50 * (2 * self.r + 1) ** 2, 2

    @functools.lru_cache(maxsize=None)
    def subpix(self, agg, cost, u, lr):
        V, inv, pairs = self.volume(agg, cost)
        return subpix_ref.subpix(V, u, inv, lr, pairs)


# ---- wrong variants of the recursion ----
_INF = sgm_ref._INF


def make_step(cut=0, post=None):
    """sgm_ref._step with two optional faults: `cut` drops the d - 1 term of every d = k * cut and the d + 1 term of
    every d = k * cut - 1 (the exchange between neighbouring lanes or chunks of `cut` disparities lost); `post` is
    applied to every L before it is kept (a narrower or saturating store).  Without either it is the recursion."""
    def step(C, prev, E, P1, P2):
        if prev is None:
            v = C
        else:
            M = prev.min(axis=0)
            below = np.full_like(prev, _INF)
            below[1:] = prev[:-1]
            above = np.full_like(prev, _INF)
            above[:-1] = prev[1:]
            if cut:
                below[cut::cut] = _INF
                above[cut - 1::cut] = _INF
            v = C + np.minimum(np.minimum(prev, below + P1), np.minimum(above + P1, M[None, :] + P2)) - M[None, :]
        if post is not None:
            v = post(v)
        return np.where(E, v, _INF)
    return step


def scan(C, rho, P1, P2, step):
    """sgm_ref.path with the step handed in."""
    C = np.asarray(C, np.int64)
    D, H, W = C.shape
    E = sgm_ref.exists(D, W)
    out = np.full((D, H, W), _INF, np.int64)
    dx, dy = rho
    prev = None
    if dx:
        for x in (range(W) if dx > 0 else range(W - 1, -1, -1)):
            prev = out[:, :, x] = step(C[:, :, x], prev, np.broadcast_to(E[:, x:x + 1], (D, H)), P1, P2)
    else:
        for y in (range(H) if dy > 0 else range(H - 1, -1, -1)):
            prev = out[:, y, :] = step(C[:, y, :], prev, E, P1, P2)
    return out


def mutant_path(horizontal=None, vertical=None):
    """A path_fn for sgm_ref.aggregate: the given step along the horizontal / vertical directions, the reference's
    own path along the others."""
    def path_fn(C, rho, P1, P2):
        step = horizontal if rho[0] else vertical
        return sgm_ref.path(C, rho, P1, P2) if step is None else scan(C, rho, P1, P2, step)
    return path_fn


LANE_CUT_H = mutant_path(horizontal=make_step(cut=3))      # sgm_h_kernel<3, *>: lane ends at d = 3k - 1 | 3k
CHUNK_CUT_V = mutant_path(vertical=make_step(cut=8))       # sgm_col_kernel<8, false>: chunk ends at d = 8k - 1 | 8k
MOD_2_15 = mutant_path(make_step(post=lambda v: v % 32768), make_step(post=lambda v: v % 32768))
SAT_65534 = mutant_path(make_step(post=lambda v: np.minimum(v, 65534)), make_step(post=lambda v: np.minimum(v, 65534)))


def _changes(C, P1, P2, path_fn):
    """Does the mutant change the left map or, failing that, the sub-pixel q of either view (no filter, no check)?"""
    S, dl = sgm_ref.aggregate(C, P1, P2)
    Sm, dlm = sgm_ref.aggregate(C, P1, P2, path_fn=path_fn)
    if not np.array_equal(dl, dlm):
        return True
    (q, qr, _), (qm, qrm, _) = subpix_ref.subpix(S), subpix_ref.subpix(Sm)
    return not (np.array_equal(q, qm) and np.array_equal(qr, qrm))


# ---- the tests ----
def test_scan_harness_is_the_reference(oracle):
    """The step and scan that carry the mutants are, without a fault, sgm_ref.path itself."""
    (W, H, D, r), seed, _ = VARIANT_CASES[3]
    L, R = case_pair((W, H, D, r), seed)
    C = oracle.box_cost(L, R, r, D).astype(np.int64)
    P1, P2 = sgm_ref.auto_penalties(r)
    for rho in sgm_ref.DIRECTIONS:
        assert np.array_equal(scan(C, rho, P1, P2, make_step()), sgm_ref.path(C, rho, P1, P2)), rho


def test_table_selects_what_it_says():
    for case, _, want in VARIANT_CASES:
        got = select(*case[:3])
        assert {k: got[k] for k in want} == want, case
    by_case = {c[:3]: select(*c[:3]) for c, _, _ in VARIANT_CASES}
    assert by_case[(2048, 2, 16)]["cv_nflat"] == 256 and by_case[(4096, 2, 20)]["cv_nflat"] == 256
    assert by_case[(4096, 2, 20)]["cv_lds_last"] == 4095 + 255
    assert 2100 % 16 == 4 and (2100 + 63) // 64 == 33


def test_every_compiled_variant_is_reached():
    """Restates launch_sgm_paths (bm_sgm.hip), launch_census_volume (bm_census.hip) and launch_ad_volume
    (bm_volume.hip) through `select`, and must be updated with them: the variant table together with the shapes of
    the older tests reaches every sgm_h_kernel<NJ, VEC>, sgm_col_kernel<DPT, false>, census_volume_kernel<VEC> at one and two
    rows per block, and the two ad_volume_kernel<KF> that a width <= 4096 can select (KF = 4 needs 2 * nseg > 512)."""
    assert max(select(4096, h, 256)["ad"] for h in (1, 2, 8)) == 2
    shapes = [c[:3] for c, _, _ in VARIANT_CASES] + EXISTING_SHAPES
    sel = [select(*s) for s in shapes]
    assert {s["h"] for s in sel} == {(nj, vec) for nj in (1, 2, 3, 4) for vec in (False, True)}
    assert {s["v"][0] for s in sel} == {2, 4, 8}
    assert {s["cv"] for s in sel} == {(vec, rb) for vec in (False, True) for rb in (1, 2)}
    assert {s["ad"] for s in sel} == {1, 2}
    # what the older shapes alone leave out, which is why the table exists
    old = [select(*s) for s in EXISTING_SHAPES]
    assert not any(s["h"][0] == 3 for s in old) and not any(s["cv"][1] == 1 for s in old)
    assert {s["ad"] for s in old} == {1}


def test_fuzz_draws_reach_the_edges():
    """The 24 seeds are fixed, so what they cover is a fact: every register count of the horizontal scan, every
    chunk size of the vertical one, both staging forms, D at a wave boundary and W < D."""
    cases = [fuzz_case(s)[:4] for s in range(FUZZ_SEEDS)]
    assert all(1 <= W <= 320 and 1 <= H <= 48 and 1 <= D <= 256 and 0 <= r <= 7 for W, H, D, r in cases)
    sel = [select(W, H, D) for W, H, D, _ in cases]
    assert {s["h"][0] for s in sel} == {1, 2, 3, 4} and {s["h"][1] for s in sel} == {False, True}
    assert {s["v"][0] for s in sel} == {2, 4, 8}
    assert any(D in _EDGE_D for _, _, D, _ in cases) and any(W < D for W, _, D, _ in cases)


@pytest.mark.parametrize("r", BOUND_RADII)
@pytest.mark.parametrize("kind", ["plain", "tied"])
def test_bound_input_reaches_65535(oracle, kind, r):
    """On the bound inputs the largest cost is 255 win^2 and, with the largest P2 that sgm_check admits, the largest
    path cost of the reference is exactly 65535: the GPU test of the same input runs at the bound, not near it."""
    W, H, D = BOUND_SHAPE
    L, R = bound_input(kind, r)
    win2 = (2 * r + 1) ** 2
    C = oracle.box_cost(L, R, r, D).astype(np.int64)
    E = subpix_ref.left_exists(D, H, W)
    assert C[E].max() == 255 * win2
    P1, P2 = sgm_ref.auto_penalties(r)[0], bound_p2(r, "ad")
    assert P2 == 65535 - 255 * win2
    top = max(int(sgm_ref.path(C, rho, P1, P2)[E].max()) for rho in sgm_ref.DIRECTIONS)
    assert top == 65535


CENSUS_BOUND_TOP = {2: 17309, 7: 57441}   # the reference's largest path cost on the bound input, per radius


def test_bound_input_passes_32767_with_the_census_cost():
    """With the census cost and its largest P2 the reference's largest L on the bound input is 57441 at r = 7, past
    32767, so a signed 16-bit path cost would show there.  At r = 2 it is 17309: L - M grows by at most the largest
    cost a step (866 here, of 62 * 25) and the longest path of the 72 x 20 frame is too short for more, so that
    radius runs the admitted corner of P2 but does not guard the sign; the AD test of the same input does, at both."""
    W, H, D = BOUND_SHAPE
    L, R = bound_pair()
    E = subpix_ref.left_exists(D, H, W)
    top = {}
    for r in BOUND_RADII:
        C = census_ref.cost(L, R, r, D).astype(np.int64)
        P1, P2 = census_ref.auto_penalties(r)[0], bound_p2(r, "census")
        top[r] = max(int(sgm_ref.path(C, rho, P1, P2)[E].max()) for rho in sgm_ref.DIRECTIONS)
    assert top == CENSUS_BOUND_TOP
    assert max(top.values()) > 32767


@pytest.mark.parametrize("idx", [0, 1, 2])
def test_lane_end_fault_changes_the_three_register_cases(oracle, idx):
    case, seed, want = VARIANT_CASES[idx]
    assert want["h"][0] == 3
    W, H, D, r = case
    L, R = case_pair(case, seed)
    C = oracle.box_cost(L, R, r, D).astype(np.int64)
    assert _changes(C, *sgm_ref.auto_penalties(r), LANE_CUT_H), case


@pytest.mark.parametrize("idx", [0, 1, 2, 4])
def test_chunk_end_fault_changes_the_eight_per_chunk_cases(oracle, idx):
    case, seed, want = VARIANT_CASES[idx]
    assert want["v"][0] == 8
    W, H, D, r = case
    L, R = case_pair(case, seed)
    C = oracle.box_cost(L, R, r, D).astype(np.int64)
    assert _changes(C, *sgm_ref.auto_penalties(r), CHUNK_CUT_V), case


@pytest.mark.parametrize("r", BOUND_RADII)
@pytest.mark.parametrize("kind", ["plain", "tied"])
def test_fifteen_bit_store_fault_changes_the_bound_inputs(oracle, kind, r):
    L, R = bound_input(kind, r)
    C = oracle.box_cost(L, R, r, BOUND_SHAPE[2]).astype(np.int64)
    assert _changes(C, sgm_ref.auto_penalties(r)[0], bound_p2(r, "ad"), MOD_2_15)


@pytest.mark.parametrize("r", BOUND_RADII)
def test_saturating_store_fault_changes_the_tied_bound_input(oracle, r):
    """L saturated at 65534 instead of reaching 65535: one less in a few hundred entries of S.  It shows only where
    such an entry sits in a tie or next to a winner, which is what tied_bound_pair is built for; on bound_pair it
    changes S (1970 entries at r = 2, 402 at r = 7) and none of the maps."""
    L, R = tied_bound_pair(r)
    C = oracle.box_cost(L, R, r, BOUND_SHAPE[2]).astype(np.int64)
    assert _changes(C, sgm_ref.auto_penalties(r)[0], bound_p2(r, "ad"), SAT_65534)


def test_signed_store_fault_changes_the_census_bound_input():
    r = 7   # the radius at which the census path costs pass 32767 (CENSUS_BOUND_TOP)
    L, R = bound_pair()
    C = census_ref.cost(L, R, r, BOUND_SHAPE[2]).astype(np.int64)
    assert _changes(C, census_ref.auto_penalties(r)[0], bound_p2(r, "census"), MOD_2_15)


def test_shared_reference_equals_the_references(oracle):
    W, H, D, r = 33, 7, 20, 1
    L, R = fuzz_pair(np.random.default_rng(3), W, H)
    ref = Reference(oracle, L, R, r, D)
    for a, b in zip(ref.maps("sgm", "ad"), sgm_ref.sgm_lr(oracle, L, R, r, D, *sgm_ref.auto_penalties(r))):
        assert np.array_equal(a, b)
    for agg in ("box", "sgm"):
        for a, b in zip(ref.maps(agg, "census"), census_ref.census_lr(oracle, L, R, r, D, agg)):
            assert np.array_equal(a, b)
    for agg, cost in PATHS16:
        V, inv, pairs = ref.volume(agg, cost)
        V2, inv2, pairs2 = subpix_ref.volume(oracle, L, R, r, D, agg, cost)
        assert np.array_equal(V, V2) and (inv, pairs) == (inv2, pairs2)
    # explicit penalties reach both costs' SGM as they reach subpix_ref.volume
    ref = Reference(oracle, L, R, r, D, 7, 900)
    for cost in ("ad", "census"):
        assert np.array_equal(ref.volume("sgm", cost)[0], subpix_ref.volume(oracle, L, R, r, D, "sgm", cost, 7, 900)[0])
