"""Every kernel variant of the cost-volume path (run_volume: AD or census volume -> box sums -> SGM paths -> WTA or
sub-pixel WTA) against the numpy / C references: the variant table, the 16-bit bound of the path costs, a seeded
fuzz and the non-dense device calls of the 8-bit maps.

The cases, their inputs and the reference with shared volumes live in tests/test_volume_variants_model.py, which
also shows on the CPU which variant each case selects and that the cases discriminate.  Integer arithmetic end to
end: every comparison is np.array_equal.
"""
import functools

import numpy as np
import pytest

import census_ref
from fuzz_util import fuzz_pair
from test_volume_variants_model import (BOUND_RADII, BOUND_SHAPE, FUZZ_SEEDS, PATHS8, PATHS16, VARIANT_CASES, WIDE,
                                        Reference, bound_input, bound_p2, case_pair, fuzz_case)

pytestmark = pytest.mark.gpu

SUBPIX_COMBOS = [(0, False), (0, True), (10, False), (10, True)]   # uniqueness, lr_check
WIDE_IDX = [i for i, (c, _, _) in enumerate(VARIANT_CASES) if c[0] > WIDE]


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
    m = sm_mod.BlockMatcher(0, 4096, 8, 64)
    yield m
    m.close()


def _oracle():
    from oracle import oracle as O
    O.build()
    return O


@functools.lru_cache(maxsize=None)
def _case(idx):
    """(L, R, Reference) of a table case, computed once and shared by its paths."""
    case, seed, _ = VARIANT_CASES[idx]
    L, R = case_pair(case, seed)
    return L, R, Reference(_oracle(), L, R, case[3], case[2])


@functools.lru_cache(maxsize=None)
def _bound(kind, r, cost):
    L, R = bound_input(kind, r)
    return L, R, Reference(_oracle(), L, R, r, BOUND_SHAPE[2], 0, bound_p2(r, cost))


def _check8(m, L, R, r, D, agg, cost, ref, tag):
    dl, dr, checked, mask = ref.maps(agg, cost)
    assert np.array_equal(m.match(L, R, r, D, agg=agg, cost=cost), dl), f"{tag}: left map"
    c, rr, mm = m.match_lr(L, R, r, D, agg=agg, cost=cost)
    assert np.array_equal(rr, dr), f"{tag}: right map"
    assert np.array_equal(c, checked), f"{tag}: checked map"
    assert np.array_equal(mm, mask), f"{tag}: mask"
    assert np.array_equal(m.match(L, R, r, D, agg=agg, cost=cost, lr_check=True), checked), f"{tag}: match(lr_check)"


def _check16(m, L, R, r, D, agg, cost, ref, combos, tag):
    try:
        for u, lr in combos:
            m.set_uniqueness(u)
            q, qr, mask = m.match_subpix(L, R, r, D, agg=agg, cost=cost, lr_check=lr, return_right=True,
                                         return_mask=True)
            wq, wqr, wmask = ref.subpix(agg, cost, u, lr)
            assert np.array_equal(q, wq), f"{tag} u={u} lr={lr}: q"
            assert np.array_equal(qr, wqr), f"{tag} u={u} lr={lr}: right-view q"
            assert np.array_equal(mask, wmask), f"{tag} u={u} lr={lr}: mask"
    finally:
        m.set_uniqueness(0)


# ---- 1. the variant table ----
@pytest.mark.parametrize("agg,cost", PATHS16)
@pytest.mark.parametrize("idx", range(len(VARIANT_CASES)), ids=lambda i: "x".join(map(str, VARIANT_CASES[i][0])))
def test_variant_table(matcher, wide_matcher, idx, agg, cost):
    (W, H, D, r), _, selects = VARIANT_CASES[idx]
    L, R, ref = _case(idx)
    m = wide_matcher if W > WIDE else matcher
    tag = f"{(W, H, D, r, agg, cost)} {selects}"
    if (agg, cost) in PATHS8:
        _check8(m, L, R, r, D, agg, cost, ref, tag)
    _check16(m, L, R, r, D, agg, cost, ref, SUBPIX_COMBOS, tag)


@pytest.mark.parametrize("idx", WIDE_IDX, ids=lambda i: "x".join(map(str, VARIANT_CASES[i][0])))
def test_wide_census_volume(wide_matcher, idx):
    """The Hamming volume itself at the widths that leave one row (or exactly two) per block: the host call, and the
    device call on frames whose rows are strided."""
    import torch
    (W, H, D, r), _, _ = VARIANT_CASES[idx]
    L, R, _ = _case(idx)
    ham = census_ref.hamming_volume(L, R, D)
    assert np.array_equal(wide_matcher.census_volume(L, R, D), ham)
    pitch = W + 13
    Lp = torch.zeros((H, pitch), dtype=torch.uint8, device="cuda")
    Rp = torch.full((H, pitch), 255, dtype=torch.uint8, device="cuda")
    Lp[:, :W] = torch.from_numpy(L.copy()).cuda()
    Rp[:, :W] = torch.from_numpy(R.copy()).cuda()
    vol = wide_matcher.census_volume_device(Lp[:, :W], Rp[:, :W], D)
    torch.cuda.synchronize()
    assert np.array_equal(vol.cpu().numpy(), ham)


# ---- 2. the 16-bit bound ----
@pytest.mark.parametrize("r", BOUND_RADII)
@pytest.mark.parametrize("kind", ["plain", "tied"])
def test_path_costs_at_65535(matcher, kind, r):
    """SGM on the AD cost with the largest P2 that sgm_check admits, on the pairs whose reference path costs reach
    65535 exactly at both radii (test_volume_variants_model.test_bound_input_reaches_65535): the 8-bit maps, and the
    sub-pixel maps, which take the u32 sums up to 4 * 65535 through the parabola's numerator and the uniqueness
    products.  'plain' is the 0 / 255 pair with an inverted half; 'tied' puts the 65535 entries where one less would
    change a map (test_saturating_store_fault_changes_the_tied_bound_input)."""
    W, H, D = BOUND_SHAPE
    L, R, ref = _bound(kind, r, "ad")
    matcher.set_sgm_penalties(0, bound_p2(r, "ad"))
    try:
        _check8(matcher, L, R, r, D, "sgm", "ad", ref, f"bound {kind} r={r} sgm+ad")
        _check16(matcher, L, R, r, D, "sgm", "ad", ref, SUBPIX_COMBOS, f"bound {kind} r={r} sgm+ad")
    finally:
        matcher.set_sgm_penalties()


@pytest.mark.parametrize("r", BOUND_RADII)
def test_census_path_costs_past_32767(matcher, r):
    """The same pair with the census cost and its largest P2, 65535 - 62 win^2.  The reference's largest path cost
    is 57441 at r = 7 and 17309 at r = 2 (test_volume_variants_model.CENSUS_BOUND_TOP): r = 7 is past 32767 and
    guards the sign of the 16-bit store, r = 2 runs the admitted corner of P2."""
    W, H, D = BOUND_SHAPE
    L, R, ref = _bound("plain", r, "census")
    matcher.set_sgm_penalties(0, bound_p2(r, "census"))
    try:
        _check8(matcher, L, R, r, D, "sgm", "census", ref, f"bound r={r} sgm+census")
        _check16(matcher, L, R, r, D, "sgm", "census", ref, SUBPIX_COMBOS, f"bound r={r} sgm+census")
    finally:
        matcher.set_sgm_penalties()


# ---- 3. seeded fuzz ----
@pytest.mark.parametrize("seed", range(FUZZ_SEEDS))
def test_fuzz(matcher, seed):
    W, H, D, r, L, R, lr, u = fuzz_case(seed)
    ref = Reference(_oracle(), L, R, r, D)
    for agg, cost in PATHS16:
        tag = f"(seed, W, H, D, r, agg, cost) = {(seed, W, H, D, r, agg, cost)}"
        if (agg, cost) in PATHS8:
            _check8(matcher, L, R, r, D, agg, cost, ref, tag)
        _check16(matcher, L, R, r, D, agg, cost, ref, [(u, lr)], tag)


# ---- 4. non-dense device calls of the 8-bit maps ----
def _match_device_strided(m, sm_mod, Lt, Rt, r, D, out, agg, cost, lr):
    """sm_match_device with the tensors' own row and frame strides (BlockMatcher.match_device takes dense tensors)."""
    from gpu_stereo_matching_amd import _capi
    B, H, W = Lt.shape
    assert Lt.stride() == Rt.stride() and Lt.stride(2) == 1 and out.stride(2) == 1 and out.shape == Lt.shape
    _capi.check(m._lib.sm_match_device(m._h, Lt.data_ptr(), Rt.data_ptr(), W, H, Lt.stride(1), B, Lt.stride(0), r, D,
                                       sm_mod._flags(agg, lr, False, cost), out.data_ptr(), out.stride(1),
                                       out.stride(0), m._stream_ptr(None)))


@pytest.mark.parametrize("lr", [False, True])
@pytest.mark.parametrize("agg,cost", PATHS8)
def test_device_pitch_and_strided_batch(matcher, sm_mod, agg, cost, lr):
    """Frames with pitch > width and rows between them, a batch of 2 whose frames and maps are not dense."""
    import torch
    W, H, D, r, B = 67, 9, 16, 2, 2
    SENT = 0xA5   # no disparity of D = 16
    pairs = [fuzz_pair(np.random.default_rng(900 + b), W, H) for b in range(B)]
    big_l = torch.zeros((B, H + 3, W + 13), dtype=torch.uint8, device="cuda")
    big_r = torch.full((B, H + 3, W + 13), 255, dtype=torch.uint8, device="cuda")
    for b in range(B):
        big_l[b, :H, :W] = torch.from_numpy(pairs[b][0]).cuda()
        big_r[b, :H, :W] = torch.from_numpy(pairs[b][1]).cuda()
    Lt, Rt = big_l[:, :H, :W], big_r[:, :H, :W]
    big_o = torch.full((B, H + 2, W + 5), SENT, dtype=torch.uint8, device="cuda")
    out = big_o[:, :H, :W]
    _match_device_strided(matcher, sm_mod, Lt, Rt, r, D, out, agg, cost, lr)
    single = matcher.match_device(Lt[1].contiguous(), Rt[1].contiguous(), r, D, agg=agg, cost=cost, lr_check=lr)
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    for b in range(B):
        want = Reference(_oracle(), pairs[b][0], pairs[b][1], r, D).maps(agg, cost)
        assert np.array_equal(got[b], want[2] if lr else want[0]), f"frame {b}"
    assert np.array_equal(single.cpu().numpy(), got[1])
    pad = big_o.clone()
    pad[:, :H, :W] = SENT
    assert bool((pad == SENT).all())   # nothing written outside the maps
