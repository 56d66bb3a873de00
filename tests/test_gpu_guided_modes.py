"""Every radius of the guided pass through every mode of its one launcher (csrc/bm_guided.h: GuidedPass): the map,
the map with the fused right view, a slice's keys, and a slice's keys with the right view's keys; then the frame
strides and per-frame partials of a batch.

One 75 x 40 frame with D = 40: 2 to 3 tiles wide and 2 tiles high at every radius, across the kernel's
32-disparity band chunk, the right edge cutting the valid range d <= W - x.  The contracts are those of
test_gpu_guided.py and test_gpu_dslice_lr.py (tie-aware against the fp64 oracle, guided_check.py), with no floor on
the share of exact right-view matches, which has not been measured on a frame this small."""
import functools

import numpy as np
import pytest

from guided_check import TOL, check_guided_lr, guided_reference, tie_aware_check

pytestmark = pytest.mark.gpu
EPS = 1e-4 * 255 * 255
W, H, D = 75, 40, 40
CUTS = [0, 13, 40]   # an odd d_lo, and a slice across the band chunk
NONE = 0x7FFFFFFF
RADII = list(range(8))


@pytest.fixture(scope="module")
def matcher():
    import gpu_stereo_matching_amd as sm
    m = sm.BlockMatcher(0, 128, 64, 256)
    m.set_guided_eps(EPS)
    yield m
    m.close()


@functools.lru_cache(maxsize=None)
def _frame(seed=751):
    from oracle import oracle as O
    return O.synth_pair(seed, W, H, D)


@functools.lru_cache(maxsize=None)
def _reference(r):
    from oracle import oracle as O
    L, R = _frame()
    return guided_reference(O, L, R, r, D, EPS)


def _check_left_slices(parts):
    """test_guided_slice_keys_ragged's contract: every key names a d of its slice or is INT32_MAX, it is empty
    exactly where the slice starts past the valid range; returns the signed MIN, which _finalised_ok judges."""
    xs = np.arange(W)[None, :]
    for (a, b), pk in zip(zip(CUTS[:-1], CUTS[1:]), parts):
        empty = pk == NONE
        d = pk & 0xFF
        assert ((d >= a) & (d < b) & (d <= W - xs))[~empty].all(), (a, b)
        assert (empty == (a > W - xs)).all(), (a, b)
    return np.minimum.reduce(parts)


def _finalised_ok(matcher, keys, ref):
    import torch
    got = matcher.guided_keys_to_disp_device(torch.from_numpy(keys).cuda())
    torch.cuda.synchronize()
    ok, _ = tie_aware_check(got.cpu().numpy(), ref["q"], ref, D, W)
    return ok


@pytest.mark.parametrize("r", RADII)
def test_map_and_map_lr(matcher, oracle, r):
    L, R = _frame()
    check_guided_lr(matcher, oracle, L, R, r, D, EPS, min_exact=0.0)


@pytest.mark.parametrize("r", RADII)
def test_slice_keys(matcher, r):
    import torch
    L, R = _frame()
    ref = _reference(r)
    Lt, Rt = torch.from_numpy(L).cuda(), torch.from_numpy(R).cuda()
    parts = [matcher.guided_slice_keys_device(Lt, Rt, r, a, b) for a, b in zip(CUTS[:-1], CUTS[1:])]
    torch.cuda.synchronize()
    k = _check_left_slices([p.cpu().numpy() for p in parts])
    ok = _finalised_ok(matcher, k, ref)
    assert ok.all(), f"{int((~ok).sum())} pixels outside the tie-aware tolerance"


@pytest.mark.parametrize("r", RADII)
def test_slice_lr_keys(matcher, r):
    import torch
    L, R = _frame()
    ref = _reference(r)
    Lt, Rt = torch.from_numpy(L).cuda(), torch.from_numpy(R).cuda()
    parts = [matcher.slice_keys_lr_device(Lt, Rt, r, a, b, agg="guided") for a, b in zip(CUTS[:-1], CUTS[1:])]
    torch.cuda.synchronize()
    k = _check_left_slices([lk.cpu().numpy() for lk, _ in parts])
    ok = _finalised_ok(matcher, k, ref)
    assert ok.all(), f"left: {int((~ok).sum())} pixels outside the tie-aware tolerance"
    # the right view's keys: a d of the slice with u + d < W or INT32_MAX, empty exactly where none exists, and
    # the signed MIN's d field is the right map (test_guided_slice_lr_keys' rule)
    us = np.arange(W)[None, :]
    rparts = [rk.cpu().numpy() for _, rk in parts]
    for (a, b), pk in zip(zip(CUTS[:-1], CUTS[1:]), rparts):
        empty = pk == NONE
        d = pk & 0xFF
        assert ((d >= a) & (d < b) & (us + d < W))[~empty].all(), (a, b)
        assert (empty == (us + a >= W)).all(), (a, b)
    right = (np.minimum.reduce(rparts) & 0xFF).astype(np.int64)
    ys, us = np.mgrid[0:H, 0:W]
    ok_r = (right == ref["rdisp"]) | (ref["cr"][right, ys, us] <= ref["best_r"] + TOL)
    assert ok_r.all(), f"right: {int((~ok_r).sum())} pixels outside the tie-aware tolerance"


def test_batch_of_two_frames(matcher):
    """Frame strides and per-frame right-key partials: a batch equals its frames' single calls bit for bit."""
    import torch
    r = 5
    pairs = [_frame(), _frame(752)]
    assert not np.array_equal(pairs[0][0], pairs[1][0])
    Lt = torch.from_numpy(np.stack([p[0] for p in pairs])).cuda()
    Rt = torch.from_numpy(np.stack([p[1] for p in pairs])).cuda()
    both = matcher.match_device(Lt, Rt, r, D, agg="guided", lr_check=True)
    singles = [matcher.match_device(Lt[i], Rt[i], r, D, agg="guided", lr_check=True) for i in range(2)]
    torch.cuda.synchronize()
    for i in range(2):
        assert np.array_equal(both[i].cpu().numpy(), singles[i].cpu().numpy()), i


@pytest.mark.parametrize("lr", [False, True])
def test_radius_past_the_kernels_is_an_argument_error(matcher, lr):
    """Rejected before any workspace is taken or kernel launched, in the slice calls' words."""
    import gpu_stereo_matching_amd as sm
    L, R = _frame()
    with pytest.raises(sm.SMError, match=r"guided aggregation: radius 8 > 7") as e:
        matcher.match(L, R, 8, D, agg="guided", lr_check=lr)
    assert e.value.code == sm._capi.SM_ERR_INVALID_ARG
