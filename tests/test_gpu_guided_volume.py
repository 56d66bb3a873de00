"""The guided cost volume in one pass (sm_guided_volume_device) and SM_AGG_GUIDED in the sub-pixel calls.

Volume: bit for bit the route the library already had and tests/test_gpu_guided_cost.py validates against fp64, one
one-disparity slice per d: vol[d] == guided_slice_keys_device(d, d + 1) >> 8 where the pair exists (d <= W - x),
INT32_MAX elsewhere.  Shapes: guided_volume_shapes.volume_shapes() (tests/test_guided_volume_model.py shows that they
reach every compiled path of the kernel), a pitch > W and frames cut out of a larger tensor.

Sub-pixel maps: the maps, the right map and the mask of match_subpix(agg="guided") equal subpix_ref's integer rule on
the volume read back from the GPU, V = vol + 2^23 with 2^24 - 1 where the pair does not exist (include/sm_hip.h),
right pairs u + d < W, invalid_from (50 + 512) 2^14; then median16_ref / speckle_ref / fill_ref as for the other
aggregations.  No tolerance anywhere except the tie-aware comparison with the 8-bit guided map, whose rule is in its
docstring.
"""
import functools

import numpy as np
import pytest

import fill_ref
import guided_cost_ref as G
import guided_volume_shapes as S
import median16_ref
import speckle_ref
import subpix_ref

pytestmark = pytest.mark.gpu

BIAS = 512 << 14
NONE = (1 << 24) - 1
INVALID_FROM = (50 + 512) << 14
SHAPES = S.volume_shapes()


@pytest.fixture(scope="module")
def torch():
    import torch as t
    assert t.cuda.is_available()
    return t


@pytest.fixture(scope="module")
def sm_mod():
    import gpu_stereo_matching_amd as sm
    return sm


@pytest.fixture(scope="module")
def matcher(sm_mod):
    m = sm_mod.BlockMatcher(0, 512, 256, 256)
    m.set_guided_eps(G.EPS_DEFAULT)
    m.set_guided_subpix(True)
    yield m
    m.close()


_TEX = {}


def _texture(gray, oracle, W, H, name):
    if (W, H) not in _TEX:
        _TEX[W, H] = G.texture_classes(gray, oracle, W, H)
    return _TEX[W, H][name]


def _exists(D, H, W):
    return np.broadcast_to((np.arange(D)[:, None] <= W - np.arange(W)[None, :])[:, None, :], (D, H, W))


def _slice_route(torch, matcher, Lt, Rt, r, D):
    """The parent's only route to the volume: one one-disparity slice per d (contiguous frames).  A slice past
    min(W, 255) has no valid pixel and is not launched."""
    H, W = Lt.shape
    want = np.full((D, H, W), G.INT32_MAX, np.int32)
    ds = [d for d in range(D) if d <= min(W, 255)]
    keys = torch.stack([matcher.guided_slice_keys_device(Lt, Rt, r, d, d + 1) for d in ds]).cpu().numpy()
    empty = keys == G.INT32_MAX
    assert np.array_equal(~empty, _exists(D, H, W)[ds]), "the slice route's empty keys are not d > W - x"
    want[ds] = np.where(empty, G.INT32_MAX, keys >> 8)
    return want


def _compare(got, want, what):
    D, H, W = want.shape
    ex = _exists(D, H, W)
    assert (got[~ex] == G.INT32_MAX).all(), f"{what}: an entry with d > W - x is not INT32_MAX"
    bad = got != want
    assert not bad.any(), (f"{what}: {int(bad.sum())} of {bad.size} costs differ from the slice route, first at "
                           f"(d, y, x) = {tuple(int(v[0]) for v in np.nonzero(bad))}, largest difference "
                           f"{int(np.abs(got.astype(np.int64) - want)[bad & ex].max(initial=0))}")


@pytest.mark.parametrize("r,W,H,D,name", SHAPES, ids=[f"r{r}-{W}x{H}-D{D}" for r, W, H, D, _ in SHAPES])
def test_volume_equals_the_slice_route(matcher, oracle, gray, torch, r, W, H, D, name):
    L, R = _texture(gray, oracle, W, H, name)
    Lt, Rt = torch.from_numpy(L).cuda(), torch.from_numpy(R).cuda()
    got = matcher.guided_volume_device(Lt, Rt, r, D).cpu().numpy()
    _compare(got, _slice_route(torch, matcher, Lt, Rt, r, D), f"r={r} {W}x{H} D={D} {name}")


def test_volume_pitch_window_host_form_and_eps(matcher, oracle, gray, torch):
    """Rows with a pitch > W, a frame cut out of a larger batch tensor, the host form, and another eps."""
    r, W, H, D = 4, 101, 37, 35
    L, R = _texture(gray, oracle, W, H, "synth")
    Lt, Rt = torch.from_numpy(L).cuda(), torch.from_numpy(R).cuda()
    want = _slice_route(torch, matcher, Lt, Rt, r, D)
    pad = torch.full((2, H, W + 11), 0xEE, dtype=torch.uint8, device="cuda")
    pad[0, :, 3:3 + W], pad[1, :, 3:3 + W] = Lt, Rt
    got = matcher.guided_volume_device(pad[0, :, 3:3 + W], pad[1, :, 3:3 + W], r, D).cpu().numpy()
    _compare(got, want, "pitch > W")
    big = torch.full((2, 3, H + 4, W + 10), 0x11, dtype=torch.uint8, device="cuda")
    big[0, 1, 2:2 + H, 5:5 + W], big[1, 1, 2:2 + H, 5:5 + W] = Lt, Rt
    out = torch.full((D + 2, H, W), -7, dtype=torch.int32, device="cuda")
    matcher.guided_volume_device(big[0, 1, 2:2 + H, 5:5 + W], big[1, 1, 2:2 + H, 5:5 + W], r, D, out_t=out[1:D + 1])
    out = out.cpu().numpy()
    _compare(out[1:D + 1], want, "a frame inside a larger tensor")
    assert (out[0] == -7).all() and (out[D + 1] == -7).all()          # nothing written around the planes
    _compare(matcher.guided_volume(L, R, r, D), want, "host form")
    matcher.set_guided_eps(5000.0)
    try:
        got = matcher.guided_volume_device(Lt, Rt, r, D).cpu().numpy()
        want2 = _slice_route(torch, matcher, Lt, Rt, r, D)
    finally:
        matcher.set_guided_eps(G.EPS_DEFAULT)
    _compare(got, want2, "eps = 5000")
    assert (want2 != want).any()


# ---- sub-pixel maps ----
PW, PH, PD = 131, 40, 32
GAP, SPECKLE = 12, 20


@functools.lru_cache(maxsize=None)
def _pair(flip=0):
    """oracle.synth_pair with +-4 noise on the right image (tests/test_gpu_fill.py's recipe), three tiles wide at
    r = 2; flip 1 / 2: the frames upside down / mirrored rows swapped, for the other frames of a batch."""
    from oracle import oracle as O
    seed = PW * 131 + PH * 17 + PD
    L, R = O.synth_pair(seed, PW, PH, PD)
    R = np.clip(R.astype(np.int64) + np.random.default_rng(seed).integers(-4, 5, R.shape), 0, 255).astype(np.uint8)
    if flip == 1:
        L, R = L[::-1].copy(), R[::-1].copy()
    if flip == 2:
        L, R = np.roll(L, 7, axis=0).copy(), np.roll(R, 7, axis=0).copy()
    L.setflags(write=False)
    R.setflags(write=False)
    return L, R


_VOL = {}


def _gpu_volume(torch, matcher, r, flip=0):
    """(vol int64 as the GPU returned it, V = the biased uint32 form of include/sm_hip.h), computed once."""
    if (r, flip) not in _VOL:
        L, R = _pair(flip)
        vol = matcher.guided_volume_device(torch.from_numpy(L).cuda(), torch.from_numpy(R).cuda(), r, PD)
        vol = vol.cpu().numpy().astype(np.int64)
        V = np.where(vol == G.INT32_MAX, NONE, vol + BIAS)
        assert V.min() >= 0 and V.max() <= NONE
        vol.setflags(write=False)
        V.setflags(write=False)
        _VOL[r, flip] = (vol, V)
    return _VOL[r, flip]


def _want(V, lr, med=0, speckle=0, gap=0):
    """(map, right map, mask) of the contract from the volume."""
    if med:
        q, qr, _ = subpix_ref.subpix(V, 0, INVALID_FROM, False, 2)
        q, qr, mask = median16_ref.subpix_median(q, qr, med, lr)
    else:
        q, qr, mask = subpix_ref.subpix(V, 0, INVALID_FROM, lr, 2)
    if speckle:
        q, mask = speckle_ref.speckle(q, speckle, 16, mask)
    if gap:
        q = fill_ref.fill(q, gap)
    return q, qr, mask


def _same(got, want, what):
    for g, w, name in zip(got, want, ("map", "right map", "mask")):
        assert np.array_equal(g, w), f"{what}: {name}, {int((g != w).sum())} of {w.size} pixels differ"


@pytest.mark.parametrize("lr", [False, True], ids=["nocheck", "lr"])
@pytest.mark.parametrize("r", [0, 2, 5, 7])
def test_subpix_maps_equal_the_rule_on_the_volume(matcher, torch, oracle, r, lr):
    L, R = _pair()
    _, V = _gpu_volume(torch, matcher, r)
    want = _want(V, lr)
    # non-vacuity, on the reference: fractional parts, pixels past the threshold, and with the check occlusions
    unchecked = subpix_ref.subpix(V, 0, INVALID_FROM, False, 2)
    assert (unchecked[0] % 16 != 0).sum() > want[0].size // 10 and (unchecked[2] == 0).any()
    assert not lr or (want[2] != unchecked[2]).sum() > 50
    _same(matcher.match_subpix(L, R, r, PD, agg="guided", lr_check=lr, return_right=True, return_mask=True), want,
          f"r={r} lr={lr}")
    assert np.array_equal(matcher.match_subpix(L, R, r, PD, agg="guided", lr_check=lr), want[0])   # no right16, no mask


@pytest.mark.parametrize("med,speckle,gap", [(1, 0, 0), (3, 0, 0), (0, SPECKLE, 0), (0, 0, GAP), (1, SPECKLE, GAP)],
                         ids=["median1", "median3", "speckle", "fill", "all"])
def test_subpix_later_steps(matcher, torch, oracle, med, speckle, gap):
    """SM_PARAM_SUBPIX_MEDIAN, the speckle filter and the row fill after the guided WTA, in the order of the other
    aggregations, with and without the check."""
    r = 2
    L, R = _pair()
    _, V = _gpu_volume(torch, matcher, r)
    plain = _want(V, True)
    matcher.set_subpix_median(med)
    matcher.set_speckle(speckle, 1)
    matcher.set_fill(gap)
    try:
        got_lr = matcher.match_subpix(L, R, r, PD, agg="guided", lr_check=True, return_right=True, return_mask=True)
        got_un = matcher.match_subpix(L, R, r, PD, agg="guided", lr_check=False, return_right=True, return_mask=True)
        got_alone = matcher.match_subpix(L, R, r, PD, agg="guided", lr_check=True)
    finally:
        matcher.set_subpix_median(0)
        matcher.set_speckle()
        matcher.set_fill(0)
    want = _want(V, True, med, speckle, gap)
    assert (want[0] != plain[0]).any(), "the step changes nothing on this case"
    _same(got_lr, want, "lr")
    _same(got_un, _want(V, False, med, speckle, gap), "no check")
    assert np.array_equal(got_alone, want[0])


def test_subpix_batch_of_three_in_a_larger_tensor(matcher, torch, oracle):
    r = 2
    frames = [_pair(f) for f in range(3)]
    big = torch.full((2, 3, PH + 3, PW + 9), 0x33, dtype=torch.uint8, device="cuda")
    for f, (L, R) in enumerate(frames):
        big[0, f, 1:1 + PH, 4:4 + PW] = torch.from_numpy(L).cuda()
        big[1, f, 1:1 + PH, 4:4 + PW] = torch.from_numpy(R).cuda()
    out = torch.zeros((3, PH + 4, PW + 10), dtype=torch.int16, device="cuda")
    win = out[:, 3:3 + PH, 5:5 + PW]
    rt = torch.empty((3, PH, PW), dtype=torch.int16, device="cuda")
    mt = torch.empty((3, PH, PW), dtype=torch.uint8, device="cuda")
    matcher.match_subpix_device(big[0, :, 1:1 + PH, 4:4 + PW], big[1, :, 1:1 + PH, 4:4 + PW], r, PD, out_t=win,
                                agg="guided", lr_check=True, right_t16=rt, mask_t=mt)
    torch.cuda.synchronize()
    got = out.cpu().numpy().view(np.uint16)
    for f in range(3):
        want = _want(_gpu_volume(torch, matcher, r, f)[1], True)
        _same((got[f, 3:3 + PH, 5:5 + PW], rt[f].cpu().numpy().view(np.uint16), mt[f].cpu().numpy()), want, f"frame {f}")
    got[:, 3:3 + PH, 5:5 + PW] = 0
    assert not got.any()                                       # nothing written around the window


@pytest.mark.parametrize("byte", [0x00, 0xFF, 0x5A])
def test_subpix_under_workspace_poison(sm_mod, matcher, torch, oracle, byte):
    """Every byte of the workspaces the call takes is filled first: the result is that of the plain handle, so no
    step reads an entry the frame's own launches did not write."""
    r = 2
    L, R = _pair()
    _, V = _gpu_volume(torch, matcher, r)
    with sm_mod.BlockMatcher(0, 512, 256, 256) as m:
        m.set_guided_eps(G.EPS_DEFAULT)
        m.set_guided_subpix(True)
        m.set_workspace_poison(byte)
        _same(m.match_subpix(L, R, r, PD, agg="guided", lr_check=True, return_right=True, return_mask=True),
              _want(V, True), f"poison {byte:#x}")
        m.set_subpix_median(1)
        _same(m.match_subpix(L, R, r, PD, agg="guided", lr_check=True, return_right=True, return_mask=True),
              _want(V, True, 1), f"poison {byte:#x}, median")
        vol = m.guided_volume(L, R, r, PD)
        assert np.array_equal(vol, _gpu_volume(torch, matcher, r)[0])


def test_refusals(sm_mod, matcher, torch):
    """Each comes before any device work, with a message that names what is refused."""
    from gpu_stereo_matching_amd import _capi
    L, R = _pair()
    Lt, Rt = torch.from_numpy(L).cuda(), torch.from_numpy(R).cuda()
    out_t = torch.full((PH, PW), 0x5A5A, dtype=torch.int16, device="cuda")
    with sm_mod.BlockMatcher(0, 512, 256, 256) as m:
        # SM_PARAM_GUIDED_SUBPIX is off by default: the flag is refused as before the volume existed
        for call in (lambda: m.match_subpix(L, R, 2, PD, agg="guided"),
                     lambda: m.match_subpix_device(Lt, Rt, 2, PD, out_t=out_t, agg="guided")):
            with pytest.raises(sm_mod.SMError, match="no cost volume.*SM_PARAM_GUIDED_SUBPIX"):
                call()
        for bad in (-1.0, 0.5, 2.0, float("nan")):
            assert m._lib.sm_set_param_f(m._h, _capi.SM_PARAM_GUIDED_SUBPIX, bad) == _capi.SM_ERR_INVALID_ARG
            assert b"SM_PARAM_GUIDED_SUBPIX" in m._lib.sm_last_error_string()
        m.set_guided_subpix(True)
        m.set_guided_subpix(False)
        with pytest.raises(sm_mod.SMError, match="no cost volume"):
            m.match_subpix(L, R, 2, PD, agg="guided")
        m.set_guided_subpix(True)
        m.set_uniqueness(10)
        for call in (lambda: m.match_subpix(L, R, 2, PD, agg="guided"),
                     lambda: m.match_subpix_device(Lt, Rt, 2, PD, out_t=out_t, agg="guided", lr_check=True)):
            with pytest.raises(sm_mod.SMError, match="SM_PARAM_UNIQUENESS.*SM_AGG_GUIDED") as e:
                call()
            assert e.value.code == _capi.SM_ERR_INVALID_ARG
        m.set_uniqueness(0)
        with pytest.raises(sm_mod.SMError, match="SM_PAIRS_IN_VIEW.*SM_AGG_GUIDED"):
            m.match_subpix_device(Lt, Rt, 2, PD, out_t=out_t, agg="guided", pairs="in-view")
        with pytest.raises(sm_mod.SMError, match="SM_COST_CENSUS.*SM_AGG_GUIDED"):
            m.match_subpix_device(Lt, Rt, 2, PD, out_t=out_t, agg="guided", cost="census")
        q = np.empty((PH, PW), np.uint16)
        for extra, name in ((sm_mod.SM_STAGED, "SM_STAGED"), (sm_mod.SM_DEVICE_CU_GRID, "SM_DEVICE_CU_GRID"),
                            (sm_mod.SM_AGG_SGM, "SM_AGG_SGM")):
            with pytest.raises(sm_mod.SMError, match=f"SM_AGG_GUIDED.*{name}|{name}.*SM_AGG_GUIDED"):
                _capi.check(m._lib.sm_block_match_subpix_u16(m._h, L.ctypes.data, R.ctypes.data, PW, PH, PW, 2, PD,
                                                             sm_mod.SM_AGG_GUIDED | extra, q.ctypes.data, None, None,
                                                             PW))
        with pytest.raises(sm_mod.SMError, match="radius"):
            m.match_subpix(L, R, 8, PD, agg="guided")
        with pytest.raises(sm_mod.SMError, match="radius"):
            m.guided_volume_device(Lt, Rt, 8, PD)
        with pytest.raises(sm_mod.SMError, match="num_disp"):
            m.guided_volume_device(Lt, Rt, 2, 257, out_t=torch.empty((257, PH, PW), dtype=torch.int32, device="cuda"))
        m.set_min_disp(3)
        with pytest.raises(sm_mod.SMError, match="SM_PARAM_MIN_DISP"):
            m.match_subpix_device(Lt, Rt, 2, PD, out_t=out_t, agg="guided")
        with pytest.raises(sm_mod.SMError, match="SM_PARAM_MIN_DISP"):
            m.guided_volume_device(Lt, Rt, 2, PD)
        m.set_min_disp(0)
        torch.cuda.synchronize()
        assert bool((out_t == 0x5A5A).all())                   # no refused call wrote its output
        m.match_subpix_device(Lt, Rt, 2, PD, out_t=out_t, agg="guided")   # and the handle is back to normal
        torch.cuda.synchronize()
        assert not bool((out_t == 0x5A5A).all())


@pytest.mark.parametrize("r", [2, 5])
def test_unchecked_map_against_the_8bit_guided_map(matcher, torch, oracle, r):
    """The 8-bit guided call decides on the fp32 q, the sub-pixel call on trunc(q 2^14): where (q16 + 8) >> 4 of the
    unchecked left map differs from the 8-bit map's d, the two volume costs at those d differ by at most 1 quantum;
    and the maps agree at every pixel whose best two volume costs differ by 2 quanta or more.  The share of differing
    pixels is printed, not capped.

    (q16 + 8) >> 4 is the map's whole disparity d0 except where q16 = 16 k + 8, which is d0 = k with delta = +8 or
    d0 = k + 1 with delta = -8.  delta = +8 needs no plateau: the parabola's vertex rounds half up, so it is +8 from
    a - c >= 30 (c - b) on, with c > b by any amount (first run: 14 such pixels at r = 2, their costs up to 14836
    quanta apart, 3 at r = 5).  The volume tells the two apart exactly: d0 is a first minimum, so V(k) <= V(k + 1)
    in the first case and V(k) > V(k + 1) in the second.  That d0 is what is compared here; elsewhere it is
    (q16 + 8) >> 4 as it stands."""
    L, R = _pair()
    vol, _ = _gpu_volume(torch, matcher, r)
    q16 = matcher.match_subpix(L, R, r, PD, agg="guided").astype(np.int64)
    d8 = matcher.match(L, R, r, PD, agg="guided").astype(np.int64)
    cost = lambda d: np.take_along_axis(vol, d[None], axis=0)[0]   # noqa: E731
    d16 = (q16 + 8) >> 4
    half = q16 % 16 == 8
    assert half.any() and (d16[half] >= 1).all()
    d16 = np.where(half & (cost(d16 - half) <= cost(d16)), d16 - 1, d16)
    differ = d16 != d8
    assert (cost(d16) != G.INT32_MAX).all() and (cost(d8) != G.INT32_MAX).all()
    gap = np.abs(cost(d16) - cost(d8))
    print(f"\nguided r={r}: {int(differ.sum())} of {differ.size} pixels ({100.0 * differ.mean():.3f} %) differ from "
          f"the 8-bit map; largest cost difference there {int(gap[differ].max(initial=0))} quanta")
    assert (gap[differ] <= 1).all(), f"{int((gap[differ] > 1).sum())} differing pixels are no near-tie"
    two = np.sort(vol, axis=0)[:2]                             # INT32_MAX where the pair does not exist
    clear = two[1] - two[0] >= 2
    assert clear.mean() > 0.5
    assert not (differ & clear).any(), f"{int((differ & clear).sum())} pixels with a clear winner differ"
