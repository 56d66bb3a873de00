"""GPU census cost (SM_COST_CENSUS) against the numpy restatement of its contract (tests/census_ref.py).

Integer arithmetic end to end, so every comparison is bit-exact: the census words, the Hamming volume, the left
map, the right-view map, the LR-checked map and the mask, under box and SGM aggregation.
"""
import functools

import numpy as np
import pytest

import census_ref
import sgm_ref
from test_gpu_sgm import CASES as SGM_CASES

pytestmark = pytest.mark.gpu

VOLUME_CASES = [   # W, H, D
    (67, 35, 16),    # W and H not tile multiples
    (130, 9, 70),    # three 64-column census tiles, D not a multiple of the unrolled 16
    (40, 33, 64),    # W < D: whole planes of zeros
    (96, 5, 256),    # full D range, W % 16 == 0: the 16-B stores
    (5, 3, 4),       # a frame inside the 9 x 7 window
    (9, 40, 5),      # narrow frame
    (33, 17, 1),     # D = 1
    (640, 2, 100),   # a thread walks a whole run of 16 disparities and a shorter one after it; 16-B stores
    (630, 2, 100),   # the same with the scalar stores
]
CASES = SGM_CASES + [(5, 3, 4, 0)]   # W, H, D, r
AGGS = ["box", "sgm"]


@pytest.fixture(scope="module")
def sm_mod():
    import gpu_stereo_matching_amd as sm
    return sm


@pytest.fixture(scope="module")
def matcher(sm_mod):
    m = sm_mod.BlockMatcher(0, 640, 370, 256)
    yield m
    m.close()


@functools.lru_cache(maxsize=None)
def _pair(W, H, D, seed=0):
    """oracle.synth_pair with +-4 noise on the right image, so that costs are not degenerate."""
    from oracle import oracle as O
    seed = seed or (W * 131 + H * 17 + D)
    L, R = O.synth_pair(seed, W, H, D)
    noise = np.random.default_rng(seed).integers(-4, 5, R.shape)
    return L, np.clip(R.astype(np.int64) + noise, 0, 255).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def _ref(W, H, D, r, agg, p1=0, p2=0, median=False, seed=0):
    """(left, right, checked, mask) of the reference, computed once per case and shared."""
    from oracle import oracle as O
    L, R = _pair(W, H, D, seed)
    out = census_ref.census_lr(O, L, R, r, D, agg, p1, p2, median=median)
    for a in out:
        a.setflags(write=False)
    return out


def _check_lr(matcher, L, R, r, D, agg, want, **kw):
    dl, dr, checked, mask = want
    c, rr, mm = matcher.match_lr(L, R, r, D, agg=agg, cost="census", **kw)
    assert np.array_equal(rr, dr) and np.array_equal(c, checked) and np.array_equal(mm, mask)


@pytest.mark.parametrize("W,H,D", VOLUME_CASES)
def test_census_words_and_hamming_volume(matcher, oracle, W, H, D):
    import torch
    L, R = _pair(W, H, D)
    cl, cr = census_ref.census(L), census_ref.census(R)
    ham = census_ref.hamming_volume(L, R, D)
    # host calls
    assert np.array_equal(matcher.census(L), cl) and np.array_equal(matcher.census(R), cr)
    assert np.array_equal(matcher.census_volume(L, R, D), ham)
    # device calls on frames whose rows are strided (pitch > width)
    pitch = W + 13
    Lp = torch.zeros((H, pitch), dtype=torch.uint8, device="cuda")
    Rp = torch.full((H, pitch), 255, dtype=torch.uint8, device="cuda")
    Lp[:, :W] = torch.from_numpy(L).cuda()
    Rp[:, :W] = torch.from_numpy(R).cuda()
    got = matcher.census_device(Lp[:, :W])
    vol = matcher.census_volume_device(Lp[:, :W], Rp[:, :W], D)
    torch.cuda.synchronize()
    assert np.array_equal(got.cpu().numpy().view(np.uint64), cl)
    assert np.array_equal(vol.cpu().numpy(), ham)


@pytest.mark.parametrize("lr", [False, True])
@pytest.mark.parametrize("agg", AGGS)
@pytest.mark.parametrize("W,H,D,r", CASES)
def test_synthetic(matcher, oracle, W, H, D, r, agg, lr):
    L, R = _pair(W, H, D)
    want = _ref(W, H, D, r, agg)
    if D == 1:
        assert not want[0].any()
    if lr:
        _check_lr(matcher, L, R, r, D, agg, want)
        assert np.array_equal(matcher.match(L, R, r, D, agg=agg, lr_check=True, cost="census"), want[2])
    else:
        assert np.array_equal(matcher.match(L, R, r, D, agg=agg, cost="census"), want[0])


@pytest.mark.parametrize("p1,p2", [(0, 0), (0, 3000), (250, 250), (0, 65535 - 62 * 25)])
def test_penalty_corners(matcher, oracle, p1, p2):
    """Parameter value 0 is the auto penalty (10 win^2 / 120 win^2 with the census cost), as the reference side
    resolves it too; the last corner is the largest P2 the 16-bit bound allows at r = 2."""
    W, H, D, r = 67, 35, 16, 2
    L, R = _pair(W, H, D)
    want = _ref(W, H, D, r, "sgm", p1, p2)
    matcher.set_sgm_penalties(p1, p2)
    try:
        _check_lr(matcher, L, R, r, D, "sgm", want)
    finally:
        matcher.set_sgm_penalties()


def test_arguments_are_checked_by_the_call(matcher, sm_mod):
    W, H, D = 67, 35, 16
    L, R = _pair(W, H, D)
    matcher.set_sgm_penalties(0, 65536 - 62 * 25)
    try:
        with pytest.raises(sm_mod.SMError, match="65535"):
            matcher.match(L, R, 2, D, agg="sgm", cost="census")
        matcher.match(L, R, 2, D, agg="box", cost="census")   # the penalties are SGM's alone
    finally:
        matcher.set_sgm_penalties()
    for agg in AGGS:
        with pytest.raises(sm_mod.SMError, match="radius"):
            matcher.match(L, R, 8, D, agg=agg, cost="census")
    for agg in ("guided", "box-staged"):
        with pytest.raises(sm_mod.SMError, match="does not combine"):
            matcher.match(L, R, 2, D, agg=agg, cost="census")
    out = np.empty_like(L)   # the d-slice rehearsal names its reason
    rc = matcher._lib.sm_dslice_rehearse_u8(matcher._h, L.ctypes.data, R.ctypes.data, W, H, W, 2, D,
                                            sm_mod.SM_COST_CENSUS, 2, out.ctypes.data, W)
    assert rc == 1 and b"d-slice" in matcher._lib.sm_last_error_string()
    assert b"SM_COST_CENSUS" in matcher._lib.sm_last_error_string()


@pytest.mark.parametrize("lr", [False, True])
@pytest.mark.parametrize("agg", AGGS)
def test_median(matcher, oracle, agg, lr):
    W, H, D, r = 67, 35, 16, 2
    L, R = _pair(W, H, D)
    want = _ref(W, H, D, r, agg, median=True)
    if lr:
        _check_lr(matcher, L, R, r, D, agg, want, median=True)
    else:
        assert np.array_equal(matcher.match(L, R, r, D, agg=agg, median=True, cost="census"), want[0])


@pytest.mark.parametrize("agg", AGGS)
def test_device_batch_equals_single_frames(matcher, oracle, agg):
    import torch
    W, H, D, r, B = 67, 35, 16, 2, 3
    pairs = [_pair(W, H, D, seed=900 + b) for b in range(B)]
    Lt = torch.from_numpy(np.stack([p[0] for p in pairs])).cuda()
    Rt = torch.from_numpy(np.stack([p[1] for p in pairs])).cuda()
    for lr in (False, True):
        out = matcher.match_device(Lt, Rt, r, D, agg=agg, lr_check=lr, cost="census")
        singles = [matcher.match_device(Lt[b], Rt[b], r, D, agg=agg, lr_check=lr, cost="census") for b in range(B)]
        torch.cuda.synchronize()
        for b in range(B):
            assert np.array_equal(out[b].cpu().numpy(), singles[b].cpu().numpy())
            want = _ref(W, H, D, r, agg, seed=900 + b)
            assert np.array_equal(out[b].cpu().numpy(), want[2] if lr else want[0])


@pytest.mark.parametrize("agg", AGGS)
def test_books_lr(matcher, oracle, gray, agg):
    L, R = gray["Books/view1"], gray["Books/view5"]
    r, D = 2, 80
    want = census_ref.census_lr(oracle, L, R, r, D, agg)
    assert np.array_equal(matcher.match(L, R, r, D, agg=agg, cost="census"), want[0])
    _check_lr(matcher, L, R, r, D, agg, want)


@pytest.mark.parametrize("W,H", [(640, 360), (637, 33)])
@pytest.mark.parametrize("agg", AGGS)
def test_multi_tile(matcher, oracle, agg, W, H):
    """640 x 360: many tiles, two registers per lane in the horizontal scan (D = 128), W % 16 == 0 (vector loads and
    stores); 637 x 33: the scalar variants."""
    D, r = 128, 2
    L, R = _pair(W, H, D)
    want = _ref(W, H, D, r, agg)
    _check_lr(matcher, L, R, r, D, agg, want)
    assert np.array_equal(matcher.match(L, R, r, D, agg=agg, cost="census"), want[0])


@pytest.mark.parametrize("agg", AGGS)
def test_bgr_and_group_batch(matcher, sm_mod, oracle, agg):
    """sm_block_match_bgr_u8 and sm_group_block_match_batch_u8 pass the flag through; the row bands refuse it."""
    W, H, D, r = 67, 35, 16, 2
    L, R = _pair(W, H, D)
    dl = _ref(W, H, D, r, agg)[0]
    bgr = lambda g: np.repeat(g[:, :, None], 3, axis=2)   # noqa: E731  (gray of an equal-channel BGR frame is itself)
    assert np.array_equal(sm_mod.bgr_to_gray(bgr(L)), L)
    assert np.array_equal(matcher.match_bgr(bgr(L), bgr(R), r, D, agg=agg, cost="census"), dl)
    with sm_mod.BlockMatcherGroup([0, 0], W, H, D) as g:
        outs = g.match_batch([L, L, L], [R, R, R], r, D, agg=agg, cost="census")
        assert all(np.array_equal(o, dl) for o in outs)
        with pytest.raises(sm_mod.SMError, match="whole frames" if agg == "sgm" else "replicated border"):
            g.match(L, R, r, D, agg=agg, cost="census")


def test_ad_paths_after_census_on_the_same_handle(matcher, oracle):
    """The volume workspace is shared: an AD SGM call made after census calls still equals sgm_ref, and
    cost='ad' is the call without the keyword."""
    W, H, D, r = 67, 35, 16, 2
    L, R = _pair(W, H, D)
    for agg in AGGS:
        matcher.match_lr(L, R, r, D, agg=agg, cost="census")
    dl, dr, checked, mask = sgm_ref.sgm_lr(oracle, L, R, r, D, *sgm_ref.auto_penalties(r))
    c, rr, mm = matcher.match_lr(L, R, r, D, agg="sgm")
    assert np.array_equal(rr, dr) and np.array_equal(c, checked) and np.array_equal(mm, mask)
    assert np.array_equal(matcher.match(L, R, r, D, agg="sgm"), dl)
    for agg in ("box", "sgm", "guided"):
        for lr in (False, True):
            assert np.array_equal(matcher.match(L, R, r, D, agg=agg, lr_check=lr, cost="ad"),
                                  matcher.match(L, R, r, D, agg=agg, lr_check=lr))
    assert np.array_equal(matcher.match(L, R, r, D), oracle.get_disp(L, R, r, D))
