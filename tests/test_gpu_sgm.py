"""GPU semi-global matching (SM_AGG_SGM) against the numpy restatement of its contract (tests/sgm_ref.py).

Integer arithmetic end to end, so every comparison is bit-exact: the left map, the right-view map, the
LR-checked map and the mask.
"""
import functools

import numpy as np
import pytest

import sgm_ref

pytestmark = pytest.mark.gpu

CASES = [   # W, H, D, r
    (67, 35, 16, 2),    # W and H not tile multiples
    (130, 9, 70, 1),    # D crosses one wave
    (40, 33, 64, 0),    # W < D: validity shrinks along both horizontal directions
    (96, 5, 256, 3),    # full D range
    (64, 1, 8, 0),      # single row
    (9, 40, 5, 7),      # narrow frame, widest window
    (33, 17, 1, 2),     # D = 1: the map is all zero
]


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
def _ref(W, H, D, r, p1=0, p2=0, median=False, seed=0):
    """(left, right, checked, mask) of the reference, computed once per case and shared."""
    from oracle import oracle as O
    import gpu_stereo_matching_amd as sm
    L, R = _pair(W, H, D, seed)
    out = sgm_ref.sgm_lr(O, L, R, r, D, *sm.sgm_penalties(r, p1, p2), median=median)
    for a in out:
        a.setflags(write=False)
    return out


@pytest.mark.parametrize("lr", [False, True])
@pytest.mark.parametrize("W,H,D,r", CASES)
def test_synthetic(matcher, oracle, W, H, D, r, lr):
    L, R = _pair(W, H, D)
    dl, dr, checked, mask = _ref(W, H, D, r)
    if D == 1:
        assert not dl.any()
    if lr:
        c, rr, mm = matcher.match_lr(L, R, r, D, agg="sgm")
        assert np.array_equal(rr, dr) and np.array_equal(c, checked) and np.array_equal(mm, mask)
        assert np.array_equal(matcher.match(L, R, r, D, agg="sgm", lr_check=True), checked)
    else:
        assert np.array_equal(matcher.match(L, R, r, D, agg="sgm"), dl)


@pytest.mark.parametrize("p1,p2", [(0, 0), (0, 800), (200, 200), (0, 65535 - 255 * 25)])
def test_penalty_corners(matcher, oracle, p1, p2):
    """Parameter value 0 is the auto penalty (8 win^2 / 32 win^2), as the reference side resolves it too; the
    last corner is the largest P2 the 16-bit bound allows at r = 2."""
    W, H, D, r = 67, 35, 16, 2
    L, R = _pair(W, H, D)
    dl, dr, checked, mask = _ref(W, H, D, r, p1, p2)
    matcher.set_sgm_penalties(p1, p2)
    try:
        c, rr, mm = matcher.match_lr(L, R, r, D, agg="sgm")
    finally:
        matcher.set_sgm_penalties()
    assert np.array_equal(rr, dr) and np.array_equal(c, checked) and np.array_equal(mm, mask)


def test_penalties_are_checked_by_the_call(matcher, sm_mod):
    W, H, D = 67, 35, 16
    L, R = _pair(W, H, D)
    matcher.set_sgm_penalties(900, 800)
    try:
        with pytest.raises(sm_mod.SMError, match="P1"):
            matcher.match(L, R, 2, D, agg="sgm")
    finally:
        matcher.set_sgm_penalties()
    with pytest.raises(sm_mod.SMError, match="radius"):
        matcher.match(L, R, 8, D, agg="sgm")
    out = np.empty_like(L)   # the d-slice rehearsal names its reason (the Python wrapper refuses the name earlier)
    rc = matcher._lib.sm_dslice_rehearse_u8(matcher._h, L.ctypes.data, R.ctypes.data, W, H, W, 2, D, sm_mod.SM_AGG_SGM, 2,
                                            out.ctypes.data, W)
    assert rc == 1 and b"d-slice" in matcher._lib.sm_last_error_string()


@pytest.mark.parametrize("lr", [False, True])
def test_median(matcher, oracle, lr):
    W, H, D, r = 67, 35, 16, 2
    L, R = _pair(W, H, D)
    dl, dr, checked, mask = _ref(W, H, D, r, median=True)
    if lr:
        c, rr, mm = matcher.match_lr(L, R, r, D, agg="sgm", median=True)
        assert np.array_equal(rr, dr) and np.array_equal(c, checked) and np.array_equal(mm, mask)
    else:
        assert np.array_equal(matcher.match(L, R, r, D, agg="sgm", median=True), dl)


def test_device_batch_equals_single_frames(matcher, oracle):
    import torch
    W, H, D, r, B = 67, 35, 16, 2, 3
    pairs = [_pair(W, H, D, seed=900 + b) for b in range(B)]
    Lt = torch.from_numpy(np.stack([p[0] for p in pairs])).cuda()
    Rt = torch.from_numpy(np.stack([p[1] for p in pairs])).cuda()
    for lr in (False, True):
        out = matcher.match_device(Lt, Rt, r, D, agg="sgm", lr_check=lr)
        singles = [matcher.match_device(Lt[b], Rt[b], r, D, agg="sgm", lr_check=lr) for b in range(B)]
        torch.cuda.synchronize()
        for b in range(B):
            assert np.array_equal(out[b].cpu().numpy(), singles[b].cpu().numpy())
            want = _ref(W, H, D, r, seed=900 + b)
            assert np.array_equal(out[b].cpu().numpy(), want[2] if lr else want[0])


def test_books_lr(matcher, oracle, gray):
    L, R = gray["Books/view1"], gray["Books/view5"]
    r, D = 2, 80
    dl, dr, checked, mask = sgm_ref.sgm_lr(oracle, L, R, r, D, *sgm_ref.auto_penalties(r))
    assert np.array_equal(matcher.match(L, R, r, D, agg="sgm"), dl)
    c, rr, mm = matcher.match_lr(L, R, r, D, agg="sgm")
    assert np.array_equal(rr, dr) and np.array_equal(c, checked) and np.array_equal(mm, mask)


def test_multi_tile_640x360(matcher, oracle):
    """10 column tiles in both scan directions, 360 row workgroups, two registers per lane (D = 128)."""
    W, H, D, r = 640, 360, 128, 2
    L, R = _pair(W, H, D)
    dl, dr, checked, mask = _ref(W, H, D, r)
    c, rr, mm = matcher.match_lr(L, R, r, D, agg="sgm")
    assert np.array_equal(rr, dr) and np.array_equal(c, checked) and np.array_equal(mm, mask)
    assert np.array_equal(matcher.match(L, R, r, D, agg="sgm"), dl)


def test_bgr_and_group_batch(matcher, sm_mod, oracle):
    """sm_block_match_bgr_u8 and sm_group_block_match_batch_u8 pass the flag through."""
    W, H, D, r = 67, 35, 16, 2
    L, R = _pair(W, H, D)
    dl = _ref(W, H, D, r)[0]
    bgr = lambda g: np.repeat(g[:, :, None], 3, axis=2)   # noqa: E731  (gray of an equal-channel BGR frame is itself)
    assert np.array_equal(sm_mod.bgr_to_gray(bgr(L)), L)
    assert np.array_equal(matcher.match_bgr(bgr(L), bgr(R), r, D, agg="sgm"), dl)
    with sm_mod.BlockMatcherGroup([0, 0], W, H, D) as g:
        outs = g.match_batch([L, L, L], [R, R, R], r, D, agg="sgm")
        assert all(np.array_equal(o, dl) for o in outs)
        with pytest.raises(sm_mod.SMError, match="whole frames"):
            g.match(L, R, r, D, agg="sgm")
