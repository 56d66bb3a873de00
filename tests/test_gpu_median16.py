"""GPU 16-bit median (sm_median_u16_*, SM_PARAM_SUBPIX_MEDIAN) against the numpy restatement of its contract
(tests/median16_ref.py).  Integer arithmetic end to end, so every comparison is bit-exact: the maps, the masks and
the elements between width and pitch.

The kernel (csrc/bm_median16.hip) gives a workgroup a 64 x 32 tile and a wave 8 rows of it; the shapes below sit on
both sides of both tile edges and include frames smaller than the window.
"""
import functools
import os

import numpy as np
import pytest

import fill_ref
import median16_ref
import pairs_ref
import speckle_ref
import subpix_ref

pytestmark = pytest.mark.gpu

RADII = [1, 2, 3]
WIDTHS = [1, 2, 3, 63, 64, 65, 129]       # tile width 64: 63, 64, 65; 129 = two tiles and one column
HEIGHTS = [1, 2, 3, 31, 32, 33, 65]       # tile height 32: 31, 32, 33; 65 = two tiles and one row
PAD = 0xFFFF                              # above every value of the maps it surrounds: read, it would raise a median


@pytest.fixture(scope="module")
def sm_mod():
    import gpu_stereo_matching_amd as sm
    return sm


@pytest.fixture(scope="module")
def matcher(sm_mod):
    m = sm_mod.BlockMatcher(0, 480, 380, 128)
    yield m
    m.close()


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int16)).cuda()


def _host(t):
    return t.cpu().numpy().view(np.uint16)


def check(matcher, img, r):
    want = median16_ref.median(img, r)
    got = matcher.median16(img, r)
    assert got.dtype == np.uint16 and got.shape == img.shape
    bad = np.argwhere(got != want)
    assert len(bad) == 0, f"r={r} {img.shape}: {len(bad)} of {img.size} pixels differ, first (y, x) = {bad[0].tolist()}"
    return got


@pytest.mark.parametrize("r", RADII)
def test_shapes_around_the_tile(matcher, r):
    """Every W x H of the lists: tile - 1, tile, tile + 1, more than one tile each way, frames inside the window."""
    rng = np.random.default_rng(r)
    for H in HEIGHTS:
        for W in WIDTHS:
            img = rng.integers(0, 65536, (H, W)).astype(np.uint16)
            img[rng.random((H, W)) < 0.2] = 0
            check(matcher, img, r)


def _values(kind, H=45, W=71):
    rng = np.random.default_rng(len(kind) * 7 + H)
    if kind == "full":
        return rng.integers(0, 65536, (H, W)).astype(np.uint16)
    if kind == "sign":          # both sides of 0x8000: a signed compare orders them the other way round
        return rng.integers(0x7FF0, 0x8010, (H, W)).astype(np.uint16)
    if kind == "bytes":         # 0x00FF / 0x0100, 0x01FF / 0x0200, ...: the low byte orders them the other way round
        k = rng.integers(0, 255, (H, W))
        return np.where(rng.random((H, W)) < 0.5, (k << 8) | 0xFF, (k + 1) << 8).astype(np.uint16)
    if kind == "top":           # 0xFFFF next to its neighbours and to 0
        return rng.choice(np.array([0, 1, 0xFFFE, 0xFFFF], np.uint16), (H, W))
    if kind == "all-top":
        return np.full((H, W), 0xFFFF, np.uint16)
    if kind == "constant":
        return np.full((H, W), 0x1234, np.uint16)
    if kind == "zero":
        return np.zeros((H, W), np.uint16)
    if kind == "two":           # ties at every rank
        return rng.choice(np.array([0x00FF, 0x0100], np.uint16), (H, W))
    if kind == "three":
        return rng.choice(np.array([0, 0x7FFF, 0x8000], np.uint16), (H, W))
    if kind == "holes":         # a disparity map that is 60 % zeros
        img = rng.integers(16, 4089, (H, W)).astype(np.uint16)
        img[rng.random((H, W)) < 0.6] = 0
        assert abs(float(np.mean(img == 0)) - 0.6) < 0.03
        return img
    raise ValueError(kind)


@pytest.mark.parametrize("r", RADII)
@pytest.mark.parametrize("kind", ["full", "sign", "bytes", "top", "all-top", "constant", "zero", "two", "three",
                                  "holes"])
def test_values(matcher, kind, r):
    img = _values(kind)
    got = check(matcher, img, r)
    if kind in ("all-top", "constant", "zero"):
        assert np.array_equal(got, img)
    if kind == "two":
        assert set(np.unique(got).tolist()) == {0x00FF, 0x0100}
    if kind == "holes":
        assert (got == 0).sum() > (img == 0).sum()      # the majority value wins: more holes than before


@pytest.mark.parametrize("r", RADII)
@pytest.mark.parametrize("W,H", [(65, 33), (3, 2), (64, 32)])
def test_pitch_and_padding(matcher, r, W, H):
    """Source and destination at pitch W + 6: the padding is neither read nor written."""
    import torch
    rng = np.random.default_rng(W + r)
    img = rng.integers(0, 0x4000, (H, W)).astype(np.uint16)
    src = np.full((H, W + 6), PAD, np.uint16)
    src[:, :W] = img
    # the padding value would change a border pixel's median if it were read in place of the replicated column
    leaked = median16_ref.median(src, r)[:, :W]
    want = median16_ref.median(img, r)
    assert (leaked != want).any()
    st = _dev(src)
    dt = _dev(np.full((H, W + 6), 0xA5A5, np.uint16))
    out = matcher.median16_device(st[:, :W], r, out_t=dt[:, :W])
    torch.cuda.synchronize()
    assert out.data_ptr() == dt.data_ptr()
    got = _host(dt)
    assert np.array_equal(got[:, :W], want)
    assert (got[:, W:] == 0xA5A5).all()                  # the sentinels come back
    assert np.array_equal(_host(st), src)                # not in place: the source stays


@pytest.mark.parametrize("r", RADII)
def test_batch_in_a_larger_tensor(matcher, r):
    """Three frames cut from the middle of a larger tensor: frame stride above pitch * H on both sides; each frame
    equals its single call; the rows between the frames and the columns around them stay."""
    import torch
    H, W, B = 33, 67, 3
    rng = np.random.default_rng(r)
    big = rng.integers(0, 65536, (B, H + 5, W + 9)).astype(np.uint16)
    bt = _dev(big)
    ot = _dev(np.full((B, H + 3, W + 4), 0x5A5A, np.uint16))
    win, owin = bt[:, 2:2 + H, 4:4 + W], ot[:, 1:1 + H, 3:3 + W]
    assert win.stride(0) > win.stride(1) * H and owin.stride(0) > owin.stride(1) * H
    matcher.median16_device(win, r, out_t=owin)
    singles = [matcher.median16_device(win[b], r) for b in range(B)]
    torch.cuda.synchronize()
    got = _host(ot)
    want = np.full((B, H + 3, W + 4), 0x5A5A, np.uint16)
    for b in range(B):
        frame = median16_ref.median(big[b, 2:2 + H, 4:4 + W], r)
        want[b, 1:1 + H, 3:3 + W] = frame
        assert np.array_equal(_host(singles[b]), frame), b
    assert np.array_equal(got, want)
    assert np.array_equal(_host(bt), big)
    # without out_t: a new dense tensor
    dense = matcher.median16_device(win, r)
    torch.cuda.synchronize()
    assert dense.is_contiguous() and np.array_equal(_host(dense), want[:, 1:1 + H, 3:3 + W])


def test_host_form_equals_device_form_and_refusals(matcher, sm_mod):
    import torch
    img = _values("full", 70, 130)
    for r in RADII:
        dev = matcher.median16_device(_dev(img), r)
        torch.cuda.synchronize()
        assert np.array_equal(matcher.median16(img, r), _host(dev))
    t = _dev(img)
    for call, what in ((lambda: matcher.median16(img, 0), "radius 0"),
                       (lambda: matcher.median16(img, 4), "radius 4"),
                       (lambda: matcher.median16_device(t, 1, out_t=t), "same map"),
                       (lambda: matcher.median16(np.zeros((400, 500), np.uint16), 1), "exceeds handle capacity")):
        with pytest.raises(sm_mod.SMError, match=what) as e:
            call()
        assert e.value.code in (sm_mod._capi.SM_ERR_INVALID_ARG, sm_mod._capi.SM_ERR_CAPACITY)
    with pytest.raises(ValueError):
        matcher.median16(img.astype(np.uint8), 1)


# ---- the matching calls ----
PW, PH, PD, PR = 96, 40, 32, 2
GAP, SPECKLE = 12, 20
PATHS = [("box", "ad"), ("sgm", "ad"), ("sgm", "census")]


@functools.lru_cache(maxsize=None)
def _pair(flip=False):
    """test_gpu_fill.py's pair: 96 x 40, D = 32, oracle.synth_pair with +-4 noise on the right image."""
    from oracle import oracle as O
    seed = PW * 131 + PH * 17 + PD
    L, R = O.synth_pair(seed, PW, PH, PD)
    R = np.clip(R.astype(np.int64) + np.random.default_rng(seed).integers(-4, 5, R.shape), 0, 255).astype(np.uint8)
    if flip:
        L, R = L[::-1].copy(), R[::-1].copy()
    L.setflags(write=False)
    R.setflags(write=False)
    return L, R


@functools.lru_cache(maxsize=None)
def _volume(agg, cost, flip=False):
    from oracle import oracle as O
    O.build()
    L, R = _pair(flip)
    return subpix_ref.volume(O, L, R, PR, PD, agg, cost)


@functools.lru_cache(maxsize=None)
def _views(agg, cost, u, flip=False):
    """Both views' unchecked 1/16-px maps (subpix_ref.view), and the LR-checked call's (q, right q, mask)."""
    V, inv, rp = _volume(agg, cost, flip)
    q, qr, _ = subpix_ref.subpix(V, u, inv, False, rp)
    return q, qr, subpix_ref.subpix(V, u, inv, True, rp)


def _chain(q, qr, r, lr, post=True):
    """views -> median16_ref.subpix_median -> speckle_ref (size 20, range 16 * 1) -> fill_ref (gap 12):
    (left map, right map, mask)."""
    qm, qrm, mask = median16_ref.subpix_median(q, qr, r, lr)
    if post:
        qm, mask = speckle_ref.speckle(qm, SPECKLE, 16, mask)
        qm = fill_ref.fill(qm, GAP)
    return qm, qrm, mask


def _exercised(q, qr, checked_mask, r):
    """What the cases must show on the reference: the filter changes both views, the mask differs from the unfiltered
    call's, and the check on the rounded maps differs from a check on the floored ones."""
    a, b = median16_ref.median(q, r), median16_ref.median(qr, r)
    _, _, mask = median16_ref.subpix_median(q, qr, r, True)
    occ_round = subpix_ref.lr_occluded(median16_ref.rounded(a), median16_ref.rounded(b))
    occ_floor = subpix_ref.lr_occluded(a >> 4, b >> 4)
    return int((a != q).sum()), int((b != qr).sum()), int((mask != checked_mask).sum()), \
        int((occ_round != occ_floor).sum())


@pytest.mark.parametrize("u", [0, 10])
@pytest.mark.parametrize("r", RADII)
@pytest.mark.parametrize("agg,cost", PATHS)
def test_matching_calls(matcher, oracle, agg, cost, r, u):
    import torch
    L, R = _pair()
    kw = dict(agg=agg, cost=cost)
    q, qr, (q_chk, _, mask_chk) = _views(agg, cost, u)
    q2, qr2, _ = _views(agg, cost, u, True)
    # non-vacuity, on the reference: the worst case over these paths, u and r is census SGM, u = 0, r = 1 with
    # 504 / 793 / 49 pixels, and box AD, u = 10, r = 1 with 14 for the rounding
    left_changed, right_changed, mask_changed, rounding = _exercised(q, qr, mask_chk, r)
    print(f"{agg}/{cost} u={u} r={r}: left {left_changed}, right {right_changed}, mask {mask_changed}, "
          f"rounding {rounding} of {q.size}")
    assert left_changed > 0 and right_changed > 0 and mask_changed > 0 and rounding > 0
    assert left_changed >= 450 and right_changed >= 790 and mask_changed >= 49 and rounding >= 14

    Lt, Rt = (torch.from_numpy(np.stack([a, b])).cuda() for a, b in zip(_pair(), _pair(True)))
    big = torch.zeros((2, PH + 4, PW + 10), dtype=torch.int16, device="cuda")
    out_win = big[:, 3:3 + PH, 5:5 + PW]
    rt = torch.empty((2, PH, PW), dtype=torch.int16, device="cuda")
    mt = torch.empty((2, PH, PW), dtype=torch.uint8, device="cuda")
    matcher.set_uniqueness(u)
    matcher.set_speckle(SPECKLE, 1)
    matcher.set_fill(GAP)
    matcher.set_subpix_median(r)
    try:
        got_lr = matcher.match_subpix(L, R, PR, PD, lr_check=True, return_right=True, return_mask=True, **kw)
        got_un = matcher.match_subpix(L, R, PR, PD, lr_check=False, return_right=True, return_mask=True, **kw)
        got_alone = matcher.match_subpix(L, R, PR, PD, lr_check=True, **kw)     # no right16: the temporary plane
        got_left = matcher.match_subpix(L, R, PR, PD, lr_check=False, **kw)     # no right view at all
        dev = matcher.match_subpix_device(Lt, Rt, PR, PD, out_t=out_win, lr_check=True, right_t16=rt, mask_t=mt, **kw)
        torch.cuda.synchronize()
    finally:
        matcher.set_subpix_median(0)
        matcher.set_fill(0)
        matcher.set_speckle()
        matcher.set_uniqueness(0)
    want = _chain(q, qr, r, True)
    for g, w, name in zip(got_lr, want, ("map", "right map", "mask")):
        assert np.array_equal(g, w), f"match_subpix lr: {name}, {int((g != w).sum())} pixels differ"
    want_un = _chain(q, qr, r, False)
    for g, w, name in zip(got_un, want_un, ("map", "right map", "mask")):
        assert np.array_equal(g, w), f"match_subpix no check: {name}, {int((g != w).sum())} pixels differ"
    assert np.array_equal(got_alone, want[0]) and np.array_equal(got_left, want_un[0])
    assert dev.data_ptr() == out_win.data_ptr()
    got_big = _host(big)
    for b, (qa, qb) in enumerate(((q, qr), (q2, qr2))):
        w = _chain(qa, qb, r, True)
        assert np.array_equal(got_big[b, 3:3 + PH, 5:5 + PW], w[0]), b
        assert np.array_equal(_host(rt)[b], w[1]) and np.array_equal(mt.cpu().numpy()[b], w[2]), b
    got_big[:, 3:3 + PH, 5:5 + PW] = 0
    assert not got_big.any()                                   # nothing written around the window


@pytest.mark.parametrize("r", RADII)
@pytest.mark.parametrize("cost", ["ad", "census"])
def test_volume_wta_on_the_sgm_sum(matcher, oracle, cost, r):
    """sm_volume_wta_subpix_device on the SGM sum S as a caller's volume (it runs neither speckle nor fill)."""
    import torch
    V, inv, rp = _volume("sgm", cost)
    assert inv == 0 and rp == 1
    S = np.where(subpix_ref.left_exists(*V.shape), V, 0).astype(np.int32)
    vt = torch.from_numpy(S).cuda()
    for u in (0, 10):
        q, qr, _ = _views("sgm", cost, u)
        matcher.set_uniqueness(u)
        matcher.set_subpix_median(r)
        try:
            for lr in (True, False):
                rt = torch.empty((PH, PW), dtype=torch.int16, device="cuda")
                mt = torch.empty((PH, PW), dtype=torch.uint8, device="cuda")
                qt = matcher.volume_wta_subpix_device(vt, 0, lr, right_t16=rt, mask_t=mt)
                alone = matcher.volume_wta_subpix_device(vt, 0, lr)
                torch.cuda.synchronize()
                w = _chain(q, qr, r, lr, post=False)
                assert np.array_equal(_host(qt), w[0]) and np.array_equal(_host(rt), w[1]), (u, lr)
                assert np.array_equal(mt.cpu().numpy(), w[2]) and np.array_equal(_host(alone), w[0]), (u, lr)
        finally:
            matcher.set_subpix_median(0)
            matcher.set_uniqueness(0)


def test_in_view_pairs_with_a_minimum_disparity(matcher, oracle):
    """pairs='in-view', set_min_disp(20): the views of tests/pairs_ref.py, absolute disparities 20 .. 51."""
    L, R = _pair()
    d0, r = 20, 2
    ref = pairs_ref.Reference(L, R, PR, PD, "in-view", d0)
    q, qr, _ = ref.subpix("sgm", "census", 0, False)
    assert q.max() > 16 * 32                                   # beyond what the reference rule's D = 32 reaches
    matcher.set_min_disp(d0)
    matcher.set_subpix_median(r)
    try:
        got = matcher.match_subpix(L, R, PR, PD, agg="sgm", cost="census", lr_check=True, return_right=True,
                                   return_mask=True, pairs="in-view")
    finally:
        matcher.set_subpix_median(0)
        matcher.set_min_disp(0)
    want = _chain(q, qr, r, True, post=False)
    assert all(np.array_equal(g, w) for g, w in zip(got, want))
    assert want[2].any() and not want[2].all()


def test_parameter(matcher, sm_mod, oracle):
    import torch
    L, R = _pair()
    Lt, Rt = torch.from_numpy(np.array(L)).cuda(), torch.from_numpy(np.array(R)).cuda()
    sub = lambda: matcher.match_subpix(L, R, PR, PD, lr_check=True, return_right=True, return_mask=True)  # noqa: E731
    before = sub()
    q, qr, ref_chk = _views("sgm", "ad", 0)
    assert all(np.array_equal(a, b) for a, b in zip(before, ref_chk))
    eight = (matcher.match(L, R, PR, PD, agg="sgm"), matcher.match_lr(L, R, PR, PD, agg="sgm", median=True),
             matcher.match_device(Lt, Rt, PR, PD, agg="sgm", lr_check=True).cpu().numpy())
    try:
        for bad in (-1, 4, 1.5):
            with pytest.raises(sm_mod.SMError, match="SM_PARAM_SUBPIX_MEDIAN") as e:
                matcher.set_subpix_median(bad)
            assert e.value.code == sm_mod._capi.SM_ERR_INVALID_ARG
            assert all(np.array_equal(a, b) for a, b in zip(sub(), before))      # refused: still off
        matcher.set_subpix_median(2)
        with pytest.raises(sm_mod.SMError, match="SM_PARAM_SUBPIX_MEDIAN"):
            matcher.set_subpix_median(7)
        on = sub()
        assert all(np.array_equal(a, b) for a, b in zip(on, _chain(q, qr, 2, True, post=False)))   # refused: still 2
        assert not np.array_equal(on[0], before[0]) and not np.array_equal(on[1], before[1])
        matcher.set_subpix_median(3)
        again = (matcher.match(L, R, PR, PD, agg="sgm"), matcher.match_lr(L, R, PR, PD, agg="sgm", median=True),
                 matcher.match_device(Lt, Rt, PR, PD, agg="sgm", lr_check=True).cpu().numpy())
        for a, b in zip(eight, again):      # the 8-bit calls ignore it
            assert all(np.array_equal(x, y) for x, y in zip(a, b)) if isinstance(a, tuple) else np.array_equal(a, b)
        flags = sm_mod._capi.SM_AGG_SGM | sm_mod._capi.SM_MEDIAN
        out = np.empty((PH, PW), np.uint16)
        rc = matcher._lib.sm_block_match_subpix_u16(matcher._h, L.ctypes.data, R.ctypes.data, PW, PH, PW, PR, PD, flags,
                                                    out.ctypes.data, None, None, PW)
        with pytest.raises(sm_mod.SMError, match="SM_MEDIAN"):
            sm_mod._capi.check(rc)
    finally:
        matcher.set_subpix_median(0)
    assert all(np.array_equal(a, b) for a, b in zip(sub(), before))              # back at 0: bit for bit


def test_books_census_sgm_lr(matcher, oracle, gray):
    """Books, r = 2, D = 80, census SGM, LR check, median r = 1: the maps are the reference chain's.  Over gt > 0
    (gt = disp1 / 3), with bad = |q / 16 - gt| > 1 or a hole and MAE = mean |q / 16 - gt| over the valid pixels
    within 1 px, the CPU reference gives bad 0.3493 -> 0.3472 and MAE 0.2785 -> 0.2768 with the median."""
    L, R = gray["Books/view1"], gray["Books/view5"]
    gt = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "middlebury_gt.npz"))["Books/disp1"]
    gt = gt.astype(np.float64) / 3.0
    V, inv, rp = subpix_ref.volume(oracle, L, R, 2, 80, "sgm", "census")
    q, qr, _ = subpix_ref.subpix(V, 0, inv, False, rp)
    plain_ref = subpix_ref.subpix(V, 0, inv, True, rp)
    want = median16_ref.subpix_median(q, qr, 1, True)
    kw = dict(agg="sgm", cost="census", lr_check=True, return_right=True, return_mask=True)
    plain = matcher.match_subpix(L, R, 2, 80, **kw)
    matcher.set_subpix_median(1)
    try:
        got = matcher.match_subpix(L, R, 2, 80, **kw)
    finally:
        matcher.set_subpix_median(0)
    for g, w, name in zip(got, want, ("map", "right map", "mask")):
        assert np.array_equal(g, w), f"{name}: {int((g != w).sum())} pixels differ"
    assert all(np.array_equal(g, w) for g, w in zip(plain, plain_ref))

    def figures(m):
        v = gt > 0
        d = m.astype(np.float64) / 16.0
        bad = float(((np.abs(d - gt) > 1) | (m == 0))[v].mean())
        near = v & (m != 0) & (np.abs(d - gt) <= 1)
        return bad, float(np.abs(d - gt)[near].mean())

    (bad0, mae0), (bad1, mae1) = figures(plain[0]), figures(got[0])
    print(f"Books census SGM + LR, 1/16 px: bad {bad0:.4f} -> {bad1:.4f}, MAE {mae0:.4f} -> {mae1:.4f} with the "
          f"3 x 3 median")
    assert (round(bad0, 4), round(mae0, 4)) == (0.3493, 0.2785)
    assert (round(bad1, 4), round(mae1, 4)) == (0.3472, 0.2768)
