"""GPU row fill (sm_fill_invalid_*, SM_PARAM_FILL_GAP) against the numpy restatement of its contract
(tests/fill_ref.py).  Integer arithmetic end to end, so every comparison is bit-exact: the map, the mask it must
leave alone and the bytes between width and pitch.

The kernel (csrc/bm_fill.hip) gives one lane a pixel, one wave a 64-pixel segment and one second-level ballot 64
segments = 4096 columns; wider rows carry the last valid pixel from chunk to chunk.  The shapes below are the
smallest that reach each of those edges.
"""
import functools

import numpy as np
import pytest

import census_ref
import fill_ref
import sgm_ref
import speckle_ref
import subpix_ref

pytestmark = pytest.mark.gpu

SEG, CHUNK = 64, 4096
FILL_ALL = 1 << 24
DTYPES = [np.uint8, np.uint16]


@pytest.fixture(scope="module")
def sm_mod():
    import gpu_stereo_matching_amd as sm
    return sm


@pytest.fixture(scope="module")
def matcher(sm_mod):
    m = sm_mod.BlockMatcher(0, 4100, 370, 256)
    yield m
    m.close()


def check(matcher, img, gap):
    """The host call against the reference."""
    want = fill_ref.fill(img, gap)
    got = matcher.fill_invalid(img, gap)
    assert got.dtype == img.dtype and got.shape == img.shape
    bad = np.argwhere(got != want)
    assert len(bad) == 0, f"{len(bad)} of {img.size} pixels differ at max_gap {gap}, first (y, x) = {bad[0].tolist()}"
    return got


def valid_rows(seed, dtype, H, W):
    """H x W of random valid values: neighbours differ, and uint16 values differ in both bytes."""
    top = 255 if dtype == np.uint8 else 65535
    return np.random.default_rng(seed).integers(1, top + 1, (H, W)).astype(dtype)


def with_runs(seed, dtype, W, rows):
    """One row per entry of `rows`, each a list of runs (a, b) of invalid columns, cut to the row's width."""
    img = valid_rows(seed, dtype, len(rows), W)
    for y, runs in enumerate(rows):
        for a, b in runs:
            img[y, a:min(b, W - 1) + 1] = 0
    return img


def gaps_for(img):
    """Every run length in the map, one less and one more, and the limits of the range."""
    W = img.shape[1]
    lengths = set()
    for row in img:
        edges = np.flatnonzero(np.diff(np.concatenate(([0], (row == 0).astype(np.int8), [0]))))
        lengths |= set((edges[1::2] - edges[0::2]).tolist())
    g = {1, 2, W - 1, W, FILL_ALL}
    for n in lengths:
        g |= {n - 1, n, n + 1}
    return sorted(v for v in g if 1 <= v <= FILL_ALL)


# runs at the edges of a 64-lane segment and of the 4096-column chunk; a row per case, cut to the width under test
SEGMENT_ROWS = [
    [(60, 63), (128, 130)],                      # ends on a segment's last lane; starts on a segment's first lane
    [(63, 64), (127, 128)],                      # two pixels, one in each segment
    [(30, 200)],                                 # spans three segment edges (segments 0 .. 3)
    [(0, 63), (65, 127)],                        # a whole segment from the left border; a valid pixel alone at 64
    [(1, 62), (64, 64), (66, 4098)],             # valid pixels only at a segment's two ends
]
CHUNK_ROWS = [
    [(4000, 4097)],                              # crosses column 4096: both neighbours known only in the 2nd chunk
    [(4095, 4096)],                              # one pixel on each side of the chunk edge
    [(3000, 4099)],                              # crosses it to the right border: left neighbour only, from the carry
    [(0, 4096)],                                 # from the left border across it: right neighbour only, no carry
    [(0, 4090), (4092, 4095), (4097, 4098)],     # one valid pixel in the first chunk, runs on both sides of the edge
]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("W", [1, 2, 63, 64, 65, 128, 129, 4100])
def test_widths_and_segment_edges(matcher, dtype, W):
    img = with_runs(W, dtype, W, SEGMENT_ROWS)
    assert img.shape == (5, W)
    for gap in gaps_for(img):
        check(matcher, img, gap)
    if W > CHUNK:
        img = with_runs(W + 1, dtype, W, CHUNK_ROWS)
        for gap in gaps_for(img):
            check(matcher, img, gap)
        assert check(matcher, img, W).all()      # every row has a valid pixel: nothing is left


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("W", [1, 2, 65, 130, 4100])
def test_row_cases(matcher, dtype, W):
    """All invalid, all valid, only the first / only the last pixel valid, a run at each border."""
    img = valid_rows(W, dtype, 5, W)
    img[0] = 0
    img[2, 1:] = 0
    img[3, :-1] = 0
    if W > 5:
        img[4, :3] = 0
        img[4, -2:] = 0
    for gap in gaps_for(img):
        got = check(matcher, img, gap)
        assert not got[0].any() and np.array_equal(got[1], img[1])
    full = check(matcher, img, W)
    assert (full[2] == img[2, 0]).all() and (full[3] == img[3, -1]).all()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("share", [0.05, 0.3, 0.95])
def test_random_maps(matcher, dtype, share):
    rng = np.random.default_rng(int(share * 100))
    img = valid_rows(7, dtype, 37, 299)
    img[rng.random(img.shape) < share] = 0
    assert abs(float(np.mean(img == 0)) - share) < 0.02
    for gap in (0, 1, 2, 3, 7, 64, 298, 299, FILL_ALL):
        got = check(matcher, img, gap)
        if gap == 0:
            assert np.array_equal(got, img)


def test_uint16_takes_the_whole_element(matcher):
    """Values whose order differs between the low byte and the whole value."""
    b = np.array([[0x00FF, 0, 0x0100, 0, 0xFFFF, 0, 0x0001, 0, 0, 0x0100, 0, 0x00FF]], np.uint16)
    got = check(matcher, b, 2)
    assert got.tolist() == [[0x00FF, 0x00FF, 0x0100, 0x0100, 0xFFFF, 0x0001, 0x0001, 0x0001, 0x0001, 0x0100, 0x00FF,
                             0x00FF]]
    wide = np.zeros((2, 200), np.uint16)           # the same across segment edges
    wide[0, 10], wide[0, 150] = 0x01FF, 0x0200
    wide[1, 10], wide[1, 150] = 0xFF00, 0x00FF
    got = check(matcher, wide, 200)
    assert (got[0, 11:150] == 0x01FF).all() and (got[1, 11:150] == 0x00FF).all()


@pytest.mark.parametrize("dtype", DTYPES)
def test_max_gap_is_the_run_length(matcher, dtype):
    """Border runs of 3 and 2 pixels and an inner run of 4: each is filled from max_gap = its length on."""
    a = np.array([[0, 0, 0, 5, 0, 0, 0, 0, 7, 0, 0]], dtype)
    assert check(matcher, a, 1).tolist() == a.tolist()
    assert check(matcher, a, 2).tolist() == [[0, 0, 0, 5, 0, 0, 0, 0, 7, 7, 7]]
    assert check(matcher, a, 3).tolist() == [[5, 5, 5, 5, 0, 0, 0, 0, 7, 7, 7]]
    assert check(matcher, a, 4).tolist() == [[5, 5, 5, 5, 5, 5, 5, 5, 7, 7, 7]]
    # the same lengths across segment edges: a left-border run of 70, an inner run of 100, a right-border run of 66
    img = with_runs(3, dtype, 300, [[(0, 69), (100, 199), (234, 299)]])
    for gap in (65, 66, 69, 70, 99, 100):
        check(matcher, img, gap)
    assert (check(matcher, img, 66)[0, 234:] == img[0, 233]).all() and not check(matcher, img, 65)[0, 234:].any()


def _to_device(a):
    import torch
    return torch.from_numpy(a.view(np.int16) if a.dtype == np.uint16 else a).cuda()


def _to_host(t, dtype):
    a = t.cpu().numpy()
    return a.view(np.uint16) if dtype == np.uint16 else a


@pytest.mark.parametrize("dtype", DTYPES)
def test_pitch_and_padding(matcher, dtype):
    """Rows of W elements at a pitch of W + 6.  The padding holds sentinels, and zeros right behind border runs and
    in front of the next row's border run: it comes back byte for byte and is never a neighbour."""
    import torch
    H, W = 6, 131
    rng = np.random.default_rng(2)
    img = valid_rows(5, dtype, H, W)
    img[rng.random(img.shape) < 0.3] = 0
    img[1, W - 4:] = 0          # a right-border run, followed by padding
    img[2, :5] = 0              # a left-border run, behind the row above's padding
    img[3, :] = 0               # a row with nothing but padding beside it
    buf = np.full((H, W + 6), 0xAB if dtype == np.uint8 else 0xABCD, dtype)
    buf[:, :W] = img
    buf[1, W] = 0               # a zero that would lengthen the run past max_gap if it were read
    buf[1, W + 5] = 1           # a small value that would win the minimum of row 2's border run
    buf[3, W:] = 7              # values a row without a valid pixel must not take
    for gap in (4, 5, W):
        t = _to_device(buf)
        view = t[:, :W]
        assert view.stride(0) == W + 6
        matcher.fill_invalid_device(view, gap)
        torch.cuda.synchronize()
        got = _to_host(t, dtype)
        want = fill_ref.fill(img, gap)
        assert np.array_equal(got[:, :W], want) and (want != img).any()
        assert np.array_equal(got[:, W:], buf[:, W:])
    assert (want[1, W - 4:] == img[1, W - 5]).all() and (want[2, :5] == img[2, 5]).all() and not want[3].any()


@pytest.mark.parametrize("dtype", DTYPES)
def test_batch_and_views(matcher, dtype):
    """Three frames at a frame stride above pitch * H, each equal to its single-frame call; the rows between the
    frames stay; and a window cut out of the middle of a larger tensor."""
    import torch
    H, W, gap = 5, 200, 9
    rng = np.random.default_rng(8)
    big = valid_rows(21, dtype, 3 * (H + 2), W + 3).reshape(3, H + 2, W + 3)
    big[rng.random(big.shape) < 0.4] = 0
    t = _to_device(big)
    view = t[:, :H, :W]
    assert view.stride(0) == (H + 2) * (W + 3) > view.stride(1) * H
    matcher.fill_invalid_device(view, gap)
    singles = [matcher.fill_invalid_device(_to_device(np.ascontiguousarray(big[b, :H, :W])), gap) for b in range(3)]
    torch.cuda.synchronize()
    got = _to_host(t, dtype)
    want = big.copy()
    for b in range(3):
        want[b, :H, :W] = fill_ref.fill(big[b, :H, :W], gap)
        assert np.array_equal(_to_host(singles[b], dtype), want[b, :H, :W])
    assert np.array_equal(got, want) and (want != big).any()
    # a window in the middle of one frame: the columns left and right of it are valid or not, and never used
    t = _to_device(big[0])
    win = t[1:6, 2:150]
    matcher.fill_invalid_device(win, gap)
    torch.cuda.synchronize()
    want = big[0].copy()
    want[1:6, 2:150] = fill_ref.fill(big[0, 1:6, 2:150], gap)
    assert np.array_equal(_to_host(t, dtype), want)


# ---- the matching calls ----
PW, PH, PD, PR = 96, 40, 32, 2
GAP = 12
PATHS = [("box", "ad"), ("sgm", "ad"), ("sgm", "census")]


@functools.lru_cache(maxsize=None)
def _pair(flip=False):
    """96 x 40, D = 32: oracle.synth_pair with +-4 noise on the right image (as test_gpu_sgm.py's pairs)."""
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
def _matching_ref(agg, cost, flip=False):
    """The CPU references of one path on the pair, computed once: (left map, right map, checked map, mask) and the
    LR-checked 1/16-px (q, right q, mask)."""
    from oracle import oracle as O
    O.build()
    L, R = _pair(flip)
    if agg == "box":
        eight = O.box_lr(L, R, PR, PD)
    elif cost == "census":
        eight = census_ref.census_lr(O, L, R, PR, PD, "sgm")
    else:
        eight = sgm_ref.sgm_lr(O, L, R, PR, PD, *sgm_ref.auto_penalties(PR))
    V, inv, pairs = subpix_ref.volume(O, L, R, PR, PD, agg, cost)
    return eight, subpix_ref.subpix(V, 0, inv, True, pairs)


def _chain(img, mask, speckle, diff=1):
    """reference map -> speckle_ref -> fill_ref: (unfilled map, its mask, filled map)."""
    if speckle:
        img, mask = speckle_ref.speckle(img, speckle, diff, mask)
    return img, mask, fill_ref.fill(img, GAP)


@pytest.mark.parametrize("speckle", [0, 20])
@pytest.mark.parametrize("agg,cost", PATHS)
def test_matching_calls_end_with_the_fill(matcher, oracle, agg, cost, speckle):
    import torch
    L, R = _pair()
    kw = dict(agg=agg, cost=cost)
    (dl, dr, checked, mask), (q, qr, qmask) = _matching_ref(agg, cost)
    (dl2, _, checked2, mask2), _ = _matching_ref(agg, cost, True)
    Lt, Rt = (torch.from_numpy(np.stack([a, b])).cuda() for a, b in zip(_pair(), _pair(True)))
    matcher.set_speckle(speckle, 1)
    matcher.set_fill(GAP)
    try:
        got = matcher.match(L, R, PR, PD, **kw)
        got_lr = matcher.match_lr(L, R, PR, PD, **kw)
        got_dev = matcher.match_device(Lt, Rt, PR, PD, **kw).cpu().numpy()
        got_dev_lr = matcher.match_device(Lt, Rt, PR, PD, lr_check=True, **kw).cpu().numpy()
        got_sub = matcher.match_subpix(L, R, PR, PD, lr_check=True, return_right=True, return_mask=True, **kw)
        matcher.set_fill(0)
        off_lr = matcher.match_lr(L, R, PR, PD, **kw)
        off_sub = matcher.match_subpix(L, R, PR, PD, lr_check=True, return_right=True, return_mask=True, **kw)
    finally:
        matcher.set_fill(0)
        matcher.set_speckle()
    # match: the unchecked map
    un, _, want = _chain(dl, None, speckle)
    assert np.array_equal(got, want)
    # match_lr: the checked map is filled, the right map and the mask are the unfilled call's
    un, un_mask, want = _chain(checked, mask, speckle)
    assert np.array_equal(off_lr[0], un) and np.array_equal(off_lr[2], un_mask)
    assert np.array_equal(got_lr[0], want)
    assert np.array_equal(got_lr[1], dr) and np.array_equal(got_lr[1], off_lr[1])
    assert np.array_equal(got_lr[2], un_mask)
    was_filled = fill_ref.filled(un, want)
    assert was_filled.sum() > 50 and (un == 0).sum() > was_filled.sum()     # something filled, something too long
    assert np.array_equal((got_lr[2] == 0) & (got_lr[0] != 0), was_filled)
    # match_device, a batch of the pair and the flipped pair
    for b, (raw, chk, mk) in enumerate(((dl, checked, mask), (dl2, checked2, mask2))):
        assert np.array_equal(got_dev[b], _chain(raw, None, speckle)[2]), b
        assert np.array_equal(got_dev_lr[b], _chain(chk, mk, speckle)[2]), b
    # match_subpix with the LR check: the 1/16-px map, speckle range in 1/16 px
    un, un_mask, want = _chain(q, qmask, speckle, 16)
    assert np.array_equal(off_sub[0], un) and np.array_equal(off_sub[2], un_mask)
    assert np.array_equal(got_sub[0], want) and np.array_equal(got_sub[1], qr) and np.array_equal(got_sub[2], un_mask)
    assert np.array_equal((got_sub[2] == 0) & (got_sub[0] != 0), fill_ref.filled(un, want))
    assert fill_ref.filled(un, want).any()


def test_row_band_calls_honour_it(matcher, sm_mod, oracle):
    """Two bands on one device: the kept rows are the whole-frame call's rows."""
    L, R = _pair()
    with sm_mod.BlockMatcherGroup([0, 0], PW, PH, PD) as g:
        plain = g.match(L, R, PR, PD)
        g.set_fill(GAP)
        got = g.match(L, R, PR, PD)
        got_lr = g.match_lr(L, R, PR, PD)
        outs = g.match_batch([L, L, L], [R, R, R], PR, PD)
        g.set_speckle(20, 1)
        with pytest.raises(sm_mod.SMError, match="speckle"):      # the speckle filter's refusal comes first
            g.match(L, R, PR, PD)
        g.set_speckle()
        g.set_fill()
        assert np.array_equal(g.match(L, R, PR, PD), plain)
    dl, dr, checked, mask = _matching_ref("box", "ad")[0]
    assert np.array_equal(plain, dl)
    want = fill_ref.fill(dl, GAP)
    assert np.array_equal(got, want) and (want != dl).any()
    assert all(np.array_equal(o, want) for o in outs)
    assert np.array_equal(got_lr[0], fill_ref.fill(checked, GAP))
    assert np.array_equal(got_lr[1], dr) and np.array_equal(got_lr[2], mask)


def test_calls_that_cannot_honour_it_say_so(matcher, sm_mod, oracle):
    import torch
    L, R = _pair()
    Lt, Rt = torch.from_numpy(np.array(L)).cuda(), torch.from_numpy(np.array(R)).cuda()
    plain = matcher.match(L, R, PR, PD)
    matcher.set_fill(GAP)
    try:
        for call in (lambda: matcher.dslice_rehearse(L, R, PR, PD, 2),
                     lambda: matcher.slice_keys_device(Lt, Rt, PR, 0, PD),
                     lambda: matcher.guided_slice_keys_device(Lt, Rt, PR, 0, PD),
                     lambda: matcher.slice_keys_lr_device(Lt, Rt, PR, 0, PD)):
            with pytest.raises(sm_mod.SMError, match="fill") as e:
                call()
            assert e.value.code == sm_mod._capi.SM_ERR_INVALID_ARG
    finally:
        matcher.set_fill(0)
    assert np.array_equal(matcher.dslice_rehearse(L, R, PR, PD, 2), plain)
    with sm_mod.BlockMatcherGroup([0, 0], PW, PH, PD) as g:
        g.set_fill(GAP)
        with pytest.raises(sm_mod.SMError, match="fill") as e:
            g.match_dslice(L, R, PR, PD)
        assert e.value.code == sm_mod._capi.SM_ERR_INVALID_ARG
        g.set_fill()
        assert np.array_equal(g.match(L, R, PR, PD), plain)


def test_parameter_range_and_default(matcher, sm_mod, oracle):
    L, R = _pair()
    before = matcher.match_lr(L, R, PR, PD, agg="sgm")
    try:
        for gap in (-1, FILL_ALL + 2, 2 ** 25):     # (2^24 + 1 is no float: it would arrive as 2^24)
            with pytest.raises(sm_mod.SMError, match="fill"):
                matcher.set_fill(gap)
        with pytest.raises(sm_mod.SMError, match="fill"):
            sm_mod._capi.check(matcher._lib.sm_set_param_f(matcher._h, sm_mod._capi.SM_PARAM_FILL_GAP, 1.5))
        # a refused value leaves the parameter as it was: still off
        assert all(np.array_equal(a, b) for a, b in zip(matcher.match_lr(L, R, PR, PD, agg="sgm"), before))
        matcher.set_fill(FILL_ALL)
        on = matcher.match_lr(L, R, PR, PD, agg="sgm")
        assert np.array_equal(on[0], fill_ref.fill(before[0], FILL_ALL)) and not np.array_equal(on[0], before[0])
    finally:
        matcher.set_fill(0)
    after = matcher.match_lr(L, R, PR, PD, agg="sgm")
    assert all(np.array_equal(a, b) for a, b in zip(after, before))      # back at 0: the parent's maps, bit for bit
    with pytest.raises(sm_mod.SMError, match="max_gap"):
        matcher.fill_invalid(np.ones((4, 4), np.uint8), -1)
    with pytest.raises(sm_mod.SMError, match="max_gap"):
        matcher.fill_invalid(np.ones((4, 4), np.uint8), FILL_ALL + 1)
    with pytest.raises(sm_mod.SMError):
        matcher.fill_invalid(np.ones((400, 700), np.uint8), 1)           # beyond the handle's 4100 x 370 rows


def test_books_census_sgm_lr_speckle_fill(matcher, oracle, gray):
    """The pipeline the issue measured: Books, r = 2, D = 80, census SGM, LR check, speckle(200, 1), every run
    filled.  The map is the reference chain's, and the bad-pixel rate (|d - gt| > 1 over gt > 0, gt = disp1 / 3)
    the CPU figure, 0.2414, down from 0.3431 before the fill."""
    import os
    L, R = gray["Books/view1"], gray["Books/view5"]
    gt = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "middlebury_gt.npz"))["Books/disp1"]
    gt = gt.astype(np.float64) / 3.0
    _, dr, checked, mask = census_ref.census_lr(oracle, L, R, 2, 80, "sgm")
    spk, spk_mask = speckle_ref.speckle(checked, 200, 1, mask)
    want = fill_ref.fill(spk, FILL_ALL)
    matcher.set_speckle(200, 1)
    matcher.set_fill(FILL_ALL)
    try:
        c, rr, mm = matcher.match_lr(L, R, 2, 80, agg="sgm", cost="census")
    finally:
        matcher.set_fill(0)
        matcher.set_speckle()
    assert np.array_equal(c, want) and np.array_equal(rr, dr) and np.array_equal(mm, spk_mask)
    assert np.array_equal((mm == 0) & (c != 0), fill_ref.filled(spk, want))
    rate = sgm_ref.bad_rate(c, gt)
    print(f"Books census SGM + LR + speckle(200, 1): {sgm_ref.bad_rate(spk, gt):.4f}, + row fill: {rate:.4f}")
    assert round(rate, 4) == 0.2414
