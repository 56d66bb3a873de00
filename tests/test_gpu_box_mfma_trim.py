"""The matrix-pipe box kernel's unmasked paired loop with its pass constants and R addresses carried from pass to
pass (bm_box_mfma.hip): the two key constants step by 2.0 instead of being rebuilt from d, the two R
addresses step by two columns with the swizzle term taken from the stepped column offset, and an odd last pass labels
its repeated disparity d + 1.  Maps and slice keys must still equal oracle.box_disp / box_keys_slice and the VALU
kernels (set_box_kernel(1)) bit for bit.  The shapes are the smallest at which that can go wrong:
  - d-slices of 1..9 disparities from an odd d_lo (wave ranges 0..3 long, odd ranges that end on a repeated d);
  - long slices from d_lo = 37, so a wave walks 5 to 27 passes and the swizzle term wraps mod 8 several times.  The
    d_max instantiation follows from the slice's length alone, so the slice of 40 runs <r, 64> and slices of 104, 168
    and 219 run <r, 128>, <r, 192> and <r, 256>;
  - a constant image, where every d ties and the smaller d must win, also against the relabelled odd last pass;
  - rows of several carried tiles per d_max with 1, 2, 3 and auto workgroups (a range then starts mid-row, crosses a
    row end and ends on the masked right-edge tile behind carried ones), r = 7 once, and a 2-frame batch, so a
    workgroup passes from one frame to the next.
The references of a shape are computed once and shared."""
import numpy as np
import pytest

from test_gpu_box_mfma_pairs import LEGACY, MATRIX, _keys, _maps, _pair

pytestmark = pytest.mark.gpu

WORKGROUPS = (1, 2, 3, 0)
# band slack in tiles a d_max could hold in a third of the LDS (not built): the rows are m + 2 tiles wide
SLACK_TILES = {64: 4, 128: 2, 192: 1, 256: 0}
_refs = {}


@pytest.fixture(scope="module")
def env():
    import torch
    import gpu_stereo_matching_amd as sm
    from oracle import oracle as O
    with sm.BlockMatcher(0, 400, 100, 256) as m:
        yield sm, torch, O, m


def _with_n(env, n, fn, *args):
    m = env[3]
    m.set_box_workgroups(n)
    try:
        return fn(env, *args)
    finally:
        m.set_box_workgroups(0)


def _ref(env, key, L, R, r, D):
    """Oracle map and keys of [0, D) and the VALU kernels' map and keys, once per key."""
    if key not in _refs:
        want, want_keys = env[2].box_disp(L, R, r, D, want_keys=True)
        _refs[key] = (want, want_keys, _maps(env, L, R, r, D, LEGACY), _keys(env, L, R, r, 0, D, LEGACY))
    return _refs[key]


def _ref_slice(env, key, L, R, r, d_lo, d_hi):
    if key not in _refs:
        _refs[key] = (env[2].box_keys_slice(L, R, r, d_lo, d_hi), _keys(env, L, R, r, d_lo, d_hi, LEGACY))
    return _refs[key]


@pytest.mark.parametrize("n", (1, 3, 0))
@pytest.mark.parametrize("nd", range(1, 10))
@pytest.mark.parametrize("W,H,r,d_lo", [(260, 100, 5, 37), (200, 50, 7, 21)])
def test_short_slices_from_an_odd_d_lo(env, W, H, r, d_lo, nd, n):
    """nd = 1..9 disparities over four waves: ranges of 0..3, odd ranges end on their last d twice, labelled d + 1."""
    L, R = _pair(env, 600 + r, W, H, 64)
    want, old = _ref_slice(env, ("slice", W, H, r, d_lo, nd), L, R, r, d_lo, d_lo + nd)
    assert np.array_equal(old, want)
    got = _with_n(env, n, _keys, L, R, r, d_lo, d_lo + nd, MATRIX)
    assert np.array_equal(got, want), int((got != want).sum())


@pytest.mark.parametrize("n", (1, 0))
@pytest.mark.parametrize("r", (5, 7))
@pytest.mark.parametrize("nd", (40, 104, 168, 219))
def test_long_slices_wrap_the_swizzle(env, nd, r, n):
    """From d_lo = 37 on 330 x 50: 5 to 27 passes per wave, the stepped swizzle term wraps mod 8 up to three times;
    one slice per d_max instantiation."""
    W, H, d_lo = 330, 50, 37
    L, R = _pair(env, 610 + r, W, H, 64)
    want, old = _ref_slice(env, ("long", r, nd), L, R, r, d_lo, d_lo + nd)
    assert np.array_equal(old, want)
    got = _with_n(env, n, _keys, L, R, r, d_lo, d_lo + nd, MATRIX)
    assert np.array_equal(got, want), int((got != want).sum())
    assert len(np.unique(got & 0xFF)) > 8   # a textured pair: many disparities win somewhere


@pytest.mark.parametrize("n", (1, 3, 0))
@pytest.mark.parametrize("W,H,D,r", [(260, 100, 128, 5), (200, 50, 64, 7)])
def test_constant_image_ties_go_to_the_smaller_d(env, W, H, D, r, n):
    """L = R = 77: the cost of every valid d is 0 at every pixel, so every key is d = 0's and the map is 0; in a
    slice the tie goes to d_lo, the first d of a pair or, for the odd-length range, its last (relabelled d + 1 in
    the pass, which must lose)."""
    L = np.full((H, W), 77, np.uint8)
    R = L.copy()
    want, want_keys, old, old_keys = _ref(env, ("const", W, H, D, r), L, R, r, D)
    assert np.array_equal(old, want) and np.array_equal(old_keys, want_keys)
    assert not want.any() and not (want_keys & 0xFF).any()
    got = _with_n(env, n, _maps, L, R, r, D, MATRIX)
    kg = _with_n(env, n, _keys, L, R, r, 0, D, MATRIX)
    assert np.array_equal(got, want) and np.array_equal(kg, want_keys)
    for d_lo, d_hi in ((3, 12), (3, 4), (3, 10), (5, 20)):   # wave ranges 2/2/2/3, 0/0/0/1, 1/2/2/2, 3/4/4/4
        ws, olds = _ref_slice(env, ("const_slice", W, H, r, d_lo, d_hi), L, R, r, d_lo, d_hi)
        assert np.array_equal(olds, ws)
        ks = _with_n(env, n, _keys, L, R, r, d_lo, d_hi, MATRIX)
        assert np.array_equal(ks, ws), int((ks != ws).sum())


@pytest.mark.parametrize("n", WORKGROUPS)
@pytest.mark.parametrize("D,r", [(64, 5), (128, 5), (192, 5), (256, 5), (128, 7)])
def test_rows_of_carried_tiles(env, D, r, n):
    """m + 2 tiles and 7 columns in a row, two rows of tiles (H = 49): with 1, 2 or 3 workgroups a range carries the
    band over the whole row, starts mid-row, restages at the row end, and runs the masked right-edge tile last."""
    tox = 64 - 2 * r if r <= 6 else 48
    W, H = tox * (SLACK_TILES[D] + 2) + 7, 49
    L, R = _pair(env, 620 + r, W, H, 64)
    want, want_keys, old, old_keys = _ref(env, ("rows", D, r), L, R, r, D)
    assert np.array_equal(old, want) and np.array_equal(old_keys, want_keys)
    got = _with_n(env, n, _maps, L, R, r, D, MATRIX)
    assert np.array_equal(got, want), int((got != want).sum())
    kg = _with_n(env, n, _keys, L, R, r, 0, D, MATRIX)
    assert np.array_equal(kg, want_keys), int((kg != want_keys).sum())
    assert len(np.unique(got)) > 8


@pytest.mark.parametrize("n", WORKGROUPS)
def test_two_frames(env, n):
    """A 2-frame batch of 3 x 2 tiles: with 1, 2 or 3 workgroups a range passes from one frame to the next."""
    sm, torch, O, m = env
    W, H, D, r = 54 * 2 + 7, 49, 128, 5
    pairs = [_pair(env, 630 + f, W, H, 64) for f in range(2)]
    if "two" not in _refs:
        _refs["two"] = np.stack([O.box_disp(L, R, r, D) for L, R in pairs])
    Lt = torch.from_numpy(np.stack([p[0] for p in pairs])).cuda()
    Rt = torch.from_numpy(np.stack([p[1] for p in pairs])).cuda()
    res = {}
    for kernel in (LEGACY, MATRIX):
        m.set_box_kernel(kernel)
        m.set_box_workgroups(n)
        try:
            out = m.match_device(Lt, Rt, r, D)
            torch.cuda.synchronize()
        finally:
            m.set_box_kernel(0)
            m.set_box_workgroups(0)
        res[kernel] = out.cpu().numpy()
    assert np.array_equal(res[LEGACY], _refs["two"])
    assert np.array_equal(res[MATRIX], _refs["two"]), int((res[MATRIX] != _refs["two"]).sum())
