"""The matrix-pipe box kernel's stage 1 on permuted rows (bm_box_mfma.hip; SM_PARAM_BOX_KERNEL 2): a staged
column's 16-byte row groups hold the rows 32c + 4g + j and 32c + 16 + 4g + (j - 4), and each 16-row output block is one
MFMA on its 4-register view of a lane's eight AD registers against a single band.  Maps and slice keys bit-exact against
oracle.box_disp / box_keys_slice and against the VALU kernels (set_box_kernel(1)).  The shapes are the smallest at which
a wrong row order or a wrong view shows: a row-coded pair whose every window sum changes when two rows are swapped,
with the last image row in each of the three row blocks and both chunks; textured pairs through every staging path
(whole tile, carried band with guarded and with unguarded loads) and every launch form; the one-d-per-pass route with
its fourth row block; a pitched batch; a constant image."""
import ctypes

import numpy as np
import pytest

from test_gpu_box_mfma_pairs import LEGACY, MATRIX, _keys, _maps, _pair

pytestmark = pytest.mark.gpu
_WANT = {}


@pytest.fixture(scope="module")
def env():
    import torch
    import gpu_stereo_matching_amd as sm
    from oracle import oracle as O
    with sm.BlockMatcher(0, 400, 130, 256) as m:
        yield sm, torch, O, m


def _want(env, key, L, R, r, D):
    """The oracle's map and keys of one case, computed once."""
    if key not in _WANT:
        _WANT[key] = tuple(env[2].box_disp(L, R, r, D, want_keys=True))
    return _WANT[key]


def _with(env, n, q, fn, *args):
    m = env[3]
    m.set_box_workgroups(n)
    m.set_box_queue_workgroups(q)
    try:
        return fn(env, *args)
    finally:
        m.set_box_workgroups(0)
        m.set_box_queue_workgroups(0)


def _check(env, key, L, R, r, D, slices=(), forms=((0, 0),)):
    want, want_keys = _want(env, key, L, R, r, D)
    assert np.array_equal(_maps(env, L, R, r, D, LEGACY), want)
    for n, q in forms:
        got = _with(env, n, q, _maps, L, R, r, D, MATRIX)
        assert np.array_equal(got, want), (n, q, int((got != want).sum()))
        kg = _with(env, n, q, _keys, L, R, r, 0, D, MATRIX)
        assert np.array_equal(kg, want_keys), (n, q, int((kg != want_keys).sum()))
    for d_lo, d_hi in slices:
        ws = env[2].box_keys_slice(L, R, r, d_lo, d_hi)
        assert np.array_equal(_keys(env, L, R, r, d_lo, d_hi, LEGACY), ws), (d_lo, d_hi)
        for n, q in forms:
            ks = _with(env, n, q, _keys, L, R, r, d_lo, d_hi, MATRIX)
            assert np.array_equal(ks, ws), (n, q, d_lo, d_hi, int((ks != ws).sum()))
    return want, want_keys


def _row_coded(W, H, shift=0):
    """L[y, x] = (37 y + 11 (x & 3)) & 255, R = 0.  shift = 2: the same code modulo 64, mean 32: the keys are capped
    at the seed, 50 per window pixel (Device.cu:37), which hides most sums of the full-range code and few of these."""
    y, x = np.arange(H)[:, None], np.arange(W)[None, :]
    return ((37 * y + 11 * (x & 3)) & (255 >> shift)).astype(np.uint8), np.zeros((H, W), np.uint8)


def test_row_code_tells_rows_apart():
    """37 is odd: 37 y modulo 256 or 64 differs for any two of the 64 staged rows of a tile, so two swapped rows
    change every window sum that holds exactly one of them."""
    for shift in (0, 2):
        L, _ = _row_coded(120, 97, shift)
        for y0 in (0, 33):
            assert len(set(L[y0:y0 + 64, 0].tolist())) == 64


@pytest.mark.parametrize("shift", [0, 2])
@pytest.mark.parametrize("H", [7, 17, 33, 49, 64, 97])
@pytest.mark.parametrize("r", [1, 5, 7])
def test_row_coded_pair(env, r, H, shift):
    """W = 120, D = 40 (the paired loop at every radius).  H puts the last image row in each of the three row blocks and
    both chunks, with zero-staged rows above and below; 49, 64 and 97 add a cut last row of tiles."""
    L, R = _row_coded(120, H, shift)
    _, keys = _check(env, ("rows", r, H, shift), L, R, r, 40, slices=((3, 20),))
    if shift:
        seed = (50 * (2 * r + 1) ** 2) << 8
        assert (keys < seed).mean() > 0.75, "the cap at the seed hides the sums"


TEXTURED = [(260, 100, 128, 5), (200, 50, 64, 7), (330, 49, 192, 3), (400, 130, 256, 6)]


@pytest.mark.parametrize("W,H,D,r", TEXTURED)
def test_textured_pairs_every_launch_form(env, W, H, D, r):
    """One static range (every tile carried from its left neighbour along a row), three, auto, and two queue workgroups.
    400 x 130 at r = 6: the second row of tiles is interior (rows 42..105), so its carried tiles take the unguarded
    early loads and the kept band."""
    if (W, H) == (400, 130):
        assert 48 - r >= 0 and 48 - r + 64 <= H
    L, R = _pair(env, 700 + W, W, H, min(D, 64))
    want, _ = _check(env, ("tex", W, H, D, r), L, R, r, D, slices=((5, 5 + D // 2),),
                     forms=((1, 0), (3, 0), (0, 0), (0, 2)))
    assert len(np.unique(want)) > 8


@pytest.mark.parametrize("H", [63, 125])
@pytest.mark.parametrize("r", [1, 2])
def test_one_d_per_pass_fourth_row_block(env, r, H):
    """D = 32 at r <= 2: 62- / 60-row tiles, whose rows 48.. are the fourth row block (the third block's view against
    the band 16 rows up); 125 rows: two or three rows of tiles, the last one cut."""
    L, R = _pair(env, 720 + r, 200, H, 32)
    _check(env, ("np1", r, H), L, R, r, 32, slices=((3, 30),), forms=((0, 0), (2, 0)))
    Lc, Rc = _row_coded(200, H, 2)
    _check(env, ("np1rows", r, H), Lc, Rc, r, 32)


def test_pitched_guarded_batch(env):
    """3 frames of 260 x 100 inside larger tensors (pitch != W, frame stride != H * pitch), guard bytes around the
    outputs: nothing outside the output slices changes."""
    sm, torch, O, m = env
    from gpu_stereo_matching_amd import _capi
    W, H, D, r, B = 260, 100, 128, 5, 3
    PW, PH = W + 12, H + 3
    pairs = [_pair(env, 740 + f, W, H, 64) for f in range(B)]
    bigL = torch.zeros((B, PH, PW), dtype=torch.uint8, device="cuda")
    bigR = torch.zeros_like(bigL)
    for f, (L, R) in enumerate(pairs):
        bigL[f, 1:H + 1, 3:W + 3] = torch.from_numpy(L).cuda()
        bigR[f, 1:H + 1, 3:W + 3] = torch.from_numpy(R).cuda()
    for q in (0, 2):
        out = torch.full((B, PH, PW), 0xAB, dtype=torch.uint8, device="cuda")
        m.set_box_kernel(MATRIX)
        m.set_box_queue_workgroups(q)
        try:
            _capi.check(m._lib.sm_match_device(
                m._h, bigL[0, 1:, 3:].data_ptr(), bigR[0, 1:, 3:].data_ptr(), W, H, PW, B, PH * PW, r, D, 0,
                out[0, 1:, 3:].data_ptr(), PW, PH * PW, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)))
            torch.cuda.synchronize()
        finally:
            m.set_box_kernel(0)
            m.set_box_queue_workgroups(0)
        res = out.cpu().numpy()
        for f, (L, R) in enumerate(pairs):
            want, _ = _want(env, ("pitched", f), L, R, r, D)
            assert np.array_equal(res[f, 1:H + 1, 3:W + 3], want), (q, f)
        res[:, 1:H + 1, 3:W + 3] = 0xAB
        assert (res == 0xAB).all(), "wrote outside the output slices"


def test_constant_image_ties_to_the_smaller_d(env):
    """Every d ties at cost 0: the smaller d wins, within a pair, across the waves and in a slice with d_lo > 0."""
    W, H, r = 120, 50, 5
    L = np.full((H, W), 91, np.uint8)
    want, keys = _check(env, ("const",), L, L.copy(), r, 40, slices=((3, 20),))
    assert not want.any() and (keys[:, :W] == 0).all()
    ks = _keys(env, L, L.copy(), r, 3, 20, MATRIX)
    assert (ks[:, :W - 3] == 3).all()
