"""The matrix-pipe box kernel's unmasked paired loop in its overlapped order (bm_box_mfma.hip): every
MFMA issues between vector work of its own wave, the next column block's operands are read ahead, and the mins of one
row block are carried into the next column block.  The arithmetic is unchanged, so maps and slice keys must equal
oracle.box_disp / box_keys_slice and the VALU kernels (set_box_kernel(1)) bit for bit.  The shapes are the smallest at
which a reordered pass can go wrong: all four column blocks and the three of r = 7, every d_max instantiation, tiles
whose passes are unmasked, masked and mixed, a cut last row and column; d-slices of 1..9 disparities from an odd d_lo
(wave ranges 0..3 long, pairs that end on a repeated d); a constant image (every d ties: the smaller d must win, also
within a pair); and 1, 3 and auto workgroups (carried, restaged and auto tiles).  The references of a shape are
computed once and shared."""
import numpy as np
import pytest

from test_gpu_box_mfma_pairs import LEGACY, MATRIX, _keys, _maps, _pair

pytestmark = pytest.mark.gpu

SHAPES = [(260, 100, 128, 5), (200, 50, 64, 7), (200, 50, 64, 1), (330, 49, 192, 3), (400, 97, 256, 6)]
WORKGROUPS = (1, 3, 0)
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


@pytest.mark.parametrize("n", WORKGROUPS)
@pytest.mark.parametrize("W,H,D,r", SHAPES)
def test_shapes(env, W, H, D, r, n):
    L, R = _pair(env, 500 + r, W, H, min(D, 64))
    want, want_keys, old, old_keys = _ref(env, ("full", W, H, D, r), L, R, r, D)
    assert np.array_equal(old, want) and np.array_equal(old_keys, want_keys)
    got = _with_n(env, n, _maps, L, R, r, D, MATRIX)
    assert np.array_equal(got, want), int((got != want).sum())
    kg = _with_n(env, n, _keys, L, R, r, 0, D, MATRIX)
    assert np.array_equal(kg, want_keys), int((kg != want_keys).sum())
    assert np.array_equal(kg, old_keys)
    assert len(np.unique(got)) > 8    # a textured pair: the map is not all threshold zeros


@pytest.mark.parametrize("n", WORKGROUPS)
@pytest.mark.parametrize("nd", range(1, 10))
@pytest.mark.parametrize("W,H,r,d_lo", [(260, 100, 5, 37), (200, 50, 7, 21)])
def test_short_slices_from_an_odd_d_lo(env, W, H, r, d_lo, nd, n):
    """nd = 1..9 disparities over four waves: ranges of 0..3, odd ranges end on their last d twice."""
    L, R = _pair(env, 500 + r, W, H, 64)
    want, old = _ref_slice(env, ("slice", W, H, r, d_lo, nd), L, R, r, d_lo, d_lo + nd)
    assert np.array_equal(old, want)
    got = _with_n(env, n, _keys, L, R, r, d_lo, d_lo + nd, MATRIX)
    assert np.array_equal(got, want), int((got != want).sum())


@pytest.mark.parametrize("n", WORKGROUPS)
@pytest.mark.parametrize("W,H,D,r", SHAPES[:2])
def test_constant_image_ties_go_to_the_smaller_d(env, W, H, D, r, n):
    """L = R = 77: the cost of every valid d is 0 at every pixel, so every key is d = 0's and the map is 0."""
    L = np.full((H, W), 77, np.uint8)
    R = L.copy()
    want, want_keys, old, old_keys = _ref(env, ("const", W, H, D, r), L, R, r, D)
    assert np.array_equal(old, want) and np.array_equal(old_keys, want_keys)
    assert not want.any() and not (want_keys & 0xFF).any()
    got = _with_n(env, n, _maps, L, R, r, D, MATRIX)
    kg = _with_n(env, n, _keys, L, R, r, 0, D, MATRIX)
    assert np.array_equal(got, want) and np.array_equal(kg, want_keys)
    # a slice from d_lo = 3: the tie now goes to 3, the first d of a pair or, for the odd-length range, its last
    for d_lo, d_hi in ((3, 12), (3, 4)):
        ws, olds = _ref_slice(env, ("const_slice", W, H, r, d_lo, d_hi), L, R, r, d_lo, d_hi)
        assert np.array_equal(olds, ws)
        ks = _with_n(env, n, _keys, L, R, r, d_lo, d_hi, MATRIX)
        assert np.array_equal(ks, ws), int((ks != ws).sum())
