"""The matrix-pipe box kernel's left-edge rule (bm_box_mfma.hip; SM_PARAM_BOX_KERNEL 2): a tile's d
range ends one disparity past max(x_max + R + 1, d_lo).  Maps against oracle.box_disp and slice keys against
oracle.box_keys_slice, bit for bit, and maps against the VALU kernels (SM_PARAM_BOX_KERNEL 1) on the same handle, in
the kernel's three launch forms: one tile per workgroup, static ranges of tiles (two workgroups, so that runs along a
row of tiles carry the band and cross rows and frames), and the queue (two workgroups drawing runs).  The shapes,
pairs and slices are the table of test_box_mfma_left_rule_model.py, which asserts that every case of the rule occurs
in it, plus 60-row frames for a second row of tiles; 2 or 3 frames per call.  The oracle's answers are computed once
and shared by the three forms."""
import numpy as np
import pytest

from test_box_mfma_left_rule_model import (DS, HS, KINDS, RS, WS, cases_of, geometry, pair, slices_of, tile_d_end,
                                           tiles)
from test_gpu_box_mfma_pairs import LEGACY, MATRIX, env  # noqa: F401  (env is the fixture)

pytestmark = pytest.mark.gpu

FORMS = ("tile", "ranges", "queue")
HS_GPU = HS + (60,)          # 48-row tiles: one row of tiles, and two
_WANT = {}


def _frames(H):
    return 2 if H == 40 else 3


def _batch(kind, W, H, r):
    """(L [B, H, W], R, the oracle's maps per D, the oracle's keys of frame 0 per D), computed once."""
    key = (kind, W, H, r)
    if key not in _WANT:
        from oracle import oracle as O
        B = _frames(H)
        Ls, Rs = zip(*[pair(kind, W, H, 3000 * W + 100 * r + 10 * H + f) for f in range(B)])
        maps = {D: np.stack([O.box_disp(Ls[f], Rs[f], r, D) for f in range(B)]) for D in DS}
        keys = {D: O.box_disp(Ls[0], Rs[0], r, D, want_keys=True)[1] for D in DS}
        _WANT[key] = np.stack(Ls), np.stack(Rs), maps, keys
    return _WANT[key]


def _slice_want(kind, W, r, d_lo, d_hi):
    key = ("slice", kind, W, r, d_lo, d_hi)
    if key not in _WANT:
        from oracle import oracle as O
        L, R = _batch(kind, W, HS[0], r)[:2]
        _WANT[key] = O.box_keys_slice(L[0], R[0], r, d_lo, d_hi)
    return _WANT[key]


class _Form:
    """The handle forced to the matrix kernel in one launch form (or to the VALU kernels), restored on exit."""

    def __init__(self, m, form):
        self.m, self.form = m, form

    def __enter__(self):
        m = self.m
        m.set_box_kernel(LEGACY if self.form == "valu" else MATRIX)
        if self.form == "tile":
            m.set_box_workgroups(1 << 20)      # at most one per tile: one tile per workgroup
        elif self.form == "ranges":
            m.set_box_workgroups(2)
        elif self.form == "queue":
            m.set_box_queue_workgroups(2)
        return m

    def __exit__(self, *exc):
        self.m.set_box_kernel(0)
        self.m.set_box_workgroups(0)
        self.m.set_box_queue_workgroups(0)


def _maps(env, form, Lt, Rt, r, D):
    torch, m = env[1], env[3]
    with _Form(m, form):
        out = m.match_device(Lt, Rt, r, D)
        torch.cuda.synchronize()
    return out.cpu().numpy()


def _keys(env, form, Lt, Rt, r, d_lo, d_hi):
    torch, m = env[1], env[3]
    with _Form(m, form):
        k = m.slice_keys_device(Lt, Rt, r, d_lo, d_hi)
        torch.cuda.synchronize()
    return k.cpu().numpy().view(np.uint32)


def _cut(W, r, d_lo, d_hi):
    return any(tile_d_end(W, r, d_lo, d_hi, x0) < tile_d_end(W, r, d_lo, d_hi, x0, False)
               for x0, _ in tiles(W, r, d_lo, d_hi))


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("W", WS)
@pytest.mark.parametrize("form", FORMS)
def test_maps_and_keys(env, form, W, kind):
    """Every (r, D, H) of the table at this width: 2 to 5 tiles wide, one or two rows of tiles, 2 or 3 frames."""
    torch = env[1]
    for r in RS:
        assert 2 <= len(tiles(W, r, 0, 128)) <= 5
        for H in HS_GPU:
            L, R, maps, keys = _batch(kind, W, H, r)
            Lt, Rt = torch.from_numpy(L).cuda(), torch.from_numpy(R).cuda()
            for D in DS:
                got = _maps(env, form, Lt, Rt, r, D)
                assert np.array_equal(got, maps[D]), (r, H, D, int((got != maps[D]).sum()))
                assert np.array_equal(got, _maps(env, "valu", Lt, Rt, r, D)), (r, H, D)
                kg = _keys(env, form, Lt[0], Rt[0], r, 0, D)
                assert np.array_equal(kg, keys[D]), (r, H, D, int((kg != keys[D]).sum()))


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("W", WS)
@pytest.mark.parametrize("form", FORMS)
def test_slices(env, form, W, kind):
    """The d-slices around the left bound of the first two tiles (below it, on it, past it, where exactly one pass
    runs; odd and even lengths; at r = 1 the short ones run one d per pass)."""
    torch = env[1]
    for r in RS:
        L, R = _batch(kind, W, HS[0], r)[:2]
        Lt, Rt = torch.from_numpy(L[0]).cuda(), torch.from_numpy(R[0]).cuda()
        for d_lo, d_hi in slices_of(W, r):
            want = _slice_want(kind, W, r, d_lo, d_hi)
            got = _keys(env, form, Lt, Rt, r, d_lo, d_hi)
            assert np.array_equal(got, want), (r, d_lo, d_hi, int((got != want).sum()))


@pytest.mark.parametrize("r", [1, 2])
@pytest.mark.parametrize("form", FORMS)
def test_one_d_per_pass(env, form, r):
    """D = 32 at r <= 2 is the NP = 1 loop on 64 - 2r columns: its one-tile kernel (tile, and queue, which it
    ignores) and its walking kernel (ranges).  From d_lo = 0 a range of 32 ends before the first tile's bound of
    64 - r, so the rule shows in the slices: one that ends behind the bound, one that begins on it, one past it."""
    torch, O = env[1], env[2]
    W, H, D = 140, 40, 32
    assert geometry(r, 0, D) == (1, 64 - 2 * r) and not _cut(W, r, 0, D)
    L, R = zip(*[pair("flat_left", W, H, 77 + r + f) for f in range(2)])
    Lt, Rt = torch.from_numpy(np.stack(L)).cuda(), torch.from_numpy(np.stack(R)).cuda()
    want = np.stack([O.box_disp(L[f], R[f], r, D) for f in range(2)])
    got = _maps(env, form, Lt, Rt, r, D)
    assert np.array_equal(got, want) and np.array_equal(got, _maps(env, "valu", Lt, Rt, r, D))
    b = 64 - r
    names = set()
    for d_lo, d_hi in [(b - 10, b + 22), (b - 9, b + 23), (b, b + 32), (b + 5, b + 36)]:
        assert geometry(r, d_lo, d_hi)[0] == 1
        names |= cases_of(W, r, d_lo, d_hi)
        kw = O.box_keys_slice(L[0], R[0], r, d_lo, d_hi)
        kg = _keys(env, form, Lt[0], Rt[0], r, d_lo, d_hi)
        assert np.array_equal(kg, kw), (d_lo, d_hi, int((kg != kw).sum()))
    assert {"cut", "d_lo < bound", "d_lo = bound", "d_lo > bound", "odd length", "even length"} <= names, names


@pytest.mark.parametrize("form", FORMS)
def test_seed_and_threshold(env, form):
    """match_device runs with the seed key and the threshold of Device.cu (50 per window pixel): on a pair of
    unrelated full-range frames nearly every real cost is above it, so the map is 0 there, while the left strip's
    zero-cost disparities x + r + 1 stay below it and must survive the cut range."""
    torch, O = env[1], env[2]
    W, H, r, D = 140, 40, 5, 128
    assert _cut(W, r, 0, D)
    rng = np.random.default_rng(5)
    L = rng.integers(0, 256, (2, H, W), dtype=np.uint8) | 1
    R = rng.integers(0, 256, (2, H, W), dtype=np.uint8) & 0xFE
    want = np.stack([O.box_disp(L[f], R[f], r, D) for f in range(2)])
    xs = np.arange(40)
    assert (want[:, :, xs] == xs + r + 1).all() and (want[:, :, D:W - r] == 0).mean() > 0.8
    Lt, Rt = torch.from_numpy(L).cuda(), torch.from_numpy(R).cuda()
    got = _maps(env, form, Lt, Rt, r, D)
    assert np.array_equal(got, want), int((got != want).sum())
    assert np.array_equal(got, _maps(env, "valu", Lt, Rt, r, D))
