"""The matrix-pipe box kernel drawing runs of tiles from a queue (bm_box_mfma.hip, bm_box_plan.h's box_queue_grab,
DESIGN §30; SM_PARAM_BOX_QUEUE_WORKGROUPS) against oracle.box_disp / box_keys_slice and against the static ranges of
the same handle with SM_PARAM_BOX_WORKGROUPS = T (one tile per workgroup): maps and slice keys bit for bit.  Every
frame here has a dozen tiles at most, far fewer than the GPU has workgroup slots, so only an explicit number of queue
workgroups makes the launch draw from the counter: 1 (one workgroup draws every grab, the shrinking tail included),
2 and 5 (several grabs each, who draws what is up to the hardware), and more than there are tiles (workgroups that
draw nothing).  Frames are at most 200 x 100; the oracle's answer for a shape is computed once."""
import ctypes

import numpy as np
import pytest

from test_gpu_box_mfma_pairs import LEGACY, MATRIX, _keys, _maps, _pair, env  # noqa: F401

pytestmark = pytest.mark.gpu

_WANT = {}


def _tiles(W, H, r, batch=1):
    tox = 64 - 2 * r if r <= 6 else 48
    return -(-W // tox), -(-H // 48), -(-W // tox) * -(-H // 48) * batch


def _qs(T):
    return (1, 2, 5, T + 3)


def _shape(env, seed, W, H, r, D):
    """(L, R, the oracle's map, the oracle's keys) of one shape, computed once."""
    key = (seed, W, H, r, D)
    if key not in _WANT:
        L, R = _pair(env, seed, W, H, min(D, 64))
        _WANT[key] = (L, R) + tuple(env[2].box_disp(L, R, r, D, want_keys=True))
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


def _check_every_q(env, seed, W, H, r, D):
    L, R, want, want_keys = _shape(env, seed, W, H, r, D)
    T = _tiles(W, H, r)[2]
    static = _with(env, T, 0, _maps, L, R, r, D, MATRIX), _with(env, T, 0, _keys, L, R, r, 0, D, MATRIX)
    assert np.array_equal(static[0], want) and np.array_equal(static[1], want_keys)
    for q in _qs(T):
        got = _with(env, 0, q, _maps, L, R, r, D, MATRIX)
        assert np.array_equal(got, want), (q, int((got != want).sum()))
        assert np.array_equal(got, static[0]), q
        kg = _with(env, 0, q, _keys, L, R, r, 0, D, MATRIX)
        assert np.array_equal(kg, want_keys), (q, int((kg != want_keys).sum()))
        assert np.array_equal(kg, static[1]), q


@pytest.mark.parametrize("W,H,grid", [(200, 100, (4, 3)), (120, 50, (3, 2)), (55, 49, (2, 2))])
def test_frames_at_r5(env, W, H, grid):
    """r = 5, D = 40: 4 x 3 tiles; 120 x 50 and 55 x 49, whose last tiles start a few columns and rows before the
    frame ends (55 = 54 + 1 and 49 = 48 + 1: one column and one row past a tile)."""
    assert _tiles(W, H, 5)[:2] == grid
    _check_every_q(env, 400 + W, W, H, 5, 40)


@pytest.mark.parametrize("r,D", [(5, 9), (5, 16), (1, 16), (7, 16)])
def test_radius_and_disparities(env, r, D):
    """200 x 100.  D = 9 and 16 at r = 5: waves with 2 / 3 and 4 disparities; r = 7: 48-column tiles in three blocks;
    r = 1 at D = 16 is one d per pass, which keeps its one-tile kernel whatever the queue parameter says."""
    _check_every_q(env, 410 + r, 200, 100, r, D)


@pytest.mark.parametrize("q", [1, 2, 5, 40])
def test_batch_of_three_pitched(env, q):
    """120 x 50 inside 130 x 52, 3 frames (T = 18; q = 40 is more workgroups than tiles), a frame stride that is not
    H x pitch, guard bytes 0xAB: runs cross frames, and nothing outside the output slices is written."""
    sm, torch, O, m = env
    from gpu_stereo_matching_amd import _capi
    W, H, D, r, B = 120, 50, 40, 5, 3
    PW, PH = W + 10, H + 2
    shapes = [_shape(env, 420 + f, W, H, r, D) for f in range(B)]
    bigL = torch.zeros((B, PH, PW), dtype=torch.uint8, device="cuda")
    bigR = torch.zeros_like(bigL)
    for f, (L, R, _, _) in enumerate(shapes):
        bigL[f, 1:H + 1, 3:W + 3] = torch.from_numpy(L).cuda()
        bigR[f, 1:H + 1, 3:W + 3] = torch.from_numpy(R).cuda()
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
    for f, (_, _, want, _) in enumerate(shapes):
        assert np.array_equal(res[f, 1:H + 1, 3:W + 3], want), f
    res[:, 1:H + 1, 3:W + 3] = 0xAB
    assert (res == 0xAB).all(), "wrote outside the output slices"


def _launch(torch, m, Lt, Rt, r, D):
    return m.match_device(Lt, Rt, r, D)


def test_three_launches_in_a_row(env):
    """The same handle three times on one stream without a synchronise between: each launch starts from a counter
    that the launcher has zeroed behind the launch before."""
    sm, torch, O, m = env
    L, R, want, _ = _shape(env, 600, 200, 100, 5, 40)
    Lt, Rt = torch.from_numpy(L).cuda(), torch.from_numpy(R).cuda()
    m.set_box_kernel(MATRIX)
    m.set_box_queue_workgroups(2)
    try:
        outs = [_launch(torch, m, Lt, Rt, 5, 40) for _ in range(3)]
        torch.cuda.synchronize()
    finally:
        m.set_box_kernel(0)
        m.set_box_queue_workgroups(0)
    for i, o in enumerate(outs):
        assert np.array_equal(o.cpu().numpy(), want), i


def test_two_handles_alternating(env):
    """Two handles, each with its own counter, alternating on one stream, on two shapes."""
    sm, torch, O, m = env
    a = _shape(env, 600, 200, 100, 5, 40)
    b = _shape(env, 520, 120, 50, 5, 40)
    with sm.BlockMatcher(0, 320, 100, 256) as m2:
        ms = (m, m2)
        for h in ms:
            h.set_box_kernel(MATRIX)
        m.set_box_queue_workgroups(2)
        m2.set_box_queue_workgroups(5)
        try:
            dev = [(torch.from_numpy(s[0]).cuda(), torch.from_numpy(s[1]).cuda(), s[2]) for s in (a, b)]
            outs = []
            for i in range(6):
                Lt, Rt, want = dev[(i // 2) % 2]
                outs.append((_launch(torch, ms[i % 2], Lt, Rt, 5, 40), want))
            torch.cuda.synchronize()
        finally:
            for h in ms:
                h.set_box_kernel(0)
                h.set_box_queue_workgroups(0)
        for i, (o, want) in enumerate(outs):
            assert np.array_equal(o.cpu().numpy(), want), i


@pytest.mark.parametrize("d_lo,d_hi", [(7, 40), (20, 61)])
def test_d_slice_with_keys(env, d_lo, d_hi):
    """Slices with d_lo > 0 on 200 x 100 at r = 5: the keys of the slice against the oracle and the static ranges."""
    L, R, _, _ = _shape(env, 600, 200, 100, 5, 40)
    key = ("slice", d_lo, d_hi)
    if key not in _WANT:
        _WANT[key] = env[2].box_keys_slice(L, R, 5, d_lo, d_hi)
    want = _WANT[key]
    T = _tiles(200, 100, 5)[2]
    static = _with(env, T, 0, _keys, L, R, 5, d_lo, d_hi, MATRIX)
    assert np.array_equal(static, want)
    for q in _qs(T):
        k = _with(env, 0, q, _keys, L, R, 5, d_lo, d_hi, MATRIX)
        assert np.array_equal(k, want), (q, int((k != want).sum()))


def test_parameter_values(env):
    sm, torch, O, m = env
    from gpu_stereo_matching_amd import _capi
    for bad in (-1, 1.5, float("nan"), 2 ** 20 + 1):
        with pytest.raises(_capi.SMError) as e:
            m.set_box_queue_workgroups(bad)
        assert e.value.code == _capi.SM_ERR_INVALID_ARG
    # an explicit range count keeps the static ranges whatever the queue parameter says, and the VALU kernels ignore it
    L, R, want, _ = _shape(env, 600, 200, 100, 5, 40)
    assert np.array_equal(_with(env, 3, 5, _maps, L, R, 5, 40, MATRIX), want)
    assert np.array_equal(_with(env, 0, 5, _maps, L, R, 5, 40, LEGACY), want)
