"""The matrix-pipe box kernel's masked passes in the paired loop's slot order, with its carried values (bm_box_mfma.hip,
DESIGN §27), against oracle.box_disp / box_keys_slice and against the VALU kernels forced with set_box_kernel(1): maps
and slice keys bit for bit, with the harness of test_gpu_box_mfma_pairs.py.  One body now walks a wave's unmasked
passes and then its masked ones and hands the key constants, the R addresses and the mask scalars from one to the
other, so the shapes are those where that can go wrong: odd masked ranges (the repeated disparity labelled d + 1),
waves that run both loops, waves that are masked throughout, both masks in the same pass, the label's carry at
d = 255, three column blocks (r = 7), d_lo > 0.  Frames are 50 rows high; every shape runs at auto n and with one
and three workgroups, which walk rows of tiles with a carried band and the staging loads issued after both loops.
Each test first asserts from the model (test_box_mfma_masked_order_model.py) that its shape hits its case."""
import numpy as np
import pytest

from test_box_mfma_masked_order_model import shape_stats
from test_gpu_box_mfma_pairs import LEGACY, MATRIX, _check, _check_slice, _keys, _maps, _pair, env  # noqa: F401

pytestmark = pytest.mark.gpu
H = 50
NS = (1, 3)


def _with_n(env, n, fn, *args):
    m = env[3]
    m.set_box_workgroups(n)
    try:
        return fn(env, *args)
    finally:
        m.set_box_workgroups(0)


def _check_all_n(env, L, R, r, D):
    got, kg = _check(env, L, R, r, D)                  # oracle, VALU kernels, matrix kernel at auto n
    for n in NS:
        a = _with_n(env, n, _maps, L, R, r, D, MATRIX)
        assert np.array_equal(a, got), (n, int((a != got).sum()))
        k = _with_n(env, n, _keys, L, R, r, 0, D, MATRIX)
        assert np.array_equal(k, kg), (n, int((k != kg).sum()))
    return got


def _check_slice_all_n(env, L, R, r, d_lo, d_hi):
    got = _check_slice(env, L, R, r, d_lo, d_hi)       # oracle, VALU kernels, matrix kernel at auto n
    for n in NS:
        k = _with_n(env, n, _keys, L, R, r, d_lo, d_hi, MATRIX)
        assert np.array_equal(k, got), (n, int((k != got).sum()))
    return got


def test_headline_geometry_most_passes_masked(env):
    """230 x 50, r = 5, D = 128: 168 of 235 passes masked, 7 waves with an odd masked range, 4 that run both loops."""
    s = shape_stats(230, 5, 0, 128)
    assert (s["masked"], s["passes"], s["odd_masked"], s["handovers"]) == (168, 235, 7, 4)
    L, R = _pair(env, 501, 230, H, 64)
    got = _check_all_n(env, L, R, 5, 128)
    assert len(np.unique(got)) > 8


def test_same_frame_as_slice_from_one(env):
    """The same frame as slice [1, 128): 10 odd masked ranges, 5 hand-overs."""
    s = shape_stats(230, 5, 1, 128)
    assert (s["odd_masked"], s["handovers"]) == (10, 5)
    L, R = _pair(env, 501, 230, H, 64)
    _check_slice_all_n(env, L, R, 5, 1, 128)


def test_label_carry_at_255(env):
    """262 x 50, r = 5, slice [4, 256): the tile at x0 = 0, wave 3, runs [193, 256) wholly masked and odd; its last
    pass is the single disparity 255, whose repeat is labelled 256: the carry reaches the cost."""
    s = shape_stats(262, 5, 4, 256)
    assert (0, 3, 193, 193, 256) in s["waves"]
    L, R = _pair(env, 502, 262, H, 64)
    _check_slice_all_n(env, L, R, 5, 4, 256)
    # constant frames: every cost ties, so at columns right of 255 the key of d = 255 would win wherever the repeat's
    # label were taken for a smaller d; the smallest d wins
    C = np.full((H, 262), 90, np.uint8)
    k = _check_slice_all_n(env, C, C.copy(), 5, 4, 256)
    assert (k[:, :262 - 4] == 4).all()


def test_narrow_frame_every_pass_masked(env):
    """80 x 50, r = 5, D = 128: both masks in the same passes, a tile that reaches past W, every pass masked, no
    hand-over."""
    s = shape_stats(80, 5, 0, 128)
    assert s["masked"] == s["passes"] > 0 and s["handovers"] == 0 and s["all_masked"] > 0
    assert 54 - 5 + 64 > 80                            # the second tile's staged columns reach past W
    L, R = _pair(env, 503, 80, H, 64)
    _check_all_n(env, L, R, 5, 128)


@pytest.mark.parametrize("W,d_lo,d_hi", [(159, 0, 128), (217, 1, 256)])
def test_three_column_blocks(env, W, d_lo, d_hi):
    """r = 7: three column blocks, the address step in the stage-1 path of the last one.  Both shapes have unmasked
    and masked passes and hand-overs, the slice odd masked ranges as well."""
    s = shape_stats(W, 7, d_lo, d_hi)
    assert 0 < s["masked"] < s["passes"] and s["handovers"] > 0 and s["all_masked"] > 0
    assert d_lo == 0 or s["odd_masked"] > 0
    L, R = _pair(env, 504 + W, W, H, 64)
    if d_lo == 0:
        _check_all_n(env, L, R, 7, d_hi)
    else:
        _check_slice_all_n(env, L, R, 7, d_lo, d_hi)


def test_slice_with_d_lo(env):
    """230 x 50, r = 5, slice [40, 90): d_lo > 0, 9 odd masked ranges, 3 hand-overs."""
    s = shape_stats(230, 5, 40, 90)
    assert (s["odd_masked"], s["handovers"]) == (9, 3)
    L, R = _pair(env, 505, 230, H, 64)
    _check_slice_all_n(env, L, R, 5, 40, 90)


def test_batch_of_two_in_one_workgroup(env):
    """Two 230 x 50 frames at n = 1: one workgroup crosses every row and frame with both loops."""
    sm, torch, O, m = env
    W, r, D = 230, 5, 128
    assert shape_stats(W, r, 0, D)["handovers"] > 0
    pairs = [_pair(env, 510 + f, W, H, 64) for f in range(2)]
    Ls, Rs = np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])
    want = np.stack([O.box_disp(L, R, r, D) for L, R in pairs])
    for kernel, n in ((LEGACY, 0), (MATRIX, 0), (MATRIX, 1)):
        m.set_box_kernel(kernel)
        m.set_box_workgroups(n)
        try:
            out = m.match_device(torch.from_numpy(Ls).cuda(), torch.from_numpy(Rs).cuda(), r, D)
            torch.cuda.synchronize()
        finally:
            m.set_box_kernel(0)
            m.set_box_workgroups(0)
        got = out.cpu().numpy()
        assert np.array_equal(got, want), (kernel, n, [int((got[f] != want[f]).sum()) for f in range(2)])
