"""GPU parity for the launch geometry the plan headers hold (bm_strip_plan.h's bands, the cached occupancy query of
bm_common.h): a strip launch of more workgroups than the device holds at once, and a strip and a matrix-pipe call
repeated on one handle, the second through the cache.  Every map equals the oracle's getDisp bit for bit."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def matcher():
    import gpu_stereo_matching_amd as sm
    m = sm.BlockMatcher(0, 128, 64, 256)
    yield m
    m.close()


def test_strip_more_workgroups_than_resident(matcher, oracle):
    """9000 frames of 8 x 3 at r = 16, D = 5: one edge strip in one band per frame, 9000 workgroups, past the 16 waves
    per CU x 256 CUs = 4096 the device holds at most: the bands' (1, 1) fallback, whatever the occupancy query
    answers.  Three distinct pairs, cycled."""
    import torch
    pairs = [oracle.synth_pair(9100 + i, 8, 3, 16) for i in range(3)]
    want = [oracle.box_disp(L, R, 16, 5) for L, R in pairs]
    Lt = torch.from_numpy(np.stack([p[0] for p in pairs])).cuda().repeat(3000, 1, 1)
    Rt = torch.from_numpy(np.stack([p[1] for p in pairs])).cuda().repeat(3000, 1, 1)
    assert Lt.shape == (9000, 3, 8)
    out = matcher.match_device(Lt, Rt, 16, 5)
    torch.cuda.synchronize()
    got = out.cpu().numpy().reshape(3000, 3, 3, 8)
    for i in range(3):
        assert np.array_equal(got[:, i], np.broadcast_to(want[i], (3000, 3, 8))), i


def test_repeated_calls_through_the_occupancy_cache(matcher, oracle):
    """A strip call and a forced matrix-pipe call (r = 3, D = 16, 128 x 64), each twice on one handle: the second of
    each finds the resident workgroups cached."""
    L, R = oracle.synth_pair(9200, 128, 64, 16)
    want_strip, want_matrix = oracle.box_disp(L, R, 16, 16), oracle.box_disp(L, R, 3, 16)
    matcher.set_box_kernel(2)
    try:
        for _ in range(2):
            assert np.array_equal(matcher.match(L, R, 16, 16), want_strip)
            assert np.array_equal(matcher.match(L, R, 3, 16), want_matrix)
    finally:
        matcher.set_box_kernel(0)
