"""GPU segment-tree stereo (STMatching ST-1 and ST-2) against the C restatement
(oracle/st_oracle.c), bit for bit: the cost, the tree and the filter's float operations are done in
the reference's order, so the maps are identical, not merely close."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def matcher():
    import gpu_stereo_matching_amd as sm
    m = sm.BlockMatcher(0, 640, 480, 256)
    yield m
    m.close()


def test_art_reference_defaults(matcher, oracle):
    """The bundled Art pair at the app's defaults (max level 60, scale 4, sigma 0.1: main.cpp:49-51)."""
    g = np.load(os.path.join(GOLDEN, "middlebury_bgr.npz"))
    L, R = g["Art/view1"], g["Art/view5"]
    want, levels = oracle.st_disp(L, R, 60, 4, 0.1)
    got = matcher.segment_tree(L, R)
    assert np.array_equal(got, want), int((got != want).sum())
    tree_ms, total_ms, lv = matcher.segment_tree_stats()
    assert lv == levels and 0 < tree_ms < total_ms


@pytest.mark.parametrize("W,H,D,scale,sigma,seed", [(97, 61, 16, 1, 0.1, 1), (2, 5, 3, 4, 0.1, 2),
                                                     (300, 200, 64, 2, 0.08, 3), (123, 1, 9, 3, 0.5, 4),
                                                     (64, 48, 80, 3, 0.005, 5)])
def test_random_pairs(matcher, oracle, W, H, D, scale, sigma, seed):
    """Textured and flat random BGR pairs (a right view shifted by a known disparity, plus flat
    patches that produce long equal-weight edge runs), odd sizes, a 1-row frame, sigma below the
    reference's 0.01 clamp."""
    rng = np.random.default_rng(seed)
    L = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    L[: H // 2, : W // 3] = 77
    R = np.roll(L, -min(5, W - 1), axis=1)
    R[:, -3:] = rng.integers(0, 256, (H, min(3, W), 3), dtype=np.uint8)
    want, _ = oracle.st_disp(L, R, D, scale, sigma)
    got = matcher.segment_tree(L, R, D, scale, sigma)
    assert np.array_equal(got, want), int((got != want).sum())


def test_argument_errors(matcher):
    import gpu_stereo_matching_amd as sm
    a = np.zeros((4, 1, 3), np.uint8)
    with pytest.raises(sm.SMError):
        matcher.segment_tree(a, a)                       # width 1: the gradient needs two columns
    b = np.zeros((4, 4, 3), np.uint8)
    with pytest.raises(sm.SMError):
        matcher.segment_tree(b, b, 0)
    with pytest.raises(sm.SMError):
        matcher.segment_tree(b, b, 8, 4, 0.0)


def test_st2_art_reference_defaults(matcher, oracle):
    """ST-2 (main.cpp's method 1, stereo_disparity_iteration) on the bundled Art pair at the defaults."""
    g = np.load(os.path.join(GOLDEN, "middlebury_bgr.npz"))
    L, R = g["Art/view1"], g["Art/view5"]
    want, levels, _, _, _ = oracle.st2_disp(L, R, 60, 4, 0.1)
    got = matcher.segment_tree(L, R, method=1)
    assert np.array_equal(got, want), int((got != want).sum())
    tree_ms, total_ms, lv = matcher.segment_tree_stats()
    assert lv == levels and 0 < tree_ms < total_ms
    # ST-1 still answers after an ST-2 call on the same handle (shared workspace)
    want1, _ = oracle.st_disp(L, R, 60, 4, 0.1)
    assert np.array_equal(matcher.segment_tree(L, R), want1)


@pytest.mark.parametrize("W,H,D,scale,sigma,seed", [(97, 61, 16, 1, 0.1, 11), (2, 5, 3, 4, 0.1, 12),
                                                     (300, 200, 64, 2, 0.08, 13), (123, 1, 9, 3, 0.5, 14),
                                                     (40, 30, 60, 4, 0.1, 15), (64, 48, 80, 3, 0.005, 16)])
def test_st2_random_pairs(matcher, oracle, W, H, D, scale, sigma, seed):
    """ST-2 on textured / flat random pairs: a 2-pixel-wide and a 1-row frame, sigma below the 0.01 clamp,
    and W < D (40 x 30 at D = 60, 2 x 5 at D = 3).  For W < D the reference's
    GetRightMatchingCostFromLeft starts at the negative column w - maxLevel (StereoHelper.cpp:168),
    undefined behaviour; the oracle and the GPU use the in-bounds reading (start at 0), so those
    cases are parity unpinned and check only that the GPU equals that defined extension."""
    rng = np.random.default_rng(seed)
    L = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    L[: H // 2, : W // 3] = 77
    R = np.roll(L, -min(5, W - 1), axis=1)
    R[:, -3:] = rng.integers(0, 256, (H, min(3, W), 3), dtype=np.uint8)
    want, _, _, _, _ = oracle.st2_disp(L, R, D, scale, sigma)
    got = matcher.segment_tree(L, R, D, scale, sigma, method=1)
    assert np.array_equal(got, want), int((got != want).sum())


@pytest.mark.parametrize("method", [0, 1])
def test_stmatch_cli(oracle, tmp_path, method):
    """STMatching's command line (main.cpp argument order) through PNG files: the written map equals the
    oracle's for the same decoded inputs."""
    from PIL import Image
    from gpu_stereo_matching_amd import stmatch
    g = np.load(os.path.join(GOLDEN, "middlebury_bgr.npz"))
    L, R = g["Art/view1"], g["Art/view5"]
    lp, rp, op = tmp_path / "l.png", tmp_path / "r.png", tmp_path / "d.png"
    Image.fromarray(L[:, :, ::-1].copy()).save(lp)
    Image.fromarray(R[:, :, ::-1].copy()).save(rp)
    assert stmatch._main([str(lp), str(rp), str(op), "48", "5", "0.1", str(method)]) == 0
    got = np.asarray(Image.open(op))
    want = (oracle.st2_disp if method else oracle.st_disp)(L, R, 48, 5, 0.1)[0]
    assert np.array_equal(got, want)


def test_workspace_grows_and_is_reused_across_methods(oracle):
    """One fresh handle through ST-2 and ST-1 calls ordered so that every workspace buffer of both slots
    grows after the other method used it at a smaller size, and is then reused while oversized (the
    smallest frames of this suite: 2 pixels wide, one row, W < D); every map bit-exact.  The tree arrays
    follow the last call's shape.  Then a second handle after the first is closed."""
    import gpu_stereo_matching_amd as sm

    def pair(W, H, seed):
        rng = np.random.default_rng(seed)
        L = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
        L[: H // 2, : W // 3] = 77
        R = np.roll(L, -min(5, W - 1), axis=1)
        R[:, -3:] = rng.integers(0, 256, (H, min(3, W), 3), dtype=np.uint8)
        return L, R

    def check(m, method, W, H, D, seed):
        L, R = pair(W, H, seed)
        want = (oracle.st2_disp if method else oracle.st_disp)(L, R, D, 2, 0.1)[0]
        got = m.segment_tree(L, R, D, 2, 0.1, method=method)
        assert np.array_equal(got, want), (method, W, H, D, int((got != want).sum()))

    steps = [(1, 64, 48, 16), (0, 300, 200, 64), (1, 2, 5, 3), (0, 123, 1, 9), (1, 300, 200, 64), (0, 64, 48, 16)]
    with sm.BlockMatcher(0, 320, 208, 64) as m:
        for i, (method, W, H, D) in enumerate(steps):
            check(m, method, W, H, D, 40 + i)
            if i == 4:
                assert len(m.segment_tree_arrays(300, 200)["rank"]) == 300 * 200
                with pytest.raises(sm.SMError):
                    m.segment_tree_arrays(64, 48)
    with sm.BlockMatcher(0, 320, 208, 64) as m:
        check(m, *steps[0], 40)


def test_workgroup_filter_fallback():
    """The workgroup-per-disparity filter (st_filter_kernel), which trees wider than the wave filter's
    LDS buffers take, forced by SM_ST_WAVE_FILTER=0 in a child process: ST-1 and ST-2 bit-exact."""
    import subprocess, sys, textwrap
    code = textwrap.dedent("""
        import sys, numpy as np
        sys.path.insert(0, %r)
        import gpu_stereo_matching_amd as sm
        from oracle import oracle
        rng = np.random.default_rng(21)
        L = rng.integers(0, 256, (61, 97, 3), dtype=np.uint8)
        L[:30, :32] = 77
        R = np.roll(L, -5, axis=1)
        with sm.BlockMatcher(0, 128, 64, 64) as m:
            ok1 = np.array_equal(m.segment_tree(L, R, 16, 1, 0.1), oracle.st_disp(L, R, 16, 1, 0.1)[0])
            ok2 = np.array_equal(m.segment_tree(L, R, 16, 1, 0.1, method=1), oracle.st2_disp(L, R, 16, 1, 0.1)[0])
        print("OK" if ok1 and ok2 else "MISMATCH", ok1, ok2)
    """ % ROOT)
    env = dict(os.environ, SM_ST_WAVE_FILTER="0")
    out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=240)
    assert out.returncode == 0, out.stderr[-2000:]
    assert "OK" in out.stdout, out.stdout


def _bfs_cases():
    g = np.load(os.path.join(GOLDEN, "middlebury_bgr.npz"))
    yield "art", g["Art/view1"], g["Art/view5"], 60
    for W, H, seed in ((97, 61, 31), (2, 5, 32), (123, 1, 33)):
        rng = np.random.default_rng(seed)
        L = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
        L[: H // 2, : W // 3] = 77
        yield f"{W}x{H}", L, np.roll(L, -min(5, W - 1), axis=1), 16
    flat = np.full((40, 30, 3), 9, np.uint8)                 # every weight equal: a comb-shaped tree
    yield "flat", flat, flat, 8


@pytest.mark.parametrize("method", [0, 1])
def test_device_bfs_equals_host_bfs(matcher, method):
    """The BFS on the GPU (Euler tour + pointer jumping + depth sort, bm_segtree_build.hip) against the host's
    BFS (st_host::bfs_tree, SM_ST_HOST_BFS=1, itself checked against oracle/st_oracle.c by
    tests/test_st_host.py): the tree arrays the filter reads (rank, parent, first, child words, level
    offsets, parent distances) identical, for ST-1's colour tree and ST-2's colour + depth tree, and the
    maps identical."""
    for name, L, R, D in _bfs_cases():
        H, W, _ = L.shape
        os.environ["SM_ST_HOST_BFS"] = "1"
        try:
            want_map = matcher.segment_tree(L, R, D, 2, 0.1, method=method)
            want = matcher.segment_tree_arrays(W, H)
        finally:
            del os.environ["SM_ST_HOST_BFS"]
        got_map = matcher.segment_tree(L, R, D, 2, 0.1, method=method)
        got = matcher.segment_tree_arrays(W, H)
        assert len(got["lev"]) == len(want["lev"]), name
        for k in want:
            assert np.array_equal(got[k], want[k]), (name, k, int((got[k] != want[k]).sum()))
        assert np.array_equal(got_map, want_map), name
        assert matcher.segment_tree_stats()[2] == len(want["lev"]) - 1
    import gpu_stereo_matching_amd as sm
    with pytest.raises(sm.SMError):   # a stale frame size is refused, not mis-sliced
        matcher.segment_tree_arrays(W + 1, H)
