"""The segment-tree path (bm_segtree.hip, bm_segtree_build.hip, bm_segtree_host.h) on the smallest
constructed frames at which each branch of the device build and of both filters runs: trees deeper than
two 8-bit passes of the depth sort, the path tree (levels == P), every count around the wave filter's
task blocks, levels around the 64-node task, and every block boundary of the scans, the sorts and the
edge download.  tests/st_shapes.py builds the frames, tests/test_st_shapes.py asserts their tree shapes
on the CPU.  Every comparison is bit for bit: the map against the C oracle, the tree arrays against the
host BFS (SM_ST_HOST_BFS=1) and, for ST-1, against oracle.st_tree directly."""
import os

import numpy as np
import pytest

import st_shapes as S

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_refs = {}


def _ref(oracle, key, L, R, D, scale, sigma, method):
    """(oracle map, its level count, oracle.st_tree of L for ST-1), computed once per input and method."""
    k = (key, D, scale, sigma, method)
    if k not in _refs:
        if method:
            r = oracle.st2_disp(L, R, D, scale, sigma)
            _refs[k] = (r[0], r[1], None)
        else:
            r = oracle.st_disp(L, R, D, scale, sigma)
            _refs[k] = (r[0], r[1], oracle.st_tree(L))
        for a in _refs[k]:
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
    return _refs[k]


def _check_map(m, oracle, key, L, R, D, scale, sigma, method):
    want, levels, _ = _ref(oracle, key, L, R, D, scale, sigma, method)
    got = m.segment_tree(L, R, D, scale, sigma, method=method)
    assert np.array_equal(got, want), (key, method, int((got != want).sum()))
    assert m.segment_tree_stats()[2] == levels, (key, method)
    return got


def _check(m, oracle, key, L, R, D, scale=1, sigma=0.1, method=0):
    """The common check: map and level count against the oracle; the device-built tree arrays against the
    host BFS's of the same call, key by key; for ST-1 also against oracle.st_tree."""
    H, W, _ = L.shape
    P = W * H
    got_map = _check_map(m, oracle, key, L, R, D, scale, sigma, method)
    got = m.segment_tree_arrays(W, H)
    os.environ["SM_ST_HOST_BFS"] = "1"
    try:
        host_map = m.segment_tree(L, R, D, scale, sigma, method=method)
        host = m.segment_tree_arrays(W, H)
    finally:
        del os.environ["SM_ST_HOST_BFS"]
    assert np.array_equal(host_map, got_map), (key, method)
    assert set(got) == set(host)
    for k in host:
        assert got[k].shape == host[k].shape, (key, method, k, got[k].shape, host[k].shape)
        assert np.array_equal(got[k], host[k]), (key, method, k, int((got[k] != host[k]).sum()))
    levels, tree = _ref(oracle, key, L, R, D, scale, sigma, method)[1:]
    assert len(got["lev"]) == levels + 1 and got["lev"][0] == 0 and got["lev"][-1] == P
    if tree is not None:
        assert tree["levels"] == levels
        assert np.array_equal(got["rank"][tree["node"]], np.arange(P)), key
        for k in ("parent", "first", "pdist"):
            assert np.array_equal(got[k], tree[k]), (key, k, int((got[k] != tree[k]).sum()))
        assert np.array_equal(got["child"] & 0xFF, tree["nchild"]), key
        assert int(tree["nchild"].max()) <= 3          # the child word has three distance bytes
        for z in range(3):
            assert np.array_equal((got["child"] >> (8 * (z + 1))) & 0xFF, tree["cdist"][:, z]), (key, z)
        assert np.array_equal(np.diff(got["lev"]), S.level_widths(tree)), key


@pytest.fixture(scope="module")
def sm():
    import gpu_stereo_matching_amd
    return gpu_stereo_matching_amd


@pytest.fixture(scope="module")
def small(sm):
    """One handle for every shape up to 2050 x 1 / 200 x 200: its workspace is reused across them."""
    with sm.BlockMatcher(0, 2050, 200, 8) as m:
        yield m


@pytest.fixture(scope="module")
def deep_handle(sm):
    with sm.BlockMatcher(0, S.DEEP["W"], S.DEEP["H"], 8) as m:
        yield m


@pytest.mark.parametrize("method", [0, 1])
def test_deep_tree_third_radix_pass(deep_handle, oracle, method):
    """The textured serpentine at 640 x 440 (about 71 k levels, each a single task): the depth sort of
    gpu_bfs launches three 8-bit passes (P = 281,600 > 2^16) and all three run (largest depth >= 2^16), so
    st_radix_passes_run returns 3 and st_bfs_arrays_kernel reads the sorted order from buffer B; both
    passes of st_filter_wave_kernel walk ~71 k one-task levels (~4,400 task blocks)."""
    L, R = S.deep_pair()
    d = S.DEEP
    _check(deep_handle, oracle, "deep", L, R, d["D"], d["scale"], d["sigma"], method)


def test_deep_tree_workgroup_filter():
    """st_filter_kernel (forced by SM_ST_WAVE_FILTER=0, read once per process: a child process) walks the
    deep case's ~71 k levels, two workgroup barriers each: ST-1 and ST-2 bit-exact."""
    import subprocess, sys, textwrap
    code = textwrap.dedent("""
        import sys, numpy as np
        sys.path[:0] = [%r, %r]
        import gpu_stereo_matching_amd as sm
        from oracle import oracle
        import st_shapes as S
        L, R = S.deep_pair()
        d = S.DEEP
        a = (L, R, d["D"], d["scale"], d["sigma"])
        with sm.BlockMatcher(0, d["W"], d["H"], 8) as m:
            ok1 = np.array_equal(m.segment_tree(*a), oracle.st_disp(*a)[0])
            ok2 = np.array_equal(m.segment_tree(*a, method=1), oracle.st2_disp(*a)[0])
        print("OK" if ok1 and ok2 else "MISMATCH", ok1, ok2)
    """ % (ROOT, os.path.join(ROOT, "tests")))
    env = dict(os.environ, SM_ST_WAVE_FILTER="0")
    out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr[-2000:]
    assert "OK" in out.stdout, out.stdout


@pytest.mark.parametrize("method", [0, 1])
@pytest.mark.parametrize("W", S.RADIX_ROWS)
def test_radix_pass_switches(sm, oracle, W, method):
    """Rows of 256, 257, 65,536 and 65,537 pixels: largest depths 255, 256, 65,535 and 65,536 against 1, 2,
    2 and 3 launched passes of the depth sort, i.e. the gate hdr[4] >> (8 k) of st_rx_skip /
    st_radix_passes_run on both sides of 2^8 and 2^16, and the A / B choice of st_bfs_arrays_kernel for
    (launched, ran) = (1, 1), (2, 2), (2, 2), (3, 3).  The path tree is also the maximal level count
    (levels == P): the bound of upload_tree, lev[P], E[P + 2] and task_slot_cap(P), at 65,537."""
    L, R = S.row_pair(W)
    with sm.BlockMatcher(0, W, 1, 8) as m:
        _check(m, oracle, ("row", W), L, R, S.ROW_D, S.ROW_SCALE, S.ROW_SIGMA, method)


@pytest.mark.parametrize("method", [0, 1])
@pytest.mark.parametrize("W", S.TASK_ROWS)
def test_task_block_counts(small, oracle, W, method):
    """Rows of 2 .. 49 pixels: W leaf-to-root and W - 1 root-to-leaf tasks of one node, on both sides of
    one, two and three blocks of kStBlk = 16 in st_filter_wave_kernel's pipeline, whose prefetches of the
    records of block b + 2 and of the operands of block b + 1 are clamped to the last task when those
    blocks do not exist (a single task: every record of all three blocks is that task).  The tasks show
    only in the map: the rows are low in contrast (weights >= 0.77 per step at sigma 0.3, the aggregation
    reaches over several blocks) and tests/test_st_shapes.py asserts that each map depends on the filter."""
    L, R = S.row_pair(W)
    _check(small, oracle, ("row", W), L, R, S.ROW_D, S.ROW_SCALE, S.ROW_SIGMA, method)


@pytest.mark.parametrize("method", [0, 1])
@pytest.mark.parametrize("W,H", S.FLAT_SHAPES)
def test_level_widths_around_the_task(small, oracle, W, H, method):
    """A left frame whose edge weights all tie at 1 (a comb: level widths 1 .. 131 and back): levels of
    exactly 63, 64, 65, 128 and 129 nodes, so st_task_kernel / wave_tasks cut two and three tasks per
    level with a last task one lane wide, whose other 63 lanes compute into the level buffer's 64-float
    pad.  Every tree distance is 1, so the filtered cost and the map differ from pixel to pixel
    (tests/test_st_shapes.py): a dropped or misplaced task changes the map."""
    L, R = S.flat_left(W, H, 1)
    _check(small, oracle, ("flat", W, H), L, R, 8, 4, 0.1, method)


@pytest.mark.parametrize("method", [0, 1])
@pytest.mark.parametrize("W,H,listed", S.BOUNDARY_SHAPES, ids=lambda v: str(v) if isinstance(v, int) else
                         ",".join(f"{k}={x}" for k, x in v.items()))
def test_block_boundaries(small, oracle, W, H, listed, method):
    """`listed` names what the shape is there for: P, the tour length 2 (P - 1) or the level count one
    item below, at or above a multiple of kScIPB = 512 (st_scan_*_kernel, st_tour_apply_kernel,
    st_level_sums_kernel, the depth sort's blocks); the edge count around kRxIPB = 2048 (the edge sort's
    blocks; ST-2 sorts its float weights in four passes); or 1 .. 4 edges, at most one per download chunk
    (kEdgeChunks = 4: empty chunks, wait_edges with a chunk of one edge)."""
    L, R, D, scale, sigma = S.boundary_case(W, H)
    _check(small, oracle, ("boundary", W, H), L, R, D, scale, sigma, method)


def test_workspace_reused_oversized_after_a_deep_tree(sm, oracle):
    """One handle runs deep -> 2 x 1 -> deep -> 2 x 1 -> deep with the methods alternating around each
    step: after a 71 k-level tree the BFS scratch (carved anew from the same block for P = 2), the task
    buffer and the page-locked header are reused oversized, then grow back into the deep layout; every
    map and level count bit-exact.  The 2 x 1 map is [1, 1] where the unfiltered cost gives [0, 1]
    (tests/test_st_shapes.py), so it shows whether the filter ran on the right tasks."""
    Ld, Rd = S.deep_pair()
    d = S.DEEP
    Lt, Rt = S.row_pair(2)
    with sm.BlockMatcher(0, d["W"], d["H"], 8) as m:
        for which, method in (("deep", 0), ("tiny", 1), ("deep", 1), ("tiny", 0), ("deep", 0)):
            if which == "deep":
                _check_map(m, oracle, "deep", Ld, Rd, d["D"], d["scale"], d["sigma"], method)
            else:
                _check_map(m, oracle, ("row", 2), Lt, Rt, S.ROW_D, S.ROW_SCALE, S.ROW_SIGMA, method)
