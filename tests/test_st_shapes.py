"""The premises of tests/test_gpu_segtree_shapes.py, on the CPU: every GPU case there rests on a claim
about the tree its input builds (tests/st_shapes.py), asserted here with the C oracle (oracle.st_tree,
oracle.st_disp, oracle.st2_disp).  A change to a generator or to the oracle fails here first."""
import numpy as np
import pytest

import st_shapes as S


@pytest.fixture(scope="module")
def deep(oracle):
    L, R = S.deep_pair()
    tree = oracle.st_tree(L)
    d = S.DEEP
    return dict(L=L, R=R, tree=tree, st1=oracle.st_disp(L, R, d["D"], d["scale"], d["sigma"]),
                st2=oracle.st2_disp(L, R, d["D"], d["scale"], d["sigma"]))


@pytest.mark.parametrize("W,H,levels", [(640, 440, 70933), (520, 512, 66955), (60, 40, 653)])
def test_serpentine_depth(oracle, W, H, levels):
    """The plain serpentine: measured 70,933 levels at 640 x 440, 66,955 at 520 x 512 and 653 at 60 x 40,
    the widest level 6 nodes each (the corridor is 2 thick and turns through 2-column openings).  About
    W H / 4 - a few per turn: the tree follows the corridor and nothing cuts through a wall."""
    t = oracle.st_tree(S.serpentine(W, H))
    widths = S.level_widths(t)
    assert len(widths) == t["levels"] == levels
    assert max(widths) == 6
    assert t["levels"] >= W * H // 4


def test_deep_case_is_deeper_than_two_radix_passes(deep):
    """The textured serpentine (noise amplitude 8) at 640 x 440: measured 70,837 levels for the colour
    tree (ST-1) and 70,779 for ST-2's colour + depth tree (70,837 to 71,482 over seeds 0..2), the widest
    level 12 nodes.  levels >= 65,537 makes the largest depth >= 65,536 = 2^16, so the third 8-bit pass of
    the depth sort runs; P > 65,536 makes the host launch three.  Every level is one task (<= 64 nodes)."""
    P = S.DEEP["W"] * S.DEEP["H"]
    assert P > 65536
    widths = S.level_widths(deep["tree"])
    assert len(widths) == deep["tree"]["levels"] == deep["st1"][1]
    assert deep["st1"][1] >= 65537
    assert deep["st2"][1] >= 65537          # the depth tree of ST-2's second run
    assert max(widths) <= 64


@pytest.mark.parametrize("method", [0, 1])
def test_deep_case_map_is_not_vacuous(deep, method):
    """The oracle map of the deep case has at least two disparities on >= 25 % of the pixels each (the
    right view is the left shifted by 2 in the top half and by 5 in the bottom half; measured at D = 8,
    scale 4: 140,793 / 140,807 pixels for ST-1, 140,794 / 140,806 for ST-2), so a bit-exact map
    comparison on it says something about the filter."""
    disp = deep["st2" if method else "st1"][0]
    _, counts = np.unique(disp, return_counts=True)
    assert (counts >= disp.size // 4).sum() >= 2, counts


ROWS_IN_USE = sorted(set(S.RADIX_ROWS + S.TASK_ROWS + tuple(W for W, H, _ in S.BOUNDARY_SHAPES if H == 1)))


def _signal(oracle, L, R, D, scale, sigma):
    """(pixels whose unfiltered cost varies with d, the winner-takes-all map of the unfiltered cost after
    the path's scale and 7 x 7 median, the ST-1 map, the ST-2 map)."""
    c = oracle.st_cost(L, R, D)
    raw = oracle.median(np.minimum(np.argmin(c, axis=2) * scale, 255).astype(np.uint8), 3)
    vary = int((c.max(axis=2) != c.min(axis=2)).sum())
    return vary, raw, oracle.st_disp(L, R, D, scale, sigma)[0], oracle.st2_disp(L, R, D, scale, sigma)[0]


@pytest.mark.parametrize("W", ROWS_IN_USE)
def test_row_is_the_path(oracle, W):
    """A 1 x W frame builds the path: levels == W (every level one node), so the largest depth is W - 1
    and the wave filter gets W leaf-to-root and W - 1 root-to-leaf tasks."""
    t = oracle.st_tree(S.row_pair(W)[0])
    assert t["levels"] == W
    assert np.array_equal(t["parent"], np.arange(-1, W - 1))
    assert int(t["pdist"].max()) <= 20          # 15 of colour, 5 of cross-segment penalty


@pytest.mark.parametrize("W", ROWS_IN_USE)
def test_row_map_observes_the_filter(oracle, W):
    """The map is the only observable of the wave filter's tasks, so on every row in use it must depend on
    the filter.  The cost varies with d on at least 3 / 4 of the W - 1 pixels that have a left neighbour
    (pixel 0 reads right pixel 0 at every d); the ST-1 and ST-2 maps are not all 0 and differ from the
    winner-takes-all of the unfiltered cost; from W = 31 they take both disparities.  Below that a
    two-valued map is not required: the weights are >= 0.77 per step, so a short row aggregates to nearly
    one sum, and at W = 2 both pixels get the same argmin whatever the colours.  Measured: W = 2, 3, 4 and
    ST-1 at W = 18 give one value, with every pixel of W = 3, 4 and 5 of 18 moved off the unfiltered
    choice; W = 15, 16, 17 split 9 / 6, 10 / 6, 13 / 4; W = 31 .. 49 split near the middle; at 65,537 the
    map splits 32,770 / 32,767 and the filter moves 226 pixels."""
    L, R = S.row_pair(W)
    vary, raw, st1, st2 = _signal(oracle, L, R, S.ROW_D, S.ROW_SCALE, S.ROW_SIGMA)
    assert 4 * vary >= 3 * (W - 1), vary
    for disp in (st1, st2):
        assert disp.max() > 0
        assert (disp != raw).any()
        if W >= 31:
            assert len(np.unique(disp)) >= 2


def test_task_rows_straddle_the_task_blocks():
    """kStBlk = 16 tasks per block: the up (W) and down (W - 1) counts of TASK_ROWS hit 1, 2, 15, 16, 17,
    32 and 33, i.e. both sides of one and two full blocks, and counts with no block b + 1 or b + 2."""
    counts = {W for W in S.TASK_ROWS} | {W - 1 for W in S.TASK_ROWS}
    assert {1, 2, 15, 16, 17, 32, 33} <= counts


def test_radix_rows_straddle_the_pass_switches():
    """Largest depth W - 1 on both sides of 2^8 and 2^16; launched passes ceil(ceil_log2(W) / 8)."""
    def launched(P):
        bits = max(1, (P - 1).bit_length())
        return (bits + 7) // 8
    assert [W - 1 for W in S.RADIX_ROWS] == [255, 256, 65535, 65536]
    assert [launched(W) for W in S.RADIX_ROWS] == [1, 2, 2, 3]


@pytest.mark.parametrize("W,H", S.FLAT_SHAPES)
def test_flat_left_level_widths(oracle, W, H):
    """Every weight ties at 1: W + H - 1 levels (330 for 200 x 131 and for 131 x 200) whose widths ramp 1,
    2, .., 131 and back, so levels of exactly 63, 64, 65, 128 and 129 nodes exist: one full task less a
    lane, one full task, a full task plus a one-lane task, two full tasks, two full tasks plus a one-lane
    task.  Every tree distance but the root's is 1."""
    L, _ = S.flat_left(W, H, 1)
    t = oracle.st_tree(L)
    widths = S.level_widths(t)
    assert len(widths) == t["levels"] == W + H - 1
    assert max(widths) == min(W, H)
    assert set(S.LEVEL_WIDTHS) <= set(widths)
    assert t["pdist"][0] == 0 and (t["pdist"][1:] == 1).all()


@pytest.mark.parametrize("W,H", S.FLAT_SHAPES)
def test_flat_left_map_observes_the_filter(oracle, W, H):
    """With distance 1 on every edge the filtered cost differs from pixel to pixel: the cost varies with d
    on > 90 % of the pixels, the ST-1 and ST-2 maps take at least two values on >= 10 % of the pixels each
    and differ from the winner-takes-all of the unfiltered cost on >= 25 % of the pixels (measured for
    200 x 131: 26,062 of 26,200 pixels vary; ST-1 takes 7 values, the largest groups 8,922 / 8,149 /
    6,598 pixels, and differs from the unfiltered choice on 16,159; ST-2 on 18,346)."""
    L, R = S.flat_left(W, H, 1)
    vary, raw, st1, st2 = _signal(oracle, L, R, 8, 4, 0.1)
    assert 10 * vary > 9 * W * H
    for disp in (st1, st2):
        _, counts = np.unique(disp, return_counts=True)
        assert (10 * counts >= disp.size).sum() >= 2, counts
        assert 4 * int((disp != raw).sum()) >= disp.size


@pytest.mark.parametrize("W,H,listed", S.BOUNDARY_SHAPES)
def test_boundary_shape_quantities(oracle, W, H, listed):
    """Every shape of the block-boundary list has the pixel, tour-arc, edge and level counts it is listed
    for."""
    q = S.shape_quantities(W, H)
    L = S.boundary_case(W, H)[0]
    assert L.shape == (H, W, 3)
    q["levels"] = oracle.st_tree(L)["levels"]
    for k, v in listed.items():
        assert q[k] == v, (W, H, k, q[k], v)


@pytest.mark.parametrize("W,H", [(W, H) for W, H, _ in S.BOUNDARY_SHAPES if H > 1])
def test_boundary_shape_map_observes_the_filter(oracle, W, H):
    """The block-boundary cases rest on the tree arrays first, but their maps are not vacuous either: on
    every shape of more than one row the cost varies with d on >= 3 / 4 of the pixels right of column 0
    (2 x 2: on both), the ST-1 and ST-2 maps differ from the winner-takes-all of the unfiltered cost, and
    they take at least two values (2 x 2: one value, not 0).  The 1-row shapes are rows: see
    test_row_map_observes_the_filter."""
    L, R, D, scale, sigma = S.boundary_case(W, H)
    vary, raw, st1, st2 = _signal(oracle, L, R, D, scale, sigma)
    assert 4 * vary >= 3 * (W - 1) * H, vary
    for disp in (st1, st2):
        assert disp.max() > 0
        assert (disp != raw).any()
        if W * H > 4:
            assert len(np.unique(disp)) >= 2


def test_boundary_shapes_cover_each_block_on_both_sides():
    """Over the list: P, the tour length and the level count one item (the tour: one arc pair) below, at
    and above a multiple of the scan block; the edge count below, at and above the edge-sort block; and
    1 .. kEdgeChunks edges."""
    seen = {}
    for _, _, listed in S.BOUNDARY_SHAPES:
        for k, v in listed.items():
            seen.setdefault(k, set()).add(v)
    B, E = S.SCAN_BLOCK, S.EDGE_BLOCK
    assert {B - 1, B, B + 1, 2 * B - 1, 2 * B, 2 * B + 1} <= seen["P"]
    assert {B - 2, B, B + 2, 2 * B - 2, 2 * B, 2 * B + 2, 4 * B - 2, 4 * B, 4 * B + 2} <= seen["tour"]
    assert {B - 1, B, B + 1} <= seen["levels"]
    assert {E - 1, E, E + 1} <= seen["edges"]
    assert set(range(1, S.EDGE_CHUNKS + 1)) <= seen["edges"]
