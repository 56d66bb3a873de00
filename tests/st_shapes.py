"""Constructed BGR frames whose segment trees have a chosen shape (tests/test_st_shapes.py asserts the
shapes on the CPU oracle, tests/test_gpu_segtree_shapes.py runs the GPU path on them).

The tree is built on the 3 x 3 median of the left frame, rooted at pixel 0 and walked breadth first, so
its level count is the longest path from the top-left corner:
  serpentine   one long corridor folded over the frame: ~W * H / (corridor + wall) levels, each a few nodes
  row          a 1 x W frame: the path, W levels of one node
  flat_left    every weight ties (at 1): a comb of W + H - 1 levels whose widths ramp 1, 2, .., min(W, H)
"""
import numpy as np

COLOUR_A = (40, 90, 200)      # corridor (BGR)
COLOUR_B = (210, 160, 30)     # wall: every channel >= 110 away from the corridor's
ROW_SEED = 2                  # see row_pair
ROW_D, ROW_SCALE, ROW_SIGMA = 3, 1, 0.3


def serpentine(W, H, corridor=2, wall=2, noise=0, seed=0):
    """Horizontal corridors of COLOUR_A, `corridor` rows thick, between walls of COLOUR_B, `wall` rows
    thick; wall k with a corridor below it is opened over `corridor` columns at the right end for even k,
    at the left end for odd k.  Stripes of two pixels survive the 3 x 3 median, so the colour tree follows
    the corridor from pixel 0 to the last one.  noise > 0 adds uniform integers of [0, noise) to every
    channel (the "textured" serpentine: the matching cost then has structure, the 110-level colour gap
    keeps the walls)."""
    img = np.empty((H, W, 3), np.uint8)
    img[:] = COLOUR_A
    period = corridor + wall
    for k, y0 in enumerate(range(corridor, H, period)):
        img[y0:y0 + wall] = COLOUR_B
        if y0 + wall >= H:
            continue                      # a wall along the bottom edge leads nowhere: it stays closed
        if k % 2 == 0:
            img[y0:y0 + wall, max(W - corridor, 0):] = COLOUR_A
        else:
            img[y0:y0 + wall, :corridor] = COLOUR_A
    if noise > 0:
        rng = np.random.default_rng(seed)
        img = img + rng.integers(0, noise, img.shape, dtype=np.uint8)
    return img


def row(W, seed):
    """A low-contrast random 1 x W frame: every channel 100 + [0, 16).  Its only edges are the W - 1
    horizontal ones, so the tree is the path whatever the colours: W levels, largest depth W - 1, W
    leaf-to-root and W - 1 root-to-leaf tasks, W - 1 edges.  The colour differences stay below the cost's
    truncation (7 per channel on average) and the tree distances at or below 20 (15 of colour, 5 where the
    tree crosses two segments), so with sigma = 0.3 a node's weight is >= exp(-20 / 76.5) = 0.77, mostly
    above 0.9, and the aggregation reaches over several blocks of 16 one-node tasks."""
    return low_contrast(W, 1, seed)


def low_contrast(W, H, seed):
    """row's colours on H rows: every channel 100 + [0, 16)."""
    return (100 + np.random.default_rng(seed).integers(0, 16, (H, W, 3))).astype(np.uint8)


def row_right(L, seed):
    """The right view of a row (or of a low_contrast frame, row by row): the left half of the columns
    shifted by 1, the right half by 2 (both below the rows' D = 3), columns with no source far off (200),
    then noise of [-2, 2] on every channel: the unfiltered cost picks the wrong disparity at many pixels
    and the tree filter repairs them."""
    W = L.shape[1]
    x = np.arange(W)
    src = x + np.where(x < W // 2, 1, 2)
    R = np.full(L.shape, 200, np.int64)
    R[:, src < W] = L[:, src[src < W]]
    R += np.random.default_rng(seed + 1000).integers(-2, 3, L.shape)
    return R.astype(np.uint8)


def row_pair(W):
    """(left, right) of the W-pixel row every suite uses, at ROW_D, ROW_SCALE, ROW_SIGMA (ROW_SEED: chosen
    once so that the premises of tests/test_st_shapes.py hold for every width in use)."""
    L = row(W, ROW_SEED + W)
    return L, row_right(L, ROW_SEED + W)


def textured(W, H, seed):
    """A random W x H frame with a flat patch (long runs of equal-weight edges), as the end-to-end
    suite's frames."""
    L = np.random.default_rng(seed).integers(0, 256, (H, W, 3), dtype=np.uint8)
    L[: H // 2, : W // 3] = 77
    return L


def right_view(L, seed=0, noise=0):
    """The right view of L: the top half shifted by 2, the bottom half by 5 (a 1-row frame: by 5), the
    shift capped at W - 1, with up to 3 random columns at the right edge; noise > 0 adds uniform integers
    of [-noise, noise] to every channel (clipped)."""
    H, W, _ = L.shape
    R = np.empty_like(L)
    R[: H // 2] = np.roll(L[: H // 2], -min(2, W - 1), axis=1)
    R[H // 2:] = np.roll(L[H // 2:], -min(5, W - 1), axis=1)
    n = min(3, W)
    rng = np.random.default_rng(seed + 1000)
    R[:, W - n:] = rng.integers(0, 256, (H, n, 3), dtype=np.uint8)
    if noise > 0:
        R = np.clip(R.astype(np.int64) + rng.integers(-noise, noise + 1, R.shape), 0, 255).astype(np.uint8)
    return R


def flat_left(W, H, seed):
    """(left, right): a left frame that is flat in slope, not in value: channel 0 = 20 + x, channel 1 =
    20 + y, channel 2 constant (W, H <= 235).  Each channel depends on one coordinate, so the 3 x 3 median
    (replicate borders) leaves it unchanged and every edge weight is exactly 1: all weights tie, the edge
    order alone decides, and the tree is the comb of a constant frame, W + H - 1 levels of widths 1, 2, ..,
    min(W, H), .., 2, 1, but with tree distance 1 on every edge, so the filtered cost differs from pixel
    to pixel (a constant frame has distance 0 and weight 1 everywhere: every pixel gets the same global
    sum and the map is one constant).  The right frame is right_view(left) with noise of [-4, 4]."""
    assert W <= 235 and H <= 235
    L = np.empty((H, W, 3), np.uint8)
    L[:, :, 0] = 20 + np.arange(W)[None, :]
    L[:, :, 1] = 20 + np.arange(H)[:, None]
    L[:, :, 2] = 9
    return L, right_view(L, seed, noise=4)


def level_widths(tree):
    """Nodes per BFS level of an oracle.st_tree dict.  In BFS order the parent indices never decrease
    (the root's is -1), so the level after [lo, hi) ends at the first node whose parent is >= hi."""
    parent = np.asarray(tree["parent"], np.int64)     # the dtype of the needle: no cast of P items per level
    P = len(parent)
    widths, lo, hi = [], 0, 1
    while lo < P:
        widths.append(hi - lo)
        lo, hi = hi, int(np.searchsorted(parent, np.int64(hi), side="left"))
    return widths


def edge_count(W, H):
    return (H - 1) * (2 * W - 1) + W - 1


# ---- the shapes of the GPU suite; tests/test_st_shapes.py asserts what each is listed for ----
DEEP = dict(W=640, H=440, noise=8, seed=1, D=8, scale=4, sigma=0.1)


def deep_pair():
    L = serpentine(DEEP["W"], DEEP["H"], noise=DEEP["noise"], seed=DEEP["seed"])
    return L, right_view(L, DEEP["seed"])


# row widths around the depth sort's 8-bit passes: largest depth W - 1 = 255, 256, 65535, 65536
RADIX_ROWS = (256, 257, 65536, 65537)
# row widths whose task counts (W up, W - 1 down) fall on both sides of 1, 2 and 3 blocks of 16 tasks
TASK_ROWS = (2, 3, 15, 16, 17, 18, 31, 32, 33, 34, 49)
# comb trees with levels of exactly these widths
FLAT_SHAPES = ((200, 131), (131, 200))
LEVEL_WIDTHS = (63, 64, 65, 128, 129)

SCAN_BLOCK = 512     # kScIPB: items per block of the scans and of the depth sort (P, the tour, the levels)
EDGE_BLOCK = 2048    # kRxIPB: items per block of the edge sort
EDGE_CHUNKS = 4      # StSlot::kEdgeChunks

# (W, H, {quantity: the value the shape is listed for}); quantities: P = W H pixels, tour = 2 (P - 1) arcs,
# edges = (H - 1)(2 W - 1) + W - 1, levels (rows only: a textured frame's level count follows its content)
BOUNDARY_SHAPES = (
    (511, 1, dict(P=511, levels=511)),                       # one scan block less an item
    (512, 1, dict(P=512, levels=512, tour=1022)),            # exactly one block of pixels and of levels
    (513, 1, dict(P=513, levels=513, tour=1024)),            # a block and one item; the tour exactly 2 blocks
    (257, 2, dict(P=514, tour=1026)),                        # the tour 2 blocks and two arcs
    (16, 16, dict(P=256, tour=510)),                         # the tour one block less two arcs
    (257, 1, dict(P=257, tour=512)),                         # the tour exactly one block
    (43, 6, dict(P=258, tour=514)),                          # the tour one block and two arcs
    (32, 16, dict(P=512)),                                   # P = 512 in two dimensions
    (27, 19, dict(P=513, tour=1024)),
    (33, 31, dict(P=1023)),
    (32, 32, dict(P=1024, tour=2046)),
    (41, 25, dict(P=1025, tour=2048)),
    (38, 27, dict(P=1026, tour=2050)),
    (2048, 1, dict(edges=2047)),                             # one edge-sort block less an edge
    (683, 2, dict(edges=2047)),
    (2049, 1, dict(edges=2048)),                             # exactly one edge-sort block
    (121, 9, dict(edges=2048)),
    (2050, 1, dict(edges=2049)),                             # a block and one edge
    (2, 1, dict(edges=1)),                                   # fewer edges than download chunks
    (3, 1, dict(edges=2)),
    (4, 1, dict(edges=3)),
    (2, 2, dict(edges=4)),                                   # as many edges as chunks
)


def shape_quantities(W, H):
    P = W * H
    return dict(P=P, tour=2 * (P - 1), edges=edge_count(W, H))


def boundary_case(W, H):
    """(left, right, D, scale, sigma) of a block-boundary shape.  A 1-row shape is the row pair (levels ==
    W) at the rows' parameters; 2 x 2 is a low-contrast frame with the rows' right view (in a textured
    2-wide frame every right pixel is a random fill and the cost is truncated at every d); the others are
    textured random frames with the two-shift right view and noise of [-8, 8], at D = 8 > both shifts."""
    if H == 1:
        return row_pair(W) + (ROW_D, ROW_SCALE, ROW_SIGMA)
    if W * H <= 4:
        L = low_contrast(W, H, ROW_SEED + 7)
        return L, row_right(L, ROW_SEED + 7), ROW_D, ROW_SCALE, ROW_SIGMA
    L = textured(W, H, 7 * W + H)
    return L, right_view(L, W + H, noise=8), 8, 2, 0.1
