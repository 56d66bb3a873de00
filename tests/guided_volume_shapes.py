"""The shapes of the guided cost volume's tests (tests/test_gpu_guided_volume.py), and the restatement of which
compiled path of the volume kernel a tile takes (tests/test_guided_volume_model.py).

guided_fused_kernel<R | 16, false> (csrc/bm_guided.hip) is compiled once per radius; inside it S1V is instantiated
with and without its column mask (NOMASK: tile-uniform, every P column of the tile inside the image and >= every d)
and S2H with and without the validity test (LIM: some output of the tile can have d > W - x).  The right band is
restaged every 32 disparities.
"""
import guided_cost_ref as G

BAND = 32          # kBandChunk
TILE_H = 32        # kGuidedTileH
MAX_RADIUS = 7     # kMaxGuidedRadius
MAX_DISP = 256     # kMaxGuidedDisp


def tile_w(r):
    return 64 - 4 * r


def volume_shapes():
    """(r, W, H, D, texture class): guided_cost_ref.cost_shapes() with D two past the width (so d = W, valid at
    x = 0 alone, and d = W + 1, valid nowhere, are planes), or 256; for every radius a frame three tiles wide with
    few disparities, whose middle tile runs without the column mask and without the validity test; and the issue's
    odd cases."""
    out = []
    for r, W, H, _ in G.cost_shapes():
        out.append((r, W, H, min(W + 2, MAX_DISP), "art" if r % 2 == 0 else "step"))
    for r in range(MAX_RADIUS + 1):
        out.append((r, 3 * tile_w(r) + 5, 9, 8, "fuzz"))
    out += [
        (1, 45, 33, 64, "synth"),      # no multiple of the tile, W < D
        (2, 61, 35, 1, "art"),         # D = 1
        (3, 64, 8, 256, "binary"),     # D = 256, a frame lower than a tile
        (0, 70, 33, 40, "bright"),     # r = 0, a second tile row of one row
        (MAX_RADIUS, 40, 34, 33, "step"),   # the largest radius the slice call takes, one restage
    ]
    return out


def tile_paths(r, W, H, D):
    """The set of (nomask, lim, restaged) over the tiles of a frame: the volume kernel's selection, restated."""
    TW = tile_w(r)
    tiles_x, tiles_y = (W + TW - 1) // TW, (H + TILE_H - 1) // TILE_H
    assert tiles_y >= 1
    paths = set()
    for tx in range(tiles_x):
        x0 = tx * TW
        px0 = x0 - 2 * r
        nomask = px0 >= D - 1 and px0 >= 0 and px0 + 63 < W
        lim = D - 1 > W - (x0 + TW - 1)
        paths.add((nomask, lim, D > BAND))
    return paths
