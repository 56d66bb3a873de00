"""CPU model of how a workgroup of bm_box_mfma.hip walks a range of tiles and keeps the right band along a row of
tiles.  Workgroup k of n takes the tiles [k T / n, (k + 1) T / n) of the sequence [frame][ty][tx]; when
the next tile of its range is the right-hand neighbour, it moves the RC - TOX band columns both tiles share down by
TOX columns and stages only the new ones, in whole 4-column groups from column NEW0 = (RC - TOX) & ~3 on, with the
left tile in the same pass.  Restated here by the kernel's own arithmetic and checked by brute force: the split
takes every tile once and in order, a carried band equals a fresh staging of that tile column for column and 16-byte
unit for unit (the XOR swizzle of each side applied separately), row and frame changes restage, and the straight-line
staging path is taken only where every byte it loads lies inside the image."""
import numpy as np
import pytest

from test_box_mfma_masks_model import RANGES, T, geometry

THREADS = 256
OUTSIDE = -1    # a staged column left of 0 or past W: stages 0


def dims(r, d_lo, d_hi):
    """(NP, TOX, TOY, DMAX, RC, KEEP, NEW0, NEW4, MOVE_U) by launch_r / launch_rd and MG."""
    NP, TOX = geometry(r, d_lo, d_hi)
    TOY = T - 2 * r if NP == 1 else 48
    DMAX = next(d for d in (64, 128, 192, 256) if d_hi - d_lo <= d)
    RC = T + DMAX
    KEEP = RC - TOX
    NEW0 = KEEP & ~3
    return NP, TOX, TOY, DMAX, RC, KEEP, NEW0, (RC - NEW0) // 4, -(-KEEP * 8 // THREADS)


def walk(tiles_x, tiles_y, batch, n):
    """Every workgroup's tiles as (tile, frame, ty, tx, carried), by the kernel's loop: the first tile decomposed
    by division, the following ones by stepping tx, ty and frame."""
    total = tiles_x * tiles_y * batch
    out = []
    for k in range(n):
        t_begin, t_end = k * total // n, (k + 1) * total // n
        if t_begin >= t_end:
            out.append([])
            continue
        tiles = tiles_x * tiles_y
        frame = t_begin // tiles
        ty = (t_begin - frame * tiles) // tiles_x
        tx = t_begin - frame * tiles - ty * tiles_x
        carried, mine = False, []
        tile = t_begin
        while True:
            mine.append((tile, frame, ty, tx, carried))
            if tile + 1 == t_end:
                break
            carried = tx + 1 < tiles_x
            tx += 1
            if tx == tiles_x:
                tx = 0
                ty += 1
                if ty == tiles_y:
                    ty = 0
                    frame += 1
            tile += 1
        out.append(mine)
    return out


def _grids():
    """The distinct (tiles_x, tiles_y) of W = 60..260, H in (40, 50, 100, 130), r = 1..7 and both loop forms."""
    g = set()
    for r in range(1, 8):
        for d_lo, d_hi in ((0, 24), (0, 128)):
            _, TOX, TOY = dims(r, d_lo, d_hi)[:3]
            for W in range(60, 261):
                for H in (40, 50, 100, 130):
                    g.add((-(-W // TOX), -(-H // TOY)))
    return sorted(g)


def test_every_tile_once_in_order_and_restage_on_row_and_frame_changes():
    grids = _grids()
    assert (1, 1) in grids and max(g[0] for g in grids) >= 5 and max(g[1] for g in grids) >= 3
    for tiles_x, tiles_y in grids:
        for batch in (1, 2, 3):
            total = tiles_x * tiles_y * batch
            for n in range(1, total + 2):
                w = walk(tiles_x, tiles_y, batch, min(n, total))     # the launcher clamps n to the tile count
                flat = [t for mine in w for t in mine]
                assert [t[0] for t in flat] == list(range(total)), (tiles_x, tiles_y, batch, n)
                for mine in w:
                    assert n > total or len(mine) in (total // n, total // n + 1)
                    for i, (tile, frame, ty, tx, carried) in enumerate(mine):
                        assert (frame, ty, tx) == (tile // (tiles_x * tiles_y), tile // tiles_x % tiles_y,
                                                   tile % tiles_x)
                        # carried exactly when the workgroup's previous tile is the left-hand neighbour
                        left = i > 0 and mine[i - 1][1:4] == (frame, ty, tx - 1)
                        assert carried == left, (tiles_x, tiles_y, batch, n, tile)
                        assert not (carried and tx == 0)
                if n >= total:
                    assert not any(t[4] for t in flat)               # one tile per workgroup: nothing carried


def test_split_in_64_bit():
    """k T / n with T and n near 2^31 / 4: the product needs 64 bits, as the kernel computes it."""
    total, n = 0x7FFFFFFF, 768
    assert (n - 1) * total > 2 ** 31
    ends = [(k + 1) * total // n for k in range(n)]
    assert ends[-1] == total and all(b > a for a, b in zip(ends, ends[1:]))


def slot(col, q):
    """bm_box_mfma.hip's slot(), in 16-byte units."""
    return col * 8 + (q ^ ((col >> 1) & 7))


def fresh_band(x0, r, d_lo, DMAX, RC, W):
    """image column of every staged right column of the tile at x0 (OUTSIDE: stages 0)."""
    c = x0 - r - d_lo - DMAX + np.arange(RC)
    return np.where((c >= 0) & (c < W), c, OUTSIDE)


def fresh_left(x0, r, W):
    c = x0 - r + np.arange(T)
    return np.where((c >= 0) & (c < W), c, OUTSIDE)


def carry(band, x0_next, r, d_lo, W, dm):
    """the band of the tile at x0_next from its left neighbour's: move by TOX, stage the groups from NEW0 on."""
    NP, TOX, TOY, DMAX, RC, KEEP, NEW0, NEW4, MOVE_U = dm
    out = np.full(RC, -7)                      # -7: never written
    out[:KEEP] = band[TOX:]
    xr = x0_next - r - d_lo - DMAX + NEW0
    c = xr + np.arange(4 * NEW4)
    out[NEW0:NEW0 + 4 * NEW4] = np.where((c >= 0) & (c < W), c, OUTSIDE)
    return out


@pytest.mark.parametrize("r", range(1, 8))
def test_carried_band_is_the_fresh_band(r):
    for d_lo, d_hi in RANGES:
        dm = dims(r, d_lo, d_hi)
        NP, TOX, TOY, DMAX, RC, KEEP, NEW0, NEW4, MOVE_U = dm
        assert NEW0 % 4 == 0 and NEW0 <= KEEP < NEW0 + 4 and NEW0 + 4 * NEW4 == RC
        assert 8 * NEW4 + 8 * (T // 4) <= THREADS                   # one staging pass per carried tile
        assert (48 if NP == 2 else TOY) * (16 * (4 if TOX != 48 else 3) + 1) * 4 <= T * 128 + TOX * 128
        for W in range(60, 261):
            tiles_x = -(-W // TOX)
            band = fresh_band(0, r, d_lo, DMAX, RC, W)
            for tx in range(1, tiles_x):
                band = carry(band, tx * TOX, r, d_lo, W, dm)        # carried all the way along the row
                want = fresh_band(tx * TOX, r, d_lo, DMAX, RC, W)
                assert np.array_equal(band, want), (W, d_lo, d_hi, tx)
            # and from a fresh band at any tile of the row (a range that starts mid-row)
            for tx in range(1, tiles_x):
                got = carry(fresh_band((tx - 1) * TOX, r, d_lo, DMAX, RC, W), tx * TOX, r, d_lo, W, dm)
                assert np.array_equal(got, fresh_band(tx * TOX, r, d_lo, DMAX, RC, W))


@pytest.mark.parametrize("r", range(1, 8))
@pytest.mark.parametrize("d_lo,d_hi", [(0, 24), (0, 64), (0, 128), (40, 90), (0, 192), (0, 256)])
def test_move_by_units_with_both_swizzles(r, d_lo, d_hi):
    """The move as the threads do it: MOVE_U 16-byte units each, indices past the last unit clamped to it, all reads
    before all writes, source and destination slot() each with its own column's swizzle."""
    dm = dims(r, d_lo, d_hi)
    NP, TOX, TOY, DMAX, RC, KEEP, NEW0, NEW4, MOVE_U = dm
    assert (MOVE_U - 1) * THREADS < KEEP * 8 <= MOVE_U * THREADS
    lds = np.full(RC * 8, -1)
    for col in range(RC):
        for q in range(8):
            lds[slot(col, q)] = col * 8 + q                          # content: (column, row group) of the old band
    regs = {}
    for tid in range(THREADS):
        for i in range(MOVE_U):
            u = min(tid + i * THREADS, KEEP * 8 - 1)
            regs[tid, i] = lds[slot((u >> 3) + TOX, u & 7)]
    for tid in range(THREADS):
        for i in range(MOVE_U):
            u = min(tid + i * THREADS, KEEP * 8 - 1)
            lds[slot(u >> 3, u & 7)] = regs[tid, i]
    for col in range(KEEP):
        for q in range(8):
            assert lds[slot(col, q)] == (col + TOX) * 8 + q, (col, q)
    # the staging pass: thread -> (piece, row group, 4-column group), every element once, all inside the buffers
    seen = set()
    for tid in range(THREADS):
        NR = 8 * NEW4
        if tid >= NR + 8 * (T // 4):
            continue
        right = tid < NR
        el = tid - NR
        q = tid // NEW4 if right else el // (T // 4)
        j = tid - q * NEW4 if right else el - q * (T // 4)
        col = (NEW0 if right else 0) + 4 * j
        assert 0 <= q < 8 and 0 <= col and col + 4 <= (RC if right else T)
        seen.add((right, q, col))
    assert len(seen) == 8 * NEW4 + 8 * (T // 4)


@pytest.mark.parametrize("r", [1, 3, 5, 7])
def test_interior_path_only_where_every_byte_is_inside(r):
    for d_lo, d_hi in ((0, 24), (0, 128), (40, 90), (100, 141)):
        NP, TOX, TOY, DMAX, RC, KEEP, NEW0, NEW4, MOVE_U = dims(r, d_lo, d_hi)
        for W in (60, 108, 150, 217, 230, 260):
            for H in (50, 70, 130):
                taken = 0
                for ty in range(-(-H // TOY)):
                    for tx in range(1, -(-W // TOX)):
                        ytop, xl = ty * TOY - r, tx * TOX - r
                        xr = tx * TOX - r - d_lo - DMAX + NEW0
                        interior = (ytop >= 0 and ytop + T <= H and xr >= 0 and xl >= 0 and xl + T <= W and
                                    xr + 4 * NEW4 <= W)
                        rows = np.arange(ytop, ytop + T)
                        cols = np.concatenate([np.arange(xr, xr + 4 * NEW4), np.arange(xl, xl + T)])
                        inside = (rows >= 0).all() and (rows < H).all() and (cols >= 0).all() and (cols < W).all()
                        assert interior == inside, (W, H, ty, tx)
                        taken += interior
                if W == 260 and H == 130 and d_lo == 0:
                    assert taken > 0


def test_left_tile_is_always_staged_fresh():
    """The left tile is not carried: every tile stages its 64 columns from x0 - r."""
    W, r = 230, 5
    for tx in range(5):
        c = fresh_left(tx * 54, r, W)
        assert c[0] == (OUTSIDE if tx == 0 else tx * 54 - r) and (c[c != OUTSIDE] < W).all()
