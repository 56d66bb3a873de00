"""CPU model of where bm_box_mfma.hip ends a tile's disparity range at the left edge of the frame.

Under valid_mode 0 a staged column c < d contributes AD = 0, so for an output column x every d >= x + R + 1 has its
whole window left of d: cost 0, key (0 << 8) | d.  In a slice [d_lo, d_hi) the first such disparity of column x is
max(x + R + 1, d_lo); it beats every later one (same cost, smaller low byte).  With x_max = min(x0 + TOX, W) - 1 the
tile's last output column, no disparity past max(x_max + R + 1, d_lo) can change a key of the tile, and its range is
    d_end = min(d_hi, W - x0 + 1, max(x_max + R + 1, d_lo) + 1).
The split is restated here with its own wave_split and proved against oracle.box_disp and oracle.box_keys_slice: for
every tile, the columns [x0, x_max] of the whole range's result equal the result of the range cut at the tile's d_end,
maps and keys.  passes() counts the loop passes of a launch in the old and the new split: the predicted fall of the
MFMA count (48 per pass of the paired loop)."""
import numpy as np
import pytest

from oracle import oracle as O

T, WAVES = 64, 4
TOY = 48                      # rows of a paired-loop tile


def none_key(r):
    """A slice key with no valid disparity: the seed, (50 per window pixel) << 8 (Device.cu:37's start value)."""
    return (50 * (2 * r + 1) ** 2) << 8


WS, HS, RS, DS = (70, 100, 140, 230), (20, 40), (1, 3, 5, 7), (64, 128, 256)
KINDS = ("random", "flat_left")


def geometry(r, d_lo, d_hi):
    """(NP, TOX) by launch_rd's rule and MG: one d per pass on 64 - 2r columns for ranges of at most 32 at r <= 2."""
    NP = 1 if (r <= 2 and d_hi - d_lo <= 32) else 2
    return NP, (T - 2 * r if (NP == 1 or r <= 6) else 48)


def left_bound(W, r, d_lo, d_hi, x0):
    """x_max + r + 1: the first disparity whose window lies left of d for every output column of the tile."""
    _, TOX = geometry(r, d_lo, d_hi)
    return min(x0 + TOX, W) - 1 + r + 1


def tile_d_end(W, r, d_lo, d_hi, x0, left_rule=True):
    """The end of the tile's range: d <= W - x0 on the right, and with the left rule the one zero-cost pass."""
    d_end = min(d_hi, W - x0 + 1)
    return min(d_end, max(left_bound(W, r, d_lo, d_hi, x0), d_lo) + 1) if left_rule else d_end


def wave_split(W, r, d_lo, d_hi, x0, wave, left_rule=True):
    """(dw_lo, dw_m, dw_hi, d_m) of one wave of the tile at x0, by the kernel's arithmetic."""
    NP, TOX = geometry(r, d_lo, d_hi)
    nd = max(tile_d_end(W, r, d_lo, d_hi, x0, left_rule) - d_lo, 0)
    lo, hi = d_lo + (wave * nd) // WAVES, d_lo + ((wave + 1) * nd) // WAVES
    d_free = W - (min(x0 + TOX, W) - 1)
    d_m = d_lo if x0 - r + T > W else max(min(x0 - r, d_free) + 1, d_lo)
    n_free = max(min(hi, d_m) - lo, 0)
    return lo, lo + n_free - n_free % NP, hi, d_m


def passes(W, H, r, d_lo, d_hi, batch=1, left_rule=True):
    """(unmasked, masked) loop passes of all waves of a launch."""
    NP, TOX = geometry(r, d_lo, d_hi)
    toy = TOY if NP == 2 else T - 2 * r
    free = masked = 0
    for x0 in range(0, W, TOX):
        for wave in range(WAVES):
            lo, m, hi, _ = wave_split(W, r, d_lo, d_hi, x0, wave, left_rule)
            free += (m - lo) // NP
            masked += (hi - m + NP - 1) // NP
    rows = -(-H // toy) * batch
    return free * rows, masked * rows


def tiles(W, r, d_lo, d_hi):
    _, TOX = geometry(r, d_lo, d_hi)
    return [(x0, min(x0 + TOX, W) - 1) for x0 in range(0, W, TOX)]


def pair(kind, W, H, seed):
    """random: independent uniform frames of values below 64, so that a window costs about 21 per pixel, under the
    seed's 50: every key is a real cost and the disparities below the bound compete with the zero-cost one.
    flat_left: the left 20 columns of both frames are zero as well, so several disparities tie at cost 0 below
    x + r + 1 too."""
    rng = np.random.default_rng(seed)
    L = rng.integers(0, 64, (H, W), dtype=np.uint8)
    R = rng.integers(0, 64, (H, W), dtype=np.uint8)
    if kind == "flat_left":
        L[:, :20] = 0
        R[:, :20] = 0
    return L, R


def slices_of(W, r):
    """The d-slices of a (W, r) row of the table: around the left bound b of the first and the second tile, on either
    side of it and on it, odd and even lengths, and slices of at most 32 disparities, which r <= 2 runs one d per pass."""
    out = []
    for x0, _ in tiles(W, r, 0, 128)[:2]:
        b = left_bound(W, r, 0, 128, x0)
        out += [(b - 9, b + 30), (b - 4, b + 40), (b, b + 33), (b, b + 40), (b + 3, b + 44), (b + 6, b + 43),
                (b - 5, b + 20), (b, b + 24), (b + 2, b + 31)]
    return [(lo, hi) for lo, hi in out if 0 <= lo and hi <= 256]


def cases_of(W, r, d_lo, d_hi):
    """The names of the rule's cases that the row of tiles of (W, r, [d_lo, d_hi)) runs."""
    c = {"d_lo = 0"} if d_lo == 0 else set()
    if d_lo == 0 and W < d_hi:
        c.add("W < D")
    c.add("NP = %d" % geometry(r, d_lo, d_hi)[0])
    for x0, _ in tiles(W, r, d_lo, d_hi):
        b = left_bound(W, r, d_lo, d_hi, x0)
        old, new = tile_d_end(W, r, d_lo, d_hi, x0, False), tile_d_end(W, r, d_lo, d_hi, x0)
        if new >= old:
            c.add("uncut")
            continue
        c.add("cut")
        c.add("d_lo < bound" if d_lo < b else "d_lo = bound" if d_lo == b else "d_lo > bound")
        if d_lo >= b:
            assert new - d_lo == 1              # exactly one pass runs, in wave 3
            assert [wave_split(W, r, d_lo, d_hi, x0, w)[2] - wave_split(W, r, d_lo, d_hi, x0, w)[0]
                    for w in range(WAVES)] == [0, 0, 0, 1]
        c.add("odd length" if (new - d_lo) % 2 else "even length")
        if any(lo < m < hi for lo, m, hi, _ in (wave_split(W, r, d_lo, d_hi, x0, w) for w in range(WAVES))):
            c.add("free and masked in one wave")
    return c


def test_the_table_holds_every_case():
    c = set()
    for W in WS:
        for r in RS:
            for D in DS:
                c |= cases_of(W, r, 0, D)
            for d_lo, d_hi in slices_of(W, r):
                c |= {"slice: " + n for n in cases_of(W, r, d_lo, d_hi)}
    # (from d_lo = 0 a cut tile is a whole one, and x_max + r + 2 is even for every tile width: odd lengths are the
    # slices')
    want = {"d_lo = 0", "W < D", "cut", "uncut", "d_lo < bound", "even length", "NP = 2",
            "free and masked in one wave"}
    want |= {"slice: " + n for n in ("cut", "uncut", "d_lo < bound", "d_lo = bound", "d_lo > bound", "odd length",
                                     "even length", "NP = 1", "NP = 2")}
    assert want <= c, want - c


@pytest.mark.parametrize("r", RS)
def test_split_covers_the_cut_range(r):
    """The waves' ranges tile [d_lo, d_end) in order, whole passes below d_m; d_end never passes the old end, keeps
    at least one disparity where the old range had one, and no R column of a pass leaves the staged band."""
    for d_lo, d_hi in [(0, D) for D in DS] + [(0, 24), (0, 32), (60, 92), (70, 100), (7, 8), (33, 70), (100, 141)]:
        NP, TOX = geometry(r, d_lo, d_hi)
        DMAX = next(m for m in (64, 128, 192, 256) if d_hi - d_lo <= m)
        for W in range(60, 261):
            for x0, x_max in tiles(W, r, d_lo, d_hi):
                old, new = tile_d_end(W, r, d_lo, d_hi, x0, False), tile_d_end(W, r, d_lo, d_hi, x0)
                assert new <= old and (new > d_lo) == (old > d_lo), (W, x0, old, new)
                assert new == old or new == max(x_max + r + 1, d_lo) + 1
                at = d_lo
                for wave in range(WAVES):
                    lo, m, hi, d_m = wave_split(W, r, d_lo, d_hi, x0, wave)
                    assert lo == at and lo <= m <= hi and (m - lo) % NP == 0 and m <= max(d_m, lo)
                    at = hi
                    # staged band column of lane column k at disparity d: k + DMAX + d_lo - d, k = 0..63; the odd last
                    # pass repeats its d
                    for d in (lo, hi - 1) if hi > lo else ():
                        assert 0 <= DMAX + d_lo - d and 63 + DMAX + d_lo - d < T + DMAX
                assert at == max(new, d_lo)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("r", RS)
@pytest.mark.parametrize("W", WS)
def test_cut_range_gives_the_whole_range_s_maps_and_keys(W, r, kind):
    for H in HS:
        L, R = pair(kind, W, H, 1000 * W + 10 * r + H)
        for D in DS:
            want, want_keys = O.box_disp(L, R, r, D, want_keys=True)
            for x0, x_max in tiles(W, r, 0, D):
                d_end = tile_d_end(W, r, 0, D, x0)
                assert d_end >= 1
                got, got_keys = O.box_disp(L, R, r, d_end, want_keys=True)
                assert np.array_equal(got[:, x0:x_max + 1], want[:, x0:x_max + 1]), (H, D, x0, d_end)
                assert np.array_equal(got_keys[:, x0:x_max + 1], want_keys[:, x0:x_max + 1]), (H, D, x0, d_end)
            if kind == "flat_left":
                # the left strip ties at cost 0 from d = 0 on: d = 0 wins; right of it the rule's own disparity
                # x + r + 1 is the first with cost 0 wherever no smaller d happens to cost 0
                assert (want_keys[:, :20 - r] == 0).all()


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("r", RS)
@pytest.mark.parametrize("W", WS)
def test_cut_slices_give_the_whole_slice_s_keys(W, r, kind):
    H = HS[0]
    L, R = pair(kind, W, H, 2000 * W + 10 * r)
    for d_lo, d_hi in slices_of(W, r):
        want = O.box_keys_slice(L, R, r, d_lo, d_hi)
        for x0, x_max in tiles(W, r, d_lo, d_hi):
            d_end = tile_d_end(W, r, d_lo, d_hi, x0)
            if d_end <= d_lo:        # the right-hand rule left the tile nothing: no key in the whole range either
                assert (want[:, x0:x_max + 1] == none_key(r)).all(), (d_lo, d_hi, x0)
                continue
            got = O.box_keys_slice(L, R, r, d_lo, d_end)
            assert np.array_equal(got[:, x0:x_max + 1], want[:, x0:x_max + 1]), (d_lo, d_hi, x0, d_end)
            b = left_bound(W, r, d_lo, d_hi, x0)
            if d_lo >= b and d_end < min(d_hi, W - x0 + 1):
                # the one pass that runs: cost 0 at d_lo for every column that d_lo is valid for
                valid = np.arange(x0, x_max + 1) <= W - d_lo
                assert (want[:, x0:x_max + 1][:, valid] == d_lo).all()


def test_left_strip_reads_the_rule_s_disparity():
    """Random frames, D = 128: an output column x < D - r - 1 whose smaller disparities all cost something takes
    d = x + r + 1 at cost 0 (then the map's threshold keeps it); the keys say so."""
    for W, H, r, D in [(140, 40, 5, 128), (100, 30, 1, 128), (130, 30, 7, 128), (90, 30, 3, 64)]:
        L, R = pair("random", W, H, W + r)
        L |= 1                      # with R even below, |L - R| >= 1 everywhere: no accidental zero cost
        R &= 0xFE
        _, keys = O.box_disp(L, R, r, D, want_keys=True)
        xs = np.arange(min(W, D - r - 1))
        xs = xs[xs + r + 1 <= W - xs]          # d = x + r + 1 is valid for x
        assert len(xs) and (keys[:, xs] == (xs + r + 1)[None, :]).all()


def test_headline_prediction():
    """1920 x 1080, r = 5, D = 128, 128 frames: the tiles at x0 = 0 and 54 stop at d = 60 and 114, 82 of the 4468
    disparities a row of 36 tiles walks (34 x 128 + 85 + 31).  In passes of two, rounded up per wave, a row falls from
    2236 (2055 unmasked + 181 masked) to 2198 (2055 + 143): -1.70 % of the passes and of the MFMAs, 48 per pass."""
    assert [tile_d_end(1920, 5, 0, 128, x0) for x0 in (0, 54, 108)] == [60, 114, 128]
    old = sum(tile_d_end(1920, 5, 0, 128, x0, False) for x0, _ in tiles(1920, 5, 0, 128))
    new = sum(tile_d_end(1920, 5, 0, 128, x0) for x0, _ in tiles(1920, 5, 0, 128))
    assert (old, old - new) == (4468, 82)
    po, pn = passes(1920, 1080, 5, 0, 128, 128, False), passes(1920, 1080, 5, 0, 128, 128)
    rows = 23 * 128
    assert po == (2055 * rows, 181 * rows) and pn == (2055 * rows, 143 * rows)
    assert 48 * sum(po) == 315973632 and 48 * sum(pn) == 310603776
