"""CPU model of what bm_box_mfma.hip's paired loop carries from pass to pass once the masked passes run in the same
slot order as the unmasked ones.  One body walks [lo, mid) unmasked and [mid, hi) masked and keeps, in
scalars and one address, what run() rebuilds in every pass from the disparities themselves:

  wd, c0s   W - d and x0 - R - d, - 2 per masked pass: the AD mask of column block cb and disparity p is
            (uint32)(l16 + c0s + 16 cb - p one) < (uint32)(wd - p one), `one` = 1 where p = 1 is d + 1 and 0 where it
            repeats d (the odd last pass)
  e4        4 (wd - x0 - 16 xb) - 16 g, one operand for both disparities: element i of output block xb keeps its key
            constant where 4 (i + p one) <= e4
  col       p = 0's staged R column, - 2 per pass; p = 1 reads col - one.  After the last R read of a pass the
            addresses step to the next pass's, across the hand-over from the unmasked loop to the masked one as well;
            the last pass of the range does not step (nothing reads its addresses, and they stay in the band)

Restated here from the kernel and checked by brute force against run()'s per-pass formulas and against the columns
themselves, for every tile and wave of W = 60..260, r = 1..7 and the d ranges of the masks model."""
import numpy as np
import pytest

from test_box_mfma_masks_model import RANGES, T, WAVES, geometry, loop_passes, wave_split


def dmax_of(d_lo, d_hi):
    """launch_r's d_max template argument: the span rounded up to 64."""
    return 64 * ((d_hi - d_lo + 63) // 64)


def paired_trace(W, r, d_lo, d_hi, x0, wave):
    """Every pass of run_paired for one wave of the tile at x0, with the carried values as the kernel steps them:
    dicts of masked, d, one, wd, c0s (None in unmasked passes), cols = the staged R columns of lane 0 read for
    p = 0, 1, and ahead = the columns the pass's address step leaves for the pass that follows."""
    lo, mid, hi, _ = wave_split(W, r, d_lo, d_hi, x0, wave)
    DMAX = dmax_of(d_lo, d_hi)
    col = DMAX + d_lo - lo                                  # rcol / kColB without the lane's l16
    cols = (col, col - (1 if lo + 1 < hi else 0))           # raddr_at(rcol, lo)
    wd, c0s = W - mid, x0 - r - mid
    out = []
    for masked, a, b in ((False, lo, mid), (True, mid, hi)):
        for d in range(a, b, 2):
            one = 1 if d + 1 < hi else 0
            here = cols
            col -= 2 if d + 2 < hi else 0                   # step_addr
            cols = (col, col - (1 if d + 3 < hi else 0))    # raddr_at(rcol, d + 2)
            out.append(dict(masked=masked, d=d, one=one, wd=wd if masked else None, c0s=c0s if masked else None,
                            cols=here, ahead=cols))
            if masked:
                wd -= 2
                c0s -= 2
    return out, (lo, mid, hi, DMAX)


def paired_tiles(W, r, d_lo, d_hi):
    NP, TOX = geometry(r, d_lo, d_hi)
    assert NP == 2
    return range(0, W, TOX)


def shape_stats(W, r, d_lo, d_hi):
    """Counts over one row of tiles: passes, masked passes, waves whose masked range is odd, waves that run both
    loops (a hand-over), waves whose whole range is masked."""
    s = dict(passes=0, masked=0, odd_masked=0, handovers=0, all_masked=0, waves=[])
    for x0 in paired_tiles(W, r, d_lo, d_hi):
        for wave in range(WAVES):
            tr, (lo, mid, hi, _) = paired_trace(W, r, d_lo, d_hi, x0, wave)
            s["passes"] += len(tr)
            s["masked"] += sum(p["masked"] for p in tr)
            s["odd_masked"] += (hi - mid) % 2
            s["handovers"] += lo < mid < hi
            s["all_masked"] += lo == mid < hi
            s["waves"].append((x0, wave, lo, mid, hi))
    return s


PAIRED_RANGES = [rg for rg in RANGES]


@pytest.mark.parametrize("r", range(1, 8))
def test_carried_mask_operands_and_columns(r):
    """(a) the stepped operands equal run()'s per-pass formulas, the odd last pass included; (b) every pass reads the
    columns of its own disparities, the stepped addresses are the next pass's (also where the unmasked loop hands
    over to the masked one), and those a range's last pass leaves lie in [0, RC): reads issued from them ahead of the
    next pass (measured and not kept) would stay inside the band."""
    seen = dict(odd=0, handover=0, last=0)
    for d_lo, d_hi in PAIRED_RANGES:
        if geometry(r, d_lo, d_hi)[0] != 2:
            continue                                        # one d per pass: run(), unchanged
        for W in range(60, 261):
            for x0 in paired_tiles(W, r, d_lo, d_hi):
                for wave in range(WAVES):
                    tr, (lo, mid, hi, DMAX) = paired_trace(W, r, d_lo, d_hi, x0, wave)
                    RC = T + DMAX
                    assert hi - d_lo <= DMAX
                    dds = loop_passes(lo, mid, 2) + loop_passes(mid, hi, 2)
                    assert [p["d"] for p in tr] == [dd[0] for dd in dds]
                    for k, (p, dd) in enumerate(zip(tr, dds)):
                        assert dd[1] == dd[0] + p["one"]
                        # (b) lane l16 of column block cb reads col + l16 + 16 cb = l16 + 16 cb + DMAX + d_lo - dd[p]
                        assert p["cols"] == (DMAX + d_lo - dd[0], DMAX + d_lo - dd[1]), (W, x0, wave, p)
                        if k + 1 < len(tr):
                            assert p["ahead"] == tr[k + 1]["cols"]
                            seen["handover"] += (not p["masked"]) and tr[k + 1]["masked"]
                        else:
                            # read by nobody: lanes 0..15 of chunk 0 of column block 0
                            assert 0 <= min(p["ahead"]) and max(p["ahead"]) + 15 < RC, (W, x0, wave, p)
                            assert p["ahead"] == (p["cols"][0], p["cols"][0])
                            seen["last"] += 1
                        if not p["masked"]:
                            assert p["one"] == 1
                            continue
                        seen["odd"] += p["one"] == 0
                        # (a) run(): c0 = x0 - R + 16 cb - dd[p] against W - dd[p]; e = W - x0 - 16 xb - dd[p] - 4 g
                        for q in range(2):
                            assert p["c0s"] - q * p["one"] == x0 - r - dd[q]
                            assert p["wd"] - q * p["one"] == W - dd[q]
                    if not tr:
                        # an empty range still forms its first addresses
                        assert 0 <= DMAX + d_lo - lo and DMAX + d_lo - lo + 15 < RC
    assert min(seen.values()) > 0, seen


def test_mask_forms_equal_the_direct_conditions():
    """The two per-lane forms for every operand value the loops above can produce: the AD mask's one unsigned compare
    is d <= c < W, and the key mask's shared operand e4 with the constants 4 (i + one) is i <= e of run(), for
    p = 0 and p = 1, with `one` = 1 and in the odd last pass."""
    l16 = np.arange(16)[None, None, :]
    c0 = np.arange(-330, 330)[:, None, None]                # x0 - R + 16 cb - d
    wdv = np.arange(0, 331)[None, :, None]                  # W - d >= 0: d <= W in every pass
    form = (l16 + c0).astype(np.int64).astype(np.uint32) < wdv.astype(np.uint32)
    # with c = l16 + c0 + d the staged column: d <= c < W
    assert np.array_equal(form, (l16 + c0 >= 0) & (l16 + c0 < wdv))
    s = np.arange(-330, 331)[:, None, None, None, None]     # wd - x0 - 16 xb = W - x0 - 16 xb - d
    g = np.arange(4)[None, :, None, None, None]
    i = np.arange(4)[None, None, :, None, None]
    q = np.arange(2)[None, None, None, :, None]             # p
    one = np.arange(2)[None, None, None, None, :]
    e4 = 4 * s - 16 * g
    form = 4 * (i + q * one) <= e4
    # run(): e = (W - x0 - 16 xb - dd[p]) - 4 g with dd[p] = d + p one; valid where i <= e
    assert np.array_equal(form, i <= (s - q * one) - 4 * g)
    # and that is the output column's own rule, d' <= W - x with x = x0 + 16 xb + 4 g + i
    assert np.array_equal(form, (4 * g + i) + q * one <= s)


def test_odd_last_pass_label_loses():
    """(c) the repeated disparity of an odd last pass carries the label d + 1: its key is greater than the key (c, d)
    of p = 0 as an integer and as the f32 bit pattern the min runs on, for every cost up to (2r+1)^2 255 at r = 7
    (which covers the smaller radii) and every d up to 255; at d = 255 the carry goes into the cost."""
    c = np.arange(0, 15 * 15 * 255 + 1, dtype=np.int64)[:, None]
    d = np.arange(256, dtype=np.int64)[None, :]
    key, lab = (c << 8) + d, (c << 8) + d + 1
    assert lab.max() < 1 << 24                              # exact in f32
    kf, lf = key.astype(np.float32), lab.astype(np.float32)
    assert np.array_equal(kf.astype(np.int64), key) and np.array_equal(lf.astype(np.int64), lab)
    assert (lf.view(np.uint32) > kf.view(np.uint32)).all()
    assert np.array_equal(lab[:, 255], (c[:, 0] + 1) << 8)
    # min3(best, key, label) is min(best, key)
    assert np.array_equal(np.minimum(kf.view(np.uint32), lf.view(np.uint32)), kf.view(np.uint32))


def test_gpu_test_shapes_hit_their_cases():
    """The shapes of tests/test_gpu_box_mfma_masked_order.py, by the kernel's own arithmetic."""
    s = shape_stats(230, 5, 0, 128)
    assert (s["masked"], s["passes"], s["odd_masked"], s["handovers"]) == (168, 235, 7, 4)
    s = shape_stats(230, 5, 1, 128)
    assert (s["odd_masked"], s["handovers"]) == (10, 5)
    s = shape_stats(262, 5, 4, 256)
    assert (0, 3, 193, 193, 256) in s["waves"]
    s = shape_stats(80, 5, 0, 128)
    assert s["masked"] == s["passes"] > 0 and s["handovers"] == 0
    s = shape_stats(230, 5, 40, 90)
    assert (s["odd_masked"], s["handovers"]) == (9, 3)
