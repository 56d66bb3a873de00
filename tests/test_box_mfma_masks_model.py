"""CPU model of how bm_box_mfma.hip places its edge masks.  A tile needs AD = 0 for staged columns
with c < d or c >= W, and no key for output columns with d > W - x; both conditions are monotone in d, so each
wave walks the disparities below d_m (the tile's first disparity that needs either) in the unmasked loop, in whole
passes, and the rest of its range in the masked loop.  Restated here and checked by brute force over the columns;
then the two mask forms in the kernel's number formats: an AD register ANDed with 0 instead of 0x7FFF7FFF, and a
stage-2 accumulator started from +inf."""
import numpy as np
import pytest

import test_box_mfma_model as M

T, WAVES = 64, 4


def geometry(r, d_lo, d_hi):
    """(NP, TOX) by launch_rd's rule and MG: one d per pass on 64 - 2r columns for ranges of at most 32 at r <= 2."""
    NP = 1 if (r <= 2 and d_hi - d_lo <= 32) else 2
    return NP, (T - 2 * r if (NP == 1 or r <= 6) else 48)


def wave_split(W, r, d_lo, d_hi, x0, wave):
    """(dw_lo, dw_m, dw_hi, d_m) of one wave of the tile at x0, by the kernel's arithmetic."""
    NP, TOX = geometry(r, d_lo, d_hi)
    d_end = min(d_hi, W - x0 + 1)
    nd = max(d_end - d_lo, 0)
    lo, hi = d_lo + (wave * nd) // WAVES, d_lo + ((wave + 1) * nd) // WAVES
    d_free = W - (min(x0 + TOX, W) - 1)
    d_m = d_lo if x0 - r + T > W else max(min(x0 - r, d_free) + 1, d_lo)
    n_free = max(min(hi, d_m) - lo, 0)
    return lo, lo + n_free - n_free % NP, hi, d_m


def loop_passes(lo, hi, NP):
    """The disparities of every pass of one loop over [lo, hi): the second one clamped to the loop's own end."""
    return [[d] if NP == 1 else [d, min(d + 1, hi - 1)] for d in range(lo, hi, NP)]


RANGES = [(0, 24), (0, 32), (0, 40), (0, 128), (0, 256), (7, 8), (3, 20), (5, 37), (16, 40), (33, 70), (60, 190),
          (100, 141)]


@pytest.mark.parametrize("r", range(1, 8))
def test_unmasked_part_needs_no_mask_and_the_parts_cover_the_range(r):
    for d_lo, d_hi in RANGES:
        NP, TOX = geometry(r, d_lo, d_hi)
        for W in range(60, 261):
            for x0 in range(0, W, TOX):
                staged = x0 - r + np.arange(T)                    # image columns of the staged tile
                outs = np.arange(x0, min(x0 + TOX, W))            # output columns the tile writes
                d_end = min(d_hi, W - x0 + 1)
                ds = np.arange(d_lo, max(d_end, d_lo))
                # brute force: does disparity d need a mask anywhere in this tile?
                need = ((staged[None, :] < ds[:, None]) | (staged[None, :] >= W)).any(1) | \
                       (ds[:, None] > W - outs[None, :]).any(1)
                for wave in range(WAVES):
                    lo, m, hi, d_m = wave_split(W, r, d_lo, d_hi, x0, wave)
                    assert d_lo <= lo <= m <= hi <= max(d_end, d_lo) and (m - lo) % NP == 0
                    assert not need[lo - d_lo:m - d_lo].any(), (W, x0, wave, lo, m, hi)
                    # d_m is the first disparity that needs a mask, and the masked part takes at most the one
                    # maskless disparity that does not fill a pass
                    assert d_m == d_lo or not need[d_m - 1 - d_lo:d_m - d_lo].any()
                    assert d_m >= d_end or need[d_m - d_lo], (W, x0, d_m)
                    assert 0 <= min(hi, max(d_m, lo)) - m < NP, (W, x0, wave, lo, m, hi)
                    free, masked = loop_passes(lo, m, NP), loop_passes(m, hi, NP)
                    assert all(lo <= d < m for p in free for d in p) and all(m <= d < hi for p in masked for d in p)
                    seen = [d for p in free + masked for d in p]
                    # once each, in order, apart from the repeated last d of an odd masked part
                    twice = [hi - 1] if NP == 2 and (hi - m) % 2 else []
                    assert seen == list(range(lo, hi)) + twice, (W, x0, wave, lo, m, hi)


@pytest.mark.parametrize("r", [1, 5, 7])
def test_and_with_zero_is_the_masked_ad(r):
    """keep = 0x7FFF or 0 per staged column in the AND that clears the sign gives the model's masked AD operand bit
    for bit (+0, not -0 or a stale value), and a masked column's stage-1 sums are exactly -bias: it adds 0."""
    rng = np.random.default_rng(r)
    n = T - 2 * r - 9                                  # a frame narrower than the tile: columns past W
    L = rng.integers(0, 256, (n, n), dtype=np.uint8)
    R = rng.integers(0, 256, (n, n), dtype=np.uint8)
    for d in (0, 3, 17):
        Lh = np.full((T, T), 0x6400, np.uint16)
        Rh = np.full((T, T), 0x6400, np.uint16)
        Lh[r:r + n, r:r + n] |= L
        # what the kernel stages: R at column c - d, zero outside the image; no knowledge of the mask
        for c in range(-r, T - r):
            if 0 <= c - d < n:
                Rh[r:r + n, r + c] |= R[:, c - d]
        diff = (Lh.view(np.float16) - Rh.view(np.float16)).view(np.uint16)
        cols = np.arange(T) - r
        raw = (diff & 0x7FFF).view(np.float16)
        assert d == 0 or (raw[:, cols >= n].any() and raw[:, (cols >= 0) & (cols < d)].any()), "nothing to clear"
        keep = np.where((cols >= d) & (cols < n), 0x7FFF, 0).astype(np.uint16)
        ad = (diff & keep[None, :]).view(np.float16)
        want = M._ad_tile(L, R, r, d)
        assert np.array_equal(ad.view(np.uint16), want.view(np.uint16))
        d1 = M._stage1(ad, r, np.arange(32), False)
        assert (d1[:, keep == 0] == -float(M._bias(r))).all()


@pytest.mark.parametrize("r", [1, 5, 7])
def test_stage2_from_inf_stays_inf(r):
    """Stage 2 with +inf in the C operand of the invalid output columns: finite partial sums in the model test's three
    summation orders leave the accumulator at bit pattern 0x7F800000, and the other columns hold their keys."""
    rng = np.random.default_rng(10 + r)
    n = T - 2 * r
    L, R = M._frames("random" if r != 7 else "hi_lo", n, rng)
    d = 7
    kpos = np.array([4 * g + j if j < 4 else 16 + 4 * g + (j - 4) for g in range(4) for j in range(8)])
    m = np.arange(16)
    c = np.float32(256 * (2 * r + 1) * M._bias(r) + d)
    for i, order in enumerate(M._orders(32, rng)):
        tree = i == 2
        d1 = M._stage1(M._ad_tile(L, R, r, d), r, order, tree)
        keys = M._stage2(d1, r, d, order, tree)
        d1p = np.concatenate([d1, np.zeros((T, 16), np.float16)], axis=1)
        for xb in range(4):
            for first_bad in (0, 1, 9, 15):                      # output columns first_bad.. of the block invalid
                bad = m >= first_bad
                acc = np.where(bad, np.float32(np.inf), c)[None, :].repeat(T, 0).astype(np.float32)
                prods = []
                for kk in order:
                    xin = kpos[kk]
                    band = np.where((xin - m >= 0) & (xin - m <= 2 * r), np.float16(256), np.float16(0))
                    prods.append(band[None, :].astype(np.float32) * d1p[:, 16 * xb + xin][:, None].astype(np.float32))
                assert all(np.isfinite(p).all() for p in prods)
                if tree:
                    s = np.zeros((T, 16), np.float32)
                    for p in prods:
                        s = (s + p).astype(np.float32)
                    assert np.isfinite(s).all()
                    acc = (acc + s).astype(np.float32)
                else:
                    for p in prods:
                        acc = (acc + p).astype(np.float32)
                bits = acc.view(np.uint32)
                assert (bits[:, bad] == 0x7F800000).all()
                assert np.array_equal(acc[:, ~bad].astype(np.uint32), keys[:, 16 * xb:16 * xb + 16][:, ~bad])
                # the min on raw bits: +inf never beats a key
                assert (bits[:, bad] > keys.max()).all()
