"""CPU model of bm_box_mfma.hip's stage 1 on permuted rows: the 64 staged rows of a column lie in LDS so
that row group q = 4c + g (32-row chunk c, lane group g) holds the rows 32c + 4g + j (j < 4) and 32c + 16 + 4g + (j - 4)
(j >= 4).  A lane's two chunks are then eight dwords of which the dwords 2 ob .. 2 ob + 3 are the K = 32 operand of
output row block ob: K slot (g, j) is input row 16 ob + ko(g, j), ko = j < 4 ? 4g + j : 16 + 4g + (j - 4), the K order
of stage 2.  One band, 1.0 where 0 <= ko - n <= 2r, serves the three views; the fourth row block of the one-d-per-pass
kernels is the third view against a second band, 1.0 where 0 <= ko - 16 - n <= 2r.  Stated in numpy float16 / float32
and checked against test_box_mfma_model._stage1 (the aligned chunks with two MFMAs for the middle block) and against
the integer vertical sums, r = 1..7, L = 255 / R = 0, the reverse and random frames, three summation orders."""
import numpy as np
import pytest

import test_box_mfma_model as M

T = M.T


def staged_row(q, i):
    """the staged row that element i of 16-byte row group q holds"""
    return 32 * (q >> 2) + 4 * (q & 3) + (i if i < 4 else 12 + i)


def ko(g, j):
    return 4 * g + j if j < 4 else 16 + 4 * g + (j - 4)


def lane_dwords(ad):
    """regs[x, g, w, e]: half e of dword w (0..7: chunk w // 4, register w % 4) of the lane of column x in lane group g:
    the two ds_read_b128 of a lane, row group 4c + g of each chunk"""
    regs = np.zeros((T, 4, 8, 2), np.float16)
    for g in range(4):
        for w in range(8):
            for e in range(2):
                regs[:, g, w, e] = ad[staged_row(4 * (w // 4) + g, 2 * (w % 4) + e), :]
    return regs


def view(regs, ob):
    """a[k, x], k = 8g + j: K slot (g, j) of the view at dword offset 2 ob"""
    a = np.zeros((32, T), np.float16)
    for g in range(4):
        for j in range(8):
            a[8 * g + j] = regs[:, g, 2 * ob + j // 2, j % 2]
    return a


def band(r, up=0):
    """b[k, n]: K slot k = 8g + j against output row n of the block; `up` = 16 for the fourth row block"""
    k = np.array([ko(g, j) for g in range(4) for j in range(8)])
    n = np.arange(16)
    dv = k[:, None] - up - n[None, :]
    return ((dv >= 0) & (dv <= 2 * r)).astype(np.float16)


def stage1_views(ad, r, order, tree):
    """D1 of the four row blocks: f32 accumulation from -bias over the 32 K slots in `order`, then f16 (exact)."""
    regs = lane_dwords(ad)
    out = np.zeros((T, T), np.float16)
    for ob, (v, up) in enumerate(((0, 0), (1, 0), (2, 0), (2, 16))):
        a, b = view(regs, v), band(r, up)
        acc = np.full((16, T), -float(M._bias(r)), np.float32)
        prods = [b[kk, :, None].astype(np.float32) * a[kk][None, :].astype(np.float32) for kk in order]
        if tree:
            s = np.zeros((16, T), np.float32)
            for p in prods:
                s = (s + p).astype(np.float32)
            acc = (acc + s).astype(np.float32)
        else:
            for p in prods:
                acc = (acc + p).astype(np.float32)
        h = acc.astype(np.float16)
        assert np.array_equal(h.astype(np.float32), acc), "D1 not exact in f16"
        assert np.abs(acc).max() < 2048
        out[16 * ob:16 * ob + 16] = h
    return out


def test_row_map_is_a_permutation():
    rows = [staged_row(q, i) for q in range(8) for i in range(8)]
    assert sorted(rows) == list(range(T))
    # a group's rows relative to its first do not depend on the group (the early loads of a carried tile use that)
    for q in range(8):
        assert [staged_row(q, i) - staged_row(q, 0) for i in range(8)] == [0, 1, 2, 3, 16, 17, 18, 19]


def test_views_are_offsets_into_a_lanes_eight_dwords():
    """With AD[row, x] = row, K slot (g, j) of view ob reads input row 16 ob + ko(g, j); the views overlap by two
    dwords; ko is the K order of stage 2 (test_box_mfma_model._stage2's kpos)."""
    ad = np.repeat(np.arange(T, dtype=np.float16)[:, None], T, axis=1)
    regs = lane_dwords(ad)
    for ob in range(3):
        a = view(regs, ob)
        for g in range(4):
            for j in range(8):
                assert (a[8 * g + j] == 16 * ob + ko(g, j)).all(), (ob, g, j)
    assert np.array_equal(view(regs, 0)[[8 * g + j for g in range(4) for j in range(4, 8)]],
                          view(regs, 1)[[8 * g + j for g in range(4) for j in range(4)]])
    kpos = [4 * g + j if j < 4 else 16 + 4 * g + (j - 4) for g in range(4) for j in range(8)]
    assert [ko(g, j) for g in range(4) for j in range(8)] == kpos and sorted(kpos) == list(range(32))


@pytest.mark.parametrize("r", range(1, 8))
def test_one_band_covers_each_window_once(r):
    """Column n of the band holds 2r + 1 ones, at the K slots of the input rows n .. n + 2r (at most row 29 < 32); the
    fourth block's band those of the rows 16 + n .. 16 + n + 2r that the third view holds (up to its row 31)."""
    k = np.array([ko(g, j) for g in range(4) for j in range(8)])
    b, b4 = band(r), band(r, 16)
    for n in range(16):
        assert sorted(k[b[:, n] == 1]) == list(range(n, n + 2 * r + 1))
        assert sorted(k[b4[:, n] == 1]) == list(range(16 + n, min(16 + n + 2 * r, 31) + 1))
    assert 15 + 2 * r < 32


@pytest.mark.parametrize("kind", ["hi_lo", "lo_hi", "random"])
@pytest.mark.parametrize("r", range(1, 8))
def test_views_equal_aligned_chunks_and_integer_sums(r, kind):
    rng = np.random.default_rng(300 * r + len(kind))
    n = T - 2 * r
    L, R = M._frames(kind, n, rng)
    for d in M.DS:
        ad = M._ad_tile(L, R, r, d)
        # integer vertical sums of the tile's AD: output row y sums the input rows y .. y + 2r
        adi = ad.astype(np.int64)
        cs = np.concatenate([np.zeros((1, T), np.int64), adi.cumsum(0)])
        want = cs[2 * r + 1:] - cs[:T - 2 * r] - M._bias(r)          # rows 0 .. 63 - 2r
        for i, order in enumerate(M._orders(32, rng)):
            tree = i == 2
            d1 = stage1_views(ad, r, order, tree)
            assert np.abs(d1.astype(np.float32)).max() < 2048
            assert np.array_equal(d1, M._stage1(ad, r, order, tree)), (r, kind, d, i)
            assert np.array_equal(d1[:n].astype(np.int64), want), (r, kind, d, i)
            # the paired loop's three blocks alone: rows 0..47
            assert np.array_equal(d1[:48].astype(np.int64), want[:48])


def test_worst_case_reaches_the_f16_bound():
    r, n = 7, T - 14
    L, R = M._frames("hi_lo", n, None)
    d1 = stage1_views(M._ad_tile(L, R, r, 0), r, np.arange(32), False)
    assert d1.max() == 15 * 255 - M._bias(7) == 1912 and d1.min() == -M._bias(7) == -1913
