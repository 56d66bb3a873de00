"""A numpy model of what the matrix-pipe box kernel's unmasked paired loop carries from pass to pass
(bm_box_mfma.hip run_paired), against slot() and the key constant restated here:
  - the R addresses: a carried byte offset of p = 0's column that loses two columns per pass, the swizzle term taken
    from bits 8..10 of that offset, p = 1 one column to the left or, in an odd last pass, p = 0's column;
  - the key constants: f32 splats that step by 2.0, the odd last pass labelling its repeated disparity d + 1.
No GPU: the kernel's own results are compared with the oracle in test_gpu_box_mfma_trim.py."""
import numpy as np
import pytest

COL_B = 128          # kColB: bytes per staged column
L_BYTES = 64 * COL_B
D_MAXES = (64, 128, 192, 256)


def slot(col, q):
    """bm_box_mfma.hip slot(): byte offset of 16-B row group q of staged column col."""
    return col * COL_B + ((q ^ ((col >> 1) & 7)) << 4)


def swz(colb, g16):
    """run_paired's swz(): the address of a column's row group from the column's byte address."""
    return colb + (((colb >> 4) & 0x70) ^ g16)


def stepped_addresses(col0, lo, hi, g, base):
    """[(raddr0, raddr1)] of the passes d = lo, lo + 2, .. < hi as the loop computes them."""
    g16 = g << 4
    rcol = base + col0 * COL_B
    out = []
    d = lo
    ra = (swz(rcol, g16), swz(rcol - (COL_B if d + 1 < hi else 0), g16))
    while d < hi:
        out.append(ra)
        rcol -= 2 * COL_B          # step_addr(), in the last output block of the pass
        ra = (swz(rcol, g16), swz(rcol - (COL_B if d + 3 < hi else 0), g16))
        d += 2
    return out


@pytest.mark.parametrize("lds0", (0, 2048, 6144))
def test_stepped_swizzle_200_passes(lds0):
    """200 passes from every swizzle phase and column parity, every lane: the stepped address is slot() of the
    recomputed column, behind the left tile, for any smem address that is a multiple of the swizzle period."""
    base = lds0 + L_BYTES
    for c0 in range(400, 432):
        for g in range(4):
            for odd in (0, 1):
                lo, hi = 0, 400 - odd
                got = stepped_addresses(c0, lo, hi, g, base)
                assert len(got) == 200
                for k, (a0, a1) in enumerate(got):
                    d = lo + 2 * k
                    d1 = min(d + 1, hi - 1)
                    assert a0 == base + slot(c0 - (d - lo), g), (c0, g, k)
                    assert a1 == base + slot(c0 - (d1 - lo), g), (c0, g, k)
                    for a in (a0, a1):   # chunk 1 is ^ 64 on the address as on the offset
                        assert (a ^ 64) - base == (a - base) ^ 64


@pytest.mark.parametrize("d_max", D_MAXES)
def test_wave_ranges_of_every_d_max(d_max):
    """The kernel's own columns l16 + DMAX + d_lo - dd[p]: every wave range [lo, hi) of a tile whose d range is a
    slice from d_lo, all lanes, and the last address stays inside the band (no column below 0 is formed for a read)."""
    rc = 64 + d_max
    for d_lo, nd in ((0, d_max), (37, min(40, d_max)), (21, 9), (5, 1), (3, d_max - 3)):
        for w in range(4):
            lo, hi = d_lo + (w * nd) // 4, d_lo + ((w + 1) * nd) // 4
            for l16 in range(16):
                for g in range(4):
                    col0 = l16 + d_max + d_lo - lo
                    got = stepped_addresses(col0, lo, hi, g, L_BYTES)
                    for k, (a0, a1) in enumerate(got):
                        d = lo + 2 * k
                        dd = (d, min(d + 1, hi - 1))
                        for p, a in enumerate((a0, a1)):
                            col = l16 + d_max + d_lo - dd[p]
                            assert 0 <= col and col + 48 < rc     # + 16 cb columns per block, cb <= 3
                            assert a == L_BYTES + slot(col, g)


@pytest.mark.parametrize("r", range(1, 8))
def test_stepped_key_constants(r):
    """c2[p] starts at c2base + lo + p and steps by 2.0 in f32: exact integers below 2^24, equal to c2base + dd[p]
    in every pass but an odd last one, whose p = 1 is labelled d + 1: a key with p = 0's cost and a larger low byte,
    which loses the min against p = 0's."""
    bias = ((2 * r + 1) * 255 + 1) // 2
    c2base = np.float32(256 * (2 * r + 1) * bias)
    worst = (2 * r + 1) ** 2 * 255 * 256 + 255
    assert worst < 1 << 24
    for lo, hi in ((0, 64), (37, 102), (191, 256), (255, 256), (7, 8), (100, 109)):
        c2 = [np.float32(c2base + np.float32(lo + p)) for p in range(2)]
        for d in range(lo, hi, 2):
            dd = (d, min(d + 1, hi - 1))
            assert c2[0] == np.float32(int(c2base) + dd[0]) and float(c2[0]) == int(c2base) + dd[0]
            if d + 1 < hi:
                assert float(c2[1]) == int(c2base) + dd[1]
            else:
                assert float(c2[1]) == int(c2base) + d + 1 and d + 1 <= 256
                # the same window sum S added to both constants: keys (S << 8 | d) and (S << 8 | d + 1) as f32 bits
                for s in (-256 * (2 * r + 1) * bias, 0, 256 * ((2 * r + 1) ** 2 * 255 - (2 * r + 1) * bias)):
                    k0 = np.float32(float(c2[0]) + s).view(np.uint32)
                    k1 = np.float32(float(c2[1]) + s).view(np.uint32)
                    assert min(int(k0), int(k1)) == int(k0) and int(k1) != int(k0)
            c2 = [np.float32(c + np.float32(2.0)) for c in c2]
