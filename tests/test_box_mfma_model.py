"""CPU model of bm_box_mfma.hip's arithmetic: the box-window sums as two products with banded matrices in
float16 / float32, with the kernel's staging (1024 + v in f16), biases (ceil((2r+1) * 255 / 2) in stage 1,
256 * (2r+1) * bias + d in stage 2), band constants (1.0 and 256.0), 32-row / 32-column K chunks and stage-2 K order
((4g + j, 16 + 4g + j) over the lane groups g).  Every intermediate must be an integer its format holds exactly,
so the f32 accumulator is the key (S << 8 | d) whatever the summation order: checked against integer box sums
for r = 1..7 on L = 255 / R = 0, the reverse, and random frames, with the K sums taken in several orders."""
import numpy as np
import pytest

T = 64            # input tile edge
DS = (0, 3, 7)    # disparities of the model tile


def _bias(r):
    return ((2 * r + 1) * 255 + 1) // 2


def _orders(n, rng):
    return [np.arange(n), np.arange(n)[::-1], rng.permutation(n)]


def _ad_tile(L, R, r, d):
    """The AD operand of one tile covering the whole TO x TO image: 64 x 64 f16, image origin at (r, r)."""
    H, W = L.shape
    Lh = np.full((T, T), 0x6400, np.uint16)
    Rh = np.full((T, T), 0x6400, np.uint16)           # R(c - d) per tile column c
    Lh[r:r + H, r:r + W] |= L
    Rs = np.zeros((H, W), np.uint8)
    Rs[:, d:] = R[:, :W - d]
    Rh[r:r + H, r:r + W] |= Rs
    diff = Lh.view(np.float16) - Rh.view(np.float16)   # exact: unit spacing on [1024, 2048)
    assert diff.dtype == np.float16
    ad = (diff.view(np.uint16) & 0x7FFF).view(np.float16)
    cols = np.arange(T) - r                            # image column of tile column
    ad[:, (cols < d) | (cols >= W)] = 0                # the masked tiles' select
    ad[(np.arange(T) < r) | (np.arange(T) >= r + H), :] = 0   # rows outside: both sides staged 0
    return ad


def _stage1(ad, r, order, tree):
    """D1[yout, x] = sum over the window's input rows of AD - bias, per 16-row output block from the 32-row
    chunks the kernel uses; f32 accumulation in `order` within a chunk, then f16."""
    out = np.zeros((T, T), np.float16)
    k = np.arange(32)
    for ob, chunks in enumerate(([0], [0, 1], [1], [1])):
        acc = np.full((16, T), -float(_bias(r)), np.float32)
        n = 16 * ob + np.arange(16)
        for ch in chunks:
            band = ((32 * ch + k[:, None] - n[None, :] >= 0) &
                    (32 * ch + k[:, None] - n[None, :] <= 2 * r)).astype(np.float16)       # [k, n]
            prods = [band[kk, :, None].astype(np.float32) * ad[32 * ch + kk][None, :].astype(np.float32)
                     for kk in order]
            if tree:                                   # products first, the accumulator last
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


def _stage2(d1, r, d, order, tree):
    """key[yout, xout] = C + sum over 32 input columns of 256 * D1, C = 256 * (2r+1) * bias + d; per 16-column
    output block from column blocks (xb, xb + 1), the block past the tile all zero."""
    d1p = np.concatenate([d1, np.zeros((T, 16), np.float16)], axis=1)
    kpos = np.array([4 * g + j if j < 4 else 16 + 4 * g + (j - 4) for g in range(4) for j in range(8)])
    keys = np.zeros((T, T), np.uint32)
    c = np.float32(256 * (2 * r + 1) * _bias(r) + d)
    m = np.arange(16)
    for xb in range(4):
        acc = np.full((T, 16), c, np.float32)
        prods = []
        for kk in order:
            xin = kpos[kk]
            band = np.where((xin - m >= 0) & (xin - m <= 2 * r), np.float16(256), np.float16(0))
            prods.append(band[None, :].astype(np.float32) * d1p[:, 16 * xb + xin][:, None].astype(np.float32))
        if tree:
            s = np.zeros((T, 16), np.float32)
            for p in prods:
                s = (s + p).astype(np.float32)
                assert np.abs(s).max() < 2 ** 24
            acc = (acc + s).astype(np.float32)
        else:
            for p in prods:
                acc = (acc + p).astype(np.float32)
                assert np.abs(acc).max() < 2 ** 24
        assert (acc >= 0).all()
        bits = acc.view(np.uint32)
        ints = acc.astype(np.uint32)
        # positive f32 bit patterns order like the integers they hold
        assert np.array_equal(np.argsort(bits.ravel(), kind="stable"), np.argsort(ints.ravel(), kind="stable"))
        keys[:, 16 * xb:16 * xb + 16] = ints
    return keys


def _int_keys(L, R, r, d):
    H, W = L.shape
    ad = np.zeros((H + 2 * r, W + 2 * r), np.int64)
    ad[r:r + H, r + d:r + W] = np.abs(L[:, d:].astype(np.int64) - R[:, :W - d].astype(np.int64))
    ii = np.pad(ad.cumsum(0).cumsum(1), ((1, 0), (1, 0)))
    w = 2 * r + 1
    S = ii[w:, w:] - ii[:-w, w:] - ii[w:, :-w] + ii[:-w, :-w]
    return (S << 8) | d


def _frames(kind, n, rng):
    if kind == "hi_lo":
        return np.full((n, n), 255, np.uint8), np.zeros((n, n), np.uint8)
    if kind == "lo_hi":
        return np.zeros((n, n), np.uint8), np.full((n, n), 255, np.uint8)
    return rng.integers(0, 256, (n, n), dtype=np.uint8), rng.integers(0, 256, (n, n), dtype=np.uint8)


@pytest.mark.parametrize("kind", ["hi_lo", "lo_hi", "random"])
@pytest.mark.parametrize("r", range(1, 8))
def test_mfma_model_equals_integer_box_sums(r, kind):
    rng = np.random.default_rng(100 * r + len(kind))
    n = T - 2 * r
    L, R = _frames(kind, n, rng)
    assert _bias(r) < 2048 and (2 * r + 1) * 255 - _bias(r) < 2048
    for d in DS:
        want = _int_keys(L, R, r, d)
        assert want.max() < 2 ** 24
        ad = _ad_tile(L, R, r, d)
        for i, order in enumerate(_orders(32, rng)):
            tree = i == 2
            keys = _stage2(_stage1(ad, r, order, tree), r, d, order, tree)
            assert np.array_equal(keys[:n, :n].astype(np.int64), want), (r, kind, d, i)


def test_worst_case_reaches_the_bounds():
    """r = 7, L = 255 against R = 0: interior sums are 15 * 15 * 255, the largest key the f32 holds."""
    r, n = 7, T - 14
    L, R = _frames("hi_lo", n, None)
    want = _int_keys(L, R, r, 0)
    assert want.max() == (15 * 15 * 255) << 8
    ad = _ad_tile(L, R, r, 0)
    d1 = _stage1(ad, r, np.arange(32), False)
    assert d1.max() == 15 * 255 - _bias(7) == 1912 and d1.min() == -_bias(7) == -1913
