"""numpy restatement of the 16-bit median (sm_median_u16_device) and of the sub-pixel calls' steps under
SM_PARAM_SUBPIX_MEDIAN (include/sm_hip.h).  All integer.

    median(a, r)(y, x) = the element of rank 2 r^2 + 2 r (0-based) of the (2r+1)^2 values a(clamp(y + i), clamp(x + j)),
                         |i|, |j| <= r: replicate borders, the whole 16-bit value, 0 a value like any other
    subpix_median      = median of both views' 1/16-px maps, then the LR check on d = (q' + 8) >> 4 of the two filtered
                         maps (occluded when x - d < 0, d == 0 or |d - d_R(x - d)| > 1), occluded q' = 0,
                         mask = final q' != 0
"""
import numpy as np

import subpix_ref


def median(a: np.ndarray, r: int) -> np.ndarray:
    """The (2r+1)^2 median of a 2-D integer map with replicate borders, in the map's dtype."""
    a = np.asarray(a)
    if a.ndim != 2 or r < 0:
        raise ValueError("median: a 2-D map and r >= 0")
    H, W = a.shape
    p = np.pad(a, r, mode="edge")
    k = 2 * r + 1
    win = np.stack([p[i:i + H, j:j + W] for i in range(k) for j in range(k)])   # [k*k, H, W]
    t = 2 * r * r + 2 * r
    return np.partition(win, t, axis=0)[t].astype(a.dtype)


def median_literal(a: np.ndarray, r: int) -> np.ndarray:
    """The same as the per-pixel loop of the definition (small sizes only)."""
    H, W = a.shape
    out = np.zeros_like(a)
    for y in range(H):
        for x in range(W):
            vals = sorted(int(a[min(max(y + i, 0), H - 1), min(max(x + j, 0), W - 1)])
                          for i in range(-r, r + 1) for j in range(-r, r + 1))
            out[y, x] = vals[2 * r * r + 2 * r]
    return out


def rounded(q: np.ndarray) -> np.ndarray:
    """Whole disparities of a 1/16-px map, round half up: (q + 8) >> 4 in 32 bits (65528 -> 4096)."""
    return ((q.astype(np.int64) + 8) >> 4).astype(np.int32)


def subpix_median(q: np.ndarray, qr: np.ndarray, r: int, lr: bool):
    """(q', right q', mask uint8) from the two views' unchecked 1/16-px maps (0 where a view is invalid)."""
    q = np.asarray(q, np.uint16)
    qr = np.asarray(qr, np.uint16)
    qm, qrm = median(q, r), median(qr, r)
    if lr:
        occ = subpix_ref.lr_occluded(rounded(qm), rounded(qrm))
        qm = np.where(occ, 0, qm).astype(np.uint16)
    return qm, qrm, (qm != 0).astype(np.uint8)
