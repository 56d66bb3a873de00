"""The row fill's contract (include/sm_hip.h, "row fill") restated in numpy, on a uint8 or uint16 map in which 0 is
invalid.

  * a pixel is valid iff its value is != 0; valid pixels are never changed;
  * a run is a maximal stretch of invalid pixels in one row, columns a .. b; its left neighbour is the pixel at
    a - 1 if a > 0, its right neighbour the pixel at b + 1 if b < W - 1; rows never interact;
  * a run of more than max_gap pixels stays; otherwise every pixel of it becomes min(left, right), or the one
    neighbour it has when it touches a border; a row with no valid pixel stays 0;
  * the minimum is taken on the whole element.

`fill` is vectorised: the column of the nearest valid pixel on either side by a running maximum / minimum along the
row.  `fill_literal` is the definition, one row and one run at a time in Python integers, for small maps.  numpy only.
"""
import numpy as np


def fill(img: np.ndarray, max_gap: int) -> np.ndarray:
    """The filled copy of img."""
    out = img.copy()
    if max_gap <= 0 or img.size == 0:
        return out
    H, W = img.shape
    valid = img != 0
    cols = np.broadcast_to(np.arange(W, dtype=np.int64), (H, W))
    # column of the nearest valid pixel at or left of x (-1: none), at or right of x (W: none)
    left = np.maximum.accumulate(np.where(valid, cols, -1), axis=1)
    right = np.minimum.accumulate(np.where(valid, cols, W)[:, ::-1], axis=1)[:, ::-1]
    has_l, has_r = left >= 0, right < W
    lv = np.take_along_axis(img, np.clip(left, 0, W - 1), axis=1)
    rv = np.take_along_axis(img, np.clip(right, 0, W - 1), axis=1)
    length = right - left - 1                      # of the run an invalid pixel lies in
    value = np.where(has_l & has_r, np.minimum(lv, rv), np.where(has_l, lv, rv))
    take = ~valid & (has_l | has_r) & (length <= max_gap)
    out[take] = value[take]
    return out


def fill_literal(img: np.ndarray, max_gap: int) -> np.ndarray:
    """The same, run by run."""
    H, W = img.shape
    out = img.copy()
    for y in range(H):
        x = 0
        while x < W:
            if img[y, x] != 0:
                x += 1
                continue
            a = x
            while x < W and img[y, x] == 0:
                x += 1
            b = x - 1
            if b - a + 1 > max_gap:
                continue
            left = int(img[y, a - 1]) if a > 0 else None
            right = int(img[y, b + 1]) if b < W - 1 else None
            if left is None and right is None:
                continue
            v = min(left, right) if left is not None and right is not None else (left if right is None else right)
            out[y, a:b + 1] = v
    return out


def filled(before: np.ndarray, after: np.ndarray) -> np.ndarray:
    """Where the fill wrote: invalid before, valid after."""
    return (before == 0) & (after != 0)
