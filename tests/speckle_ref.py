"""The speckle filter's contract (include/sm_hip.h, "speckle filter") restated in numpy: OpenCV's
filterSpeckles(img, newVal = 0, maxSpeckleSize, maxDiff) on a uint8 or uint16 map in which 0 is invalid.

  * a pixel is valid iff its value is != 0; invalid pixels belong to no region and are never changed;
  * two 4-neighbours are joined iff both are valid and |a - b| <= max_diff (taken in int64: nothing wraps);
  * regions are the connected components; a region of at most max_size pixels is set to 0, and the mask is set to
    0 at exactly those pixels.

`components` is min-label propagation with pointer jumping to a fixed point, vectorised; `speckle_literal` is the
stack flood fill, pixel by pixel, for small maps.  numpy only.
"""
import numpy as np

NO_LABEL = -1


def joins(img: np.ndarray, max_diff: int):
    """(right, down): right[y, x] is True where (y, x) and (y, x + 1) are joined, down[y, x] where (y, x) and
    (y + 1, x) are; both of img's shape (the last column / row is False)."""
    v = img.astype(np.int64)
    ok = v != 0
    right = np.zeros(v.shape, bool)
    down = np.zeros(v.shape, bool)
    right[:, :-1] = ok[:, :-1] & ok[:, 1:] & (np.abs(v[:, :-1] - v[:, 1:]) <= max_diff)
    down[:-1, :] = ok[:-1, :] & ok[1:, :] & (np.abs(v[:-1, :] - v[1:, :]) <= max_diff)
    return right, down


def components(img: np.ndarray, max_diff: int) -> np.ndarray:
    """int64 labels of img's shape: the smallest row-major index of the pixel's region, NO_LABEL where img == 0."""
    H, W = img.shape
    P = H * W
    right, down = joins(img, max_diff)
    lab = np.arange(P, dtype=np.int64).reshape(H, W)
    big = np.int64(P)
    while True:
        m = lab.copy()
        # the smallest label among a pixel and its joined neighbours
        np.minimum(m[:, :-1], np.where(right[:, :-1], lab[:, 1:], big), out=m[:, :-1])
        np.minimum(m[:, 1:], np.where(right[:, :-1], lab[:, :-1], big), out=m[:, 1:])
        np.minimum(m[:-1, :], np.where(down[:-1, :], lab[1:, :], big), out=m[:-1, :])
        np.minimum(m[1:, :], np.where(down[:-1, :], lab[:-1, :], big), out=m[1:, :])
        flat = m.reshape(-1)
        while True:   # pointer jumping: a label is a pixel of the same region, whose label is no larger
            nxt = flat[flat]
            if np.array_equal(nxt, flat):
                break
            flat = nxt
        m = flat.reshape(H, W)
        if np.array_equal(m, lab):
            break
        lab = m
    return np.where(img != 0, lab, NO_LABEL)


def speckle(img: np.ndarray, max_size: int, max_diff: int, mask=None):
    """(filtered copy of img, filtered copy of mask or None)."""
    out = img.copy()
    mk = None if mask is None else mask.copy()
    if max_size <= 0:
        return out, mk
    lab = components(img, max_diff)
    valid = lab != NO_LABEL
    sizes = np.bincount(lab[valid], minlength=img.size)
    remove = valid & (sizes[np.where(valid, lab, 0)] <= max_size)
    out[remove] = 0
    if mk is not None:
        mk[remove] = 0
    return out, mk


def speckle_literal(img: np.ndarray, max_size: int, max_diff: int, mask=None):
    """The same by a stack flood fill from every unvisited valid pixel, comparing each popped pixel with its four
    neighbours (filterSpeckles' loop), in Python integers."""
    H, W = img.shape
    out = img.copy()
    mk = None if mask is None else mask.copy()
    seen = np.zeros((H, W), bool)
    for y0 in range(H):
        for x0 in range(W):
            if seen[y0, x0] or img[y0, x0] == 0:
                continue
            seen[y0, x0] = True
            stack, region = [(y0, x0)], []
            while stack:
                y, x = stack.pop()
                region.append((y, x))
                v = int(img[y, x])
                for yy, xx in ((y, x + 1), (y, x - 1), (y + 1, x), (y - 1, x)):
                    if 0 <= yy < H and 0 <= xx < W and not seen[yy, xx] and img[yy, xx] != 0 \
                            and abs(v - int(img[yy, xx])) <= max_diff:
                        seen[yy, xx] = True
                        stack.append((yy, xx))
            if len(region) <= max_size:
                for y, x in region:
                    out[y, x] = 0
                    if mk is not None:
                        mk[y, x] = 0
    return out, mk
