"""numpy restatement of the SM_COST_CENSUS contract (include/sm_hip.h): the 9 x 7 census transform, its
Hamming cost volume and the two aggregations that take it (box and SGM).

census(y, x) is a uint64: the neighbours dx in [-4, 4], dy in [-3, 3] are visited row-major (dy outer, dx inner),
the centre is skipped, which leaves 62 of them on bits 0..61 in that order; a bit is 1 iff the neighbour, read
with the border replicated, is darker than the centre.  ham[d][y][x] = popcount(censusL(y, x) ^ censusR(y, x - d))
for x >= d, else 0 (the zero rule of the AD volume), and the cost C is its zero-padded (2r+1)^2 window sum.
Box: the thresholdless first minimum of C over the pairs that exist (x + d <= W); SGM: ``sgm_ref.aggregate`` on C.
The right view and the check are ``oracle.right_wta`` and ``oracle.lr_check``, as for SM_AGG_SGM.
"""
import numpy as np

import sgm_ref

WIN_DX, WIN_DY = 4, 3
OFFSETS = tuple((dy, dx) for dy in range(-WIN_DY, WIN_DY + 1) for dx in range(-WIN_DX, WIN_DX + 1)
                if (dy, dx) != (0, 0))   # bit k compares neighbour OFFSETS[k]
MAX_HAM = len(OFFSETS)                   # 62


def census(img: np.ndarray) -> np.ndarray:
    """uint64 [H, W] census words of a uint8 image."""
    img = np.asarray(img, np.uint8)
    H, W = img.shape
    pad = np.pad(img, ((WIN_DY, WIN_DY), (WIN_DX, WIN_DX)), mode="edge")
    out = np.zeros((H, W), np.uint64)
    for k, (dy, dx) in enumerate(OFFSETS):
        nb = pad[WIN_DY + dy:WIN_DY + dy + H, WIN_DX + dx:WIN_DX + dx + W]
        out |= (nb < img).astype(np.uint64) << np.uint64(k)
    return out


def census_literal(img: np.ndarray) -> np.ndarray:
    """The same, as the per-pixel, per-bit loop of the definition (small sizes only)."""
    H, W = img.shape
    out = np.zeros((H, W), np.uint64)
    for y in range(H):
        for x in range(W):
            word, k = 0, 0
            for dy in range(-3, 4):
                for dx in range(-4, 5):
                    if dy == 0 and dx == 0:
                        continue
                    yy, xx = min(max(y + dy, 0), H - 1), min(max(x + dx, 0), W - 1)
                    if int(img[yy, xx]) < int(img[y, x]):
                        word |= 1 << k
                    k += 1
            out[y, x] = word
    return out


def _popcount(a: np.ndarray) -> np.ndarray:
    return np.unpackbits(np.ascontiguousarray(a).view(np.uint8).reshape(a.shape + (8,)), axis=-1).sum(axis=-1)


def hamming_volume(left: np.ndarray, right: np.ndarray, D: int) -> np.ndarray:
    """uint8 [D, H, W]: popcount(censusL(y, x) ^ censusR(y, x - d)) for x >= d, 0 otherwise."""
    cl, cr = census(left), census(right)
    H, W = cl.shape
    ham = np.zeros((D, H, W), np.uint8)
    for d in range(min(D, W)):
        ham[d, :, d:] = _popcount(cl[:, d:] ^ cr[:, :W - d])
    return ham


def hamming_volume_literal(left: np.ndarray, right: np.ndarray, D: int) -> np.ndarray:
    cl, cr = census_literal(left), census_literal(right)
    H, W = cl.shape
    ham = np.zeros((D, H, W), np.uint8)
    for d in range(D):
        for y in range(H):
            for x in range(d, W):
                ham[d, y, x] = bin(int(cl[y, x]) ^ int(cr[y, x - d])).count("1")
    return ham


def box_sum(vol: np.ndarray, r: int) -> np.ndarray:
    """int32 [D, H, W]: the zero-padded (2r+1)^2 window sum of every plane of `vol`."""
    v = np.asarray(vol, np.int64)
    D, H, W = v.shape
    I = np.zeros((D, H + 1, W + 1), np.int64)
    I[:, 1:, 1:] = v.cumsum(1).cumsum(2)
    y0, y1 = np.clip(np.arange(H) - r, 0, H), np.clip(np.arange(H) + r + 1, 0, H)
    x0, x1 = np.clip(np.arange(W) - r, 0, W), np.clip(np.arange(W) + r + 1, 0, W)
    s = I[:, y1][:, :, x1] - I[:, y0][:, :, x1] - I[:, y1][:, :, x0] + I[:, y0][:, :, x0]
    return s.astype(np.int32)


def cost(left: np.ndarray, right: np.ndarray, r: int, D: int) -> np.ndarray:
    """The census cost C, int32 [D, H, W] (<= 62 (2r+1)^2)."""
    return box_sum(hamming_volume(left, right, D), r)


def auto_penalties(radius: int):
    win2 = (2 * radius + 1) ** 2
    return 10 * win2, 120 * win2


def box_wta(C: np.ndarray):
    """(C with SENTINEL where the pair does not exist, the thresholdless left map: smallest existing d at min C)."""
    D, H, W = C.shape
    E = np.broadcast_to(sgm_ref.exists(D, W)[:, None, :], C.shape)
    S = np.where(E, np.asarray(C, np.int64), sgm_ref.SENTINEL)
    return S, np.argmin(S, axis=0).astype(np.uint8)


def census_lr(oracle, left, right, r: int, D: int, agg: str = "sgm", P1: int = 0, P2: int = 0, median: bool = False):
    """Full pipeline on a gray pair: (left map, right map, checked map, mask) of agg 'box' or 'sgm' on the census
    cost; P1 / P2 0 = auto; median: both maps through the 7x7 median before the check (as SM_MEDIAN)."""
    C = cost(left, right, r, D)
    if agg == "box":
        S, dl = box_wta(C)
    elif agg == "sgm":
        a1, a2 = auto_penalties(r)
        S, dl = sgm_ref.aggregate(C, P1 or a1, P2 or a2)
    else:
        raise ValueError("agg must be 'box' or 'sgm'")
    dr = oracle.right_wta(S.astype(np.int32))
    if median:
        dl, dr = oracle.median(dl, 3), oracle.median(dr, 3)
    checked, mask = oracle.lr_check(dl, dr)
    return dl, dr, checked, mask
