"""numpy restatement of the sub-pixel contract (include/sm_hip.h): 1/16-px disparities from a d-major cost volume,
the uniqueness filter, the threshold and the LR check.  All integer.

A view of a pixel has costs V(d) over the d that exist, a prefix d = 0 .. dmax:
    left view    dmax = min(D - 1, W - x)                               (``sgm_ref.exists``)
    right view   V_R(u, d) = V(u + d, d) over u + 2 d <= W  (right_pairs 1: volumes that hold a cost only where
                 x + d <= W, i.e. SGM's sums and the census cost) or over u + d < W (right_pairs 2: the AD box path)
    d0    = first d at min V
    delta = floor((16 (a - c) + den) / (2 den)), a = V(d0 - 1), b = V(d0), c = V(d0 + 1), den = a + c - 2 b, where
            1 <= d0 < dmax, else 0
    q     = 16 d0 + delta
    uniqueness u in 1..99: invalid if some existing d with |d - d0| > 1 has V(d) (100 - u) < 100 b
    threshold (left view only): invalid if b >= invalid_from (0 = none)
    LR check on the views' d0, an invalid pixel of either view counting as d0 = 0: occluded when x - d < 0, d == 0 or
    |d - d0_R(x - d)| > 1
An invalid or occluded pixel has q = 0 and mask = 0.
"""
import numpy as np

import sgm_ref

SENTINEL = sgm_ref.SENTINEL


def left_exists(D: int, H: int, W: int) -> np.ndarray:
    return np.broadcast_to(sgm_ref.exists(D, W)[:, None, :], (D, H, W))


def right_view(V: np.ndarray, right_pairs: int = 1):
    """(V_R int64 [D, H, W], its existence mask): V_R(u, d) = V(u + d, d)."""
    V = np.asarray(V, np.int64)
    D, H, W = V.shape
    VR = np.full((D, H, W), SENTINEL, np.int64)
    for d in range(min(D, W)):
        VR[d, :, :W - d] = V[d, :, d:]
    u, d = np.arange(W)[None, :], np.arange(D)[:, None]
    E = (u + 2 * d <= W) if right_pairs == 1 else (u + d < W)
    return VR, np.broadcast_to(E[:, None, :], (D, H, W))


def view(V: np.ndarray, E: np.ndarray, u: int = 0, invalid_from: int = 0):
    """One view: (q uint16, d0 uint8, valid bool), each [H, W]; q and d0 are 0 where the pixel is invalid."""
    V = np.asarray(V, np.int64)
    D = V.shape[0]
    Vs = np.where(E, V, SENTINEL)
    d0 = np.argmin(Vs, axis=0)
    dmax = E.sum(axis=0) - 1
    pick = lambda d: np.take_along_axis(Vs, np.clip(d, 0, D - 1)[None], axis=0)[0]   # noqa: E731
    a, b, c = pick(d0 - 1), pick(d0), pick(d0 + 1)
    inner = (d0 >= 1) & (d0 < dmax)
    den = np.where(inner, a + c - 2 * b, 1)
    assert (den >= 1).all()
    delta = np.where(inner, (16 * (a - c) + den) // (2 * den), 0)   # // is the floor division
    q = 16 * d0 + delta
    valid = np.ones(d0.shape, bool)
    if invalid_from:
        valid &= b < invalid_from
    if u:
        far = np.abs(np.arange(D)[:, None, None] - d0[None]) > 1
        valid &= ~(E & far & (V * (100 - u) < b[None] * 100)).any(axis=0)
    return np.where(valid, q, 0).astype(np.uint16), np.where(valid, d0, 0).astype(np.uint8), valid


def view_literal(V: np.ndarray, E: np.ndarray, u: int = 0, invalid_from: int = 0):
    """The same, as the per-pixel loop of the definition (small sizes only)."""
    D, H, W = V.shape
    q = np.zeros((H, W), np.uint16)
    d0s = np.zeros((H, W), np.uint8)
    valid = np.zeros((H, W), bool)
    for y in range(H):
        for x in range(W):
            ds = [d for d in range(D) if E[d, y, x]]
            dmax = ds[-1]
            assert ds == list(range(dmax + 1))
            v = [int(V[d, y, x]) for d in ds]
            b = min(v)
            d0 = v.index(b)
            delta = 0
            if 1 <= d0 < dmax:
                a, c = v[d0 - 1], v[d0 + 1]
                den = a + c - 2 * b
                delta = (16 * (a - c) + den) // (2 * den)   # Python's // floors
            ok = not (invalid_from and b >= invalid_from)
            if u and any(abs(d - d0) > 1 and v[d] * (100 - u) < b * 100 for d in ds):
                ok = False
            if ok:
                q[y, x], d0s[y, x], valid[y, x] = 16 * d0 + delta, d0, True
    return q, d0s, valid


def lr_occluded(dl: np.ndarray, dr: np.ndarray) -> np.ndarray:
    """bool [H, W]: x - d < 0, d == 0 or |d - dR(x - d)| > 1 (launch_lr_check on the two d0 maps)."""
    H, W = dl.shape
    d = dl.astype(np.int64)
    x = np.arange(W)[None, :]
    src = np.clip(x - d, 0, W - 1)
    diff = d - np.take_along_axis(dr.astype(np.int64), src, axis=1)
    return (x - d < 0) | (d == 0) | (np.abs(diff) > 1)


def subpix(V: np.ndarray, u: int = 0, invalid_from: int = 0, lr: bool = False, right_pairs: int = 1,
           view_fn=view):
    """(q uint16, right-view q uint16, mask uint8) of a cost volume V [D, H, W] (values at entries that do not
    exist are ignored)."""
    V = np.asarray(V, np.int64)
    D, H, W = V.shape
    q, dl, valid = view_fn(V, left_exists(D, H, W), u, invalid_from)
    qr, dr, _ = view_fn(*right_view(V, right_pairs), u, 0)
    if lr:
        occ = lr_occluded(dl, dr)
        q = np.where(occ, 0, q).astype(np.uint16)
        valid = ~occ
    return q, qr, valid.astype(np.uint8)


def volume(oracle, left, right, radius: int, D: int, agg: str, cost: str, P1: int = 0, P2: int = 0):
    """(V, invalid_from, right_pairs) of one of the four paths of the matching calls."""
    import census_ref
    if cost == "census":
        C = census_ref.cost(left, right, radius, D).astype(np.int64)
        a1, a2 = census_ref.auto_penalties(radius)
    else:
        C = oracle.box_cost(left, right, radius, D).astype(np.int64)
        a1, a2 = sgm_ref.auto_penalties(radius)
    if agg == "sgm":
        return sgm_ref.aggregate(C, P1 or a1, P2 or a2)[0], 0, 1
    if cost == "census":
        return C, 0, 1
    return C, 50 * (2 * radius + 1) ** 2, 2


def mae(disp: np.ndarray, d_int: np.ndarray, gt: np.ndarray) -> float:
    """Mean |disp - gt| over the pixels with gt > 0 whose integer disparity d_int is within 1 of gt."""
    sel = (gt > 0) & (np.abs(d_int.astype(np.float64) - gt) <= 1)
    return float(np.abs(disp.astype(np.float64) - gt)[sel].mean())
