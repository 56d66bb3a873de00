"""numpy restatement of the SM_AGG_SGM contract (include/sm_hip.h): four-path semi-global matching on the
box SAD volume of ``oracle.box_cost``.

Pairs (x, d) exist iff x + d <= W (Device.cu:44).  For a direction rho and q = p - rho:
    L(p, d) = C(p, d)                                                              q outside the image
    L(p, d) = C(p, d) + min(L(q, d), L(q, d-1) + P1, L(q, d+1) + P1, M + P2) - M   M = min over existing k of L(q, k)
with the terms whose d +- 1 is outside [0, D) or does not exist at q dropped; S is the sum over rho in
{(+1,0), (-1,0), (0,+1), (0,-1)}; the left map is the smallest existing d at min S.  Each scan walks one
axis and vectorises the other two.  The right map and the check are ``oracle.right_wta(S)`` and
``oracle.lr_check``: SENTINEL at the entries that do not exist keeps them from winning there too.
"""
import numpy as np

SENTINEL = 1 << 30   # S at non-existent entries: above every sum (< 2^18), within int32 for oracle.right_wta
_INF = 1 << 40       # a non-existent L inside the scans

DIRECTIONS = ((1, 0), (-1, 0), (0, 1), (0, -1))   # rho = (dx, dy)


def auto_penalties(radius: int):
    win2 = (2 * radius + 1) ** 2
    return 8 * win2, 32 * win2


def exists(D: int, W: int) -> np.ndarray:
    """bool [D, W]: the pair (x, d) exists."""
    return np.arange(D)[:, None] + np.arange(W)[None, :] <= W


def _step(C, prev, E, P1, P2):
    """One step of the recursion for a whole slice: C, prev [D, n] (prev _INF where it does not exist),
    E [D, n] existence at the current pixels."""
    M = prev.min(axis=0)
    below = np.full_like(prev, _INF)
    below[1:] = prev[:-1]
    above = np.full_like(prev, _INF)
    above[:-1] = prev[1:]
    best = np.minimum(np.minimum(prev, below + P1), np.minimum(above + P1, M[None, :] + P2))
    return np.where(E, C + best - M[None, :], _INF)


def path(C: np.ndarray, rho, P1: int, P2: int) -> np.ndarray:
    """L_rho [D, H, W] int64 (_INF where the pair does not exist)."""
    C = np.asarray(C, np.int64)
    D, H, W = C.shape
    E = exists(D, W)
    L = np.full((D, H, W), _INF, np.int64)
    dx, dy = rho
    if dx:
        xs = range(W) if dx > 0 else range(W - 1, -1, -1)
        prev = None
        for x in xs:
            Ex = np.broadcast_to(E[:, x:x + 1], (D, H))
            cur = np.where(Ex, C[:, :, x], _INF) if prev is None else _step(C[:, :, x], prev, Ex, P1, P2)
            L[:, :, x] = cur
            prev = cur
    else:
        ys = range(H) if dy > 0 else range(H - 1, -1, -1)
        prev = None
        for y in ys:
            cur = np.where(E, C[:, y, :], _INF) if prev is None else _step(C[:, y, :], prev, E, P1, P2)
            L[:, y, :] = cur
            prev = cur
    return L


def path_literal(C: np.ndarray, rho, P1: int, P2: int) -> np.ndarray:
    """The same, as the per-pixel triple loop of the definition (small sizes only)."""
    D, H, W = C.shape
    dx, dy = rho
    ex = lambda x, d: 0 <= d < D and x + d <= W   # noqa: E731
    L = np.full((D, H, W), _INF, np.int64)
    ys = range(H) if dy >= 0 else range(H - 1, -1, -1)
    xs = range(W) if dx >= 0 else range(W - 1, -1, -1)
    for y in ys:
        for x in xs:
            qx, qy = x - dx, y - dy
            inside = 0 <= qx < W and 0 <= qy < H
            if inside:
                M = min(int(L[k, qy, qx]) for k in range(D) if ex(qx, k))
            for d in range(D):
                if not ex(x, d):
                    continue
                if not inside:
                    L[d, y, x] = int(C[d, y, x])
                    continue
                terms = [M + P2]
                if ex(qx, d):
                    terms.append(int(L[d, qy, qx]))
                if ex(qx, d - 1):
                    terms.append(int(L[d - 1, qy, qx]) + P1)
                if ex(qx, d + 1):
                    terms.append(int(L[d + 1, qy, qx]) + P1)
                L[d, y, x] = int(C[d, y, x]) + min(terms) - M
    return L


def aggregate(C: np.ndarray, P1: int, P2: int, path_fn=path):
    """(S int64 [D, H, W] with SENTINEL where the pair does not exist, left map uint8 [H, W])."""
    C = np.asarray(C, np.int64)
    D, H, W = C.shape
    E = np.broadcast_to(exists(D, W)[:, None, :], (D, H, W))
    S = np.zeros((D, H, W), np.int64)
    for rho in DIRECTIONS:
        S += np.where(E, path_fn(C, rho, P1, P2), 0)
    S = np.where(E, S, SENTINEL)
    return S, np.argmin(S, axis=0).astype(np.uint8)   # first minimum = smallest d


def sgm_lr(oracle, left, right, radius: int, D: int, P1: int, P2: int, median: bool = False):
    """Full pipeline on a gray pair: (left map, right map, checked map, mask); median: both maps through
    the 7x7 median before the check (as SM_MEDIAN)."""
    S, dl = aggregate(oracle.box_cost(left, right, radius, D), P1, P2)
    dr = oracle.right_wta(S.astype(np.int32))
    if median:
        dl, dr = oracle.median(dl, 3), oracle.median(dr, 3)
    checked, mask = oracle.lr_check(dl, dr)
    return dl, dr, checked, mask


def bad_rate(disp: np.ndarray, gt: np.ndarray) -> float:
    """Share of the pixels with ground truth (gt > 0) whose disparity is off by more than 1."""
    v = gt > 0
    return float((np.abs(disp.astype(np.float64) - gt)[v] > 1).mean())
