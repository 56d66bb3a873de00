"""numpy restatement of SM_PARAM_SGM_PATHS (include/sm_hip.h): SM_AGG_SGM's sum over four or eight scan directions.

The four directions of ``sgm_ref`` stay ``sgm_ref.path``.  With 8 paths S is also summed over the diagonals
rho in {(+1,+1), (-1,+1), (+1,-1), (-1,-1)}, under the recursion, existence rule (x + d <= W) and penalties that
``sgm_ref`` states: with q = p - rho,
    L(p, d) = C(p, d)                                                              q outside the image
    L(p, d) = C(p, d) + min(L(q, d), L(q, d-1) + P1, L(q, d+1) + P1, M + P2) - M   M = min over existing k of L(q, k)
For a diagonal, q is outside the image in the first row of the walk and in the column the path enters by.  The
diagonal scan walks the rows, shifts the previous row's L by dx and restarts the entering column; the other two axes
are vectorised.  Everything after S is ``sgm_ref``'s: SENTINEL where a pair does not exist, the first minimum,
``oracle.right_wta`` and ``oracle.lr_check``.
"""
import numpy as np

import sgm_ref
from sgm_ref import SENTINEL, _INF, _step, exists

DIAGONALS = ((1, 1), (-1, 1), (1, -1), (-1, -1))   # rho = (dx, dy)


def directions(paths: int):
    if paths not in (4, 8):
        raise ValueError(f"paths must be 4 or 8, got {paths}")
    return sgm_ref.DIRECTIONS + (DIAGONALS if paths == 8 else ())


def diagonal_path(C: np.ndarray, rho, P1: int, P2: int) -> np.ndarray:
    """L_rho [D, H, W] int64 (_INF where the pair does not exist) for a diagonal rho = (+-1, +-1)."""
    C = np.asarray(C, np.int64)
    D, H, W = C.shape
    dx, dy = rho
    assert abs(dx) == 1 and abs(dy) == 1
    E = exists(D, W)
    L = np.full((D, H, W), _INF, np.int64)
    enter = 0 if dx > 0 else W - 1   # the column whose q = (x - dx, y - dy) is outside the image in every row
    prev = None
    for y in (range(H) if dy > 0 else range(H - 1, -1, -1)):
        start = np.where(E, C[:, y, :], _INF)
        if prev is None:
            cur = start
        else:
            q = np.full((D, W), _INF, np.int64)   # the previous row's L at x - dx; the entering column has none
            if dx > 0:
                q[:, 1:] = prev[:, :-1]
            else:
                q[:, :-1] = prev[:, 1:]
            cur = _step(C[:, y, :], q, E, P1, P2)
            cur[:, enter] = start[:, enter]       # the path starts here: L = C
        L[:, y, :] = cur
        prev = cur
    return L


def path(C: np.ndarray, rho, P1: int, P2: int) -> np.ndarray:
    """sgm_ref.path for the four axis directions, diagonal_path for the diagonals."""
    return diagonal_path(C, rho, P1, P2) if rho[0] and rho[1] else sgm_ref.path(C, rho, P1, P2)


def aggregate(C: np.ndarray, P1: int, P2: int, paths: int = 4, path_fn=path):
    """(S int64 [D, H, W] with SENTINEL where the pair does not exist, left map uint8 [H, W])."""
    C = np.asarray(C, np.int64)
    D, H, W = C.shape
    E = np.broadcast_to(exists(D, W)[:, None, :], (D, H, W))
    S = np.zeros((D, H, W), np.int64)
    for rho in directions(paths):
        S += np.where(E, path_fn(C, rho, P1, P2), 0)
    S = np.where(E, S, SENTINEL)
    return S, np.argmin(S, axis=0).astype(np.uint8)   # first minimum = smallest d


def maps(oracle, S: np.ndarray, dl: np.ndarray, median: bool = False):
    """(left map, right map, checked map, mask) from S and its left map, as sgm_ref.sgm_lr forms them."""
    dr = oracle.right_wta(S.astype(np.int32))
    if median:
        dl, dr = oracle.median(dl, 3), oracle.median(dr, 3)
    checked, mask = oracle.lr_check(dl, dr)
    return dl, dr, checked, mask


def sgm_lr(oracle, left, right, radius: int, D: int, P1: int, P2: int, median: bool = False, paths: int = 4):
    """sgm_ref.sgm_lr with the path count: (left map, right map, checked map, mask) on a gray pair."""
    S, dl = aggregate(oracle.box_cost(left, right, radius, D), P1, P2, paths)
    return maps(oracle, S, dl, median)
