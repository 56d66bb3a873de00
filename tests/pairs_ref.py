"""numpy restatement of SM_PAIRS_IN_VIEW and SM_PARAM_MIN_DISP (include/sm_hip.h), parameterised by (rule, d0).

Plane k of a volume stands for the disparity d = d0 + k, k = 0 .. D - 1.  Which pairs (x, k) exist:
    rule 'reference' (d0 = 0)   x + d <= W (Device.cu:44):     kmax(x) = min(D - 1, W - x)
    rule 'in-view'              x - (d0 + k) >= 0:             kmax(x) = min(D - 1, x - d0), negative where x < d0
    right view, V_R(u, k) = V(u + d0 + k, k):
        'reference'             u + 2 d <= W (right_pairs 1) or u + d < W (right_pairs 2, the AD box volume)
        'in-view'               u + d0 + k <= W - 1, for every volume
Both are prefixes of the planes.  The costs: plane k compares L(y, x) with R(y, x - d0 - k) and is 0 for x < d0 + k; the
zero-padded box window sum is unchanged.  The recursion, the penalties, the first minimum and the parabola are
``sgm_ref``'s and ``subpix_ref``'s; a previous pixel q with no existing k acts as a q outside the image, which needs no
branch: with every L(q, .) at _INF = 2^40, M = _INF and min(...) - M = 0 (the kernels' 2^20 does the same).  The maps
hold the absolute disparity, d0 + k0 and 16 (d0 + k0) + delta; a pixel with no candidate gives 0 in either map and 0
in the mask, in either view.  Under ('reference', 0) everything here equals sgm_ref / sgm_paths_ref / subpix_ref /
census_ref (tests/test_pairs_ref.py), whose helpers it imports and does not change.
"""
import functools

import numpy as np

import census_ref
import sgm_paths_ref
import sgm_ref
import subpix_ref
from sgm_ref import SENTINEL, _INF, _step

RULES = ("reference", "in-view")


def _rule(rule, d0):
    if rule not in RULES:
        raise ValueError(f"rule must be one of {RULES}")
    if d0 < 0 or (d0 and rule != "in-view"):
        raise ValueError("a minimum disparity needs the in-view rule")


# ---- existence ----
def kmax(rule: str, D: int, W: int, d0: int = 0) -> np.ndarray:
    """int64 [W]: the largest existing k of the left view at column x (negative: none)."""
    _rule(rule, d0)
    x = np.arange(W, dtype=np.int64)
    return np.minimum(D - 1, W - x if rule == "reference" else x - d0)


def right_kmax(rule: str, D: int, W: int, d0: int = 0, right_pairs: int = 1) -> np.ndarray:
    """int64 [W]: the largest existing k of the right view at column u."""
    _rule(rule, d0)
    u = np.arange(W, dtype=np.int64)
    if rule == "in-view":
        return np.minimum(D - 1, W - 1 - u - d0)
    return np.minimum(D - 1, (W - u) // 2 if right_pairs == 1 else W - 1 - u)


def exists(rule: str, D: int, W: int, d0: int = 0) -> np.ndarray:
    """bool [D, W]: the pair (x, k) exists in the left view."""
    return np.arange(D)[:, None] <= kmax(rule, D, W, d0)[None, :]


def right_exists(rule: str, D: int, W: int, d0: int = 0, right_pairs: int = 1) -> np.ndarray:
    return np.arange(D)[:, None] <= right_kmax(rule, D, W, d0, right_pairs)[None, :]


def _e3(E, H):
    return np.broadcast_to(E[:, None, :], (E.shape[0], H, E.shape[1]))


# ---- costs ----
def ad_volume(left, right, D: int, d0: int = 0) -> np.ndarray:
    """uint8 [D, H, W]: |L(y, x) - R(y, x - d0 - k)| for x >= d0 + k, 0 otherwise."""
    L, R = np.asarray(left, np.int16), np.asarray(right, np.int16)
    H, W = L.shape
    vol = np.zeros((D, H, W), np.uint8)
    for k in range(D):
        d = d0 + k
        if d < W:
            vol[k, :, d:] = np.abs(L[:, d:] - R[:, :W - d])
    return vol


def hamming_volume(left, right, D: int, d0: int = 0) -> np.ndarray:
    """uint8 [D, H, W]: popcount(censusL(y, x) ^ censusR(y, x - d0 - k)) for x >= d0 + k, 0 otherwise."""
    cl, cr = census_ref.census(left), census_ref.census(right)
    H, W = cl.shape
    ham = np.zeros((D, H, W), np.uint8)
    for k in range(D):
        d = d0 + k
        if d < W:
            ham[k, :, d:] = census_ref._popcount(cl[:, d:] ^ cr[:, :W - d])
    return ham


def cost(left, right, r: int, D: int, kind: str = "ad", d0: int = 0) -> np.ndarray:
    """int64 [D, H, W]: the zero-padded (2r+1)^2 window sum of the AD or the Hamming volume."""
    vol = hamming_volume(left, right, D, d0) if kind == "census" else ad_volume(left, right, D, d0)
    return census_ref.box_sum(vol, r).astype(np.int64)


def auto_penalties(radius: int, kind: str = "ad"):
    return (census_ref if kind == "census" else sgm_ref).auto_penalties(radius)


# ---- the path scans, all eight directions ----
def path(C: np.ndarray, rho, P1: int, P2: int, E: np.ndarray) -> np.ndarray:
    """L_rho [D, H, W] int64 (_INF where the pair does not exist); E bool [D, W] is the left view's existence."""
    C = np.asarray(C, np.int64)
    D, H, W = C.shape
    dx, dy = rho
    L = np.full((D, H, W), _INF, np.int64)
    if dy == 0:                      # along the row: the other two axes are vectorised
        prev = None
        for x in (range(W) if dx > 0 else range(W - 1, -1, -1)):
            Ex = np.broadcast_to(E[:, x:x + 1], (D, H))
            cur = np.where(Ex, C[:, :, x], _INF) if prev is None else _step(C[:, :, x], prev, Ex, P1, P2)
            L[:, :, x] = cur
            prev = cur
        return L
    prev = None
    for y in (range(H) if dy > 0 else range(H - 1, -1, -1)):
        start = np.where(E, C[:, y, :], _INF)
        if prev is None:
            cur = start
        elif dx == 0:
            cur = _step(C[:, y, :], prev, E, P1, P2)
        else:                        # the previous row's L at x - dx; the entering column restarts
            q = np.full((D, W), _INF, np.int64)
            if dx > 0:
                q[:, 1:] = prev[:, :-1]
            else:
                q[:, :-1] = prev[:, 1:]
            cur = _step(C[:, y, :], q, E, P1, P2)
            enter = 0 if dx > 0 else W - 1
            cur[:, enter] = start[:, enter]
        L[:, y, :] = cur
        prev = cur
    return L


def path_literal(C: np.ndarray, rho, P1: int, P2: int, rule: str, d0: int = 0) -> np.ndarray:
    """The same, as the per-pixel triple loop of the contract (small sizes only).  A q inside the image with no
    existing k is treated as a q outside it, explicitly."""
    _rule(rule, d0)
    D, H, W = C.shape
    dx, dy = rho
    if rule == "reference":
        ex = lambda x, k: 0 <= k < D and x + k <= W            # noqa: E731
    else:
        ex = lambda x, k: 0 <= k < D and x - (d0 + k) >= 0     # noqa: E731
    L = np.full((D, H, W), _INF, np.int64)
    for y in (range(H) if dy >= 0 else range(H - 1, -1, -1)):
        for x in (range(W) if dx >= 0 else range(W - 1, -1, -1)):
            qx, qy = x - dx, y - dy
            prior = [int(L[k, qy, qx]) for k in range(D) if ex(qx, k)] if 0 <= qx < W and 0 <= qy < H else []
            for k in range(D):
                if not ex(x, k):
                    continue
                if not prior:
                    L[k, y, x] = int(C[k, y, x])
                    continue
                M = min(prior)
                terms = [M + P2]
                if ex(qx, k):
                    terms.append(int(L[k, qy, qx]))
                if ex(qx, k - 1):
                    terms.append(int(L[k - 1, qy, qx]) + P1)
                if ex(qx, k + 1):
                    terms.append(int(L[k + 1, qy, qx]) + P1)
                L[k, y, x] = int(C[k, y, x]) + min(terms) - M
    return L


def aggregate(C: np.ndarray, P1: int, P2: int, paths: int = 4, rule: str = "reference", d0: int = 0,
              path_fn=None) -> np.ndarray:
    """S int64 [D, H, W]: the sum of the four or eight L, SENTINEL where the pair does not exist."""
    C = np.asarray(C, np.int64)
    D, H, W = C.shape
    E = exists(rule, D, W, d0)
    fn = path_fn or (lambda C_, rho: path(C_, rho, P1, P2, E))
    E3 = _e3(E, H)
    S = np.zeros((D, H, W), np.int64)
    for rho in sgm_paths_ref.directions(paths):
        S += np.where(E3, fn(C, rho), 0)
    return np.where(E3, S, SENTINEL)


def box_volume(C: np.ndarray, rule: str = "reference", d0: int = 0) -> np.ndarray:
    """A cost volume taken without SGM (the census box WTA): C with SENTINEL where the pair does not exist."""
    D, H, W = C.shape
    return np.where(_e3(exists(rule, D, W, d0), H), np.asarray(C, np.int64), SENTINEL)


# ---- views ----
def right_volume(V: np.ndarray, rule: str = "reference", d0: int = 0, right_pairs: int = 1):
    """(V_R int64 [D, H, W], its existence [D, H, W]): V_R(u, k) = V(u + d0 + k, k)."""
    V = np.asarray(V, np.int64)
    D, H, W = V.shape
    VR = np.full((D, H, W), SENTINEL, np.int64)
    for k in range(D):
        d = d0 + k
        if d < W:
            VR[k, :, :W - d] = V[k, :, d:]
    return VR, _e3(right_exists(rule, D, W, d0, right_pairs), H)


def wta8(V: np.ndarray, E: np.ndarray, d0: int = 0) -> np.ndarray:
    """uint8 [H, W]: d0 + the first k at min V over the existing k; 0 where the pixel has no candidate."""
    Vs = np.where(E, np.asarray(V, np.int64), SENTINEL)
    any_k = E.any(axis=0)
    return np.where(any_k, d0 + np.argmin(Vs, axis=0), 0).astype(np.uint8)


def lr_check(dl: np.ndarray, dr: np.ndarray):
    """(checked map, mask uint8): occluded when x - d < 0, d == 0 or |d - dR(x - d)| > 1, on absolute disparities."""
    occ = subpix_ref.lr_occluded(dl, dr)
    return np.where(occ, 0, dl).astype(dl.dtype), (~occ).astype(np.uint8)


def maps8(V: np.ndarray, rule: str = "reference", d0: int = 0, right_pairs: int = 1, median=None):
    """(left, right, checked, mask) of the 8-bit calls from a volume V (SGM's sums or a box cost).  median: a function
    applied to both maps before the check (SM_MEDIAN)."""
    D, H, W = V.shape
    dl = wta8(V, _e3(exists(rule, D, W, d0), H), d0)
    dr = wta8(*right_volume(V, rule, d0, right_pairs), d0)
    if median:
        dl, dr = median(dl), median(dr)
    checked, mask = lr_check(dl, dr)
    return dl, dr, checked, mask


def view16(V: np.ndarray, E: np.ndarray, d0: int = 0, u: int = 0, invalid_from: int = 0):
    """One view of the sub-pixel rule: (q uint16, absolute d uint16, valid bool), 0 / 0 / False where the pixel is
    invalid or has no candidate.  subpix_ref.view's rule on the planes, with d0 added and 16-bit disparities."""
    V = np.asarray(V, np.int64)
    D = V.shape[0]
    Vs = np.where(E, V, SENTINEL)
    k0 = np.argmin(Vs, axis=0)                   # the first minimum
    km = E.sum(axis=0) - 1                       # E is a prefix of the planes
    pick = lambda k: np.take_along_axis(Vs, np.clip(k, 0, D - 1)[None], axis=0)[0]   # noqa: E731
    a, b, c = pick(k0 - 1), pick(k0), pick(k0 + 1)
    inner = (k0 >= 1) & (k0 < km)
    den = np.where(inner, a + c - 2 * b, 1)
    assert (den >= 1).all()
    delta = np.where(inner, (16 * (a - c) + den) // (2 * den), 0)   # // floors
    valid = km >= 0
    if invalid_from:
        valid = valid & (b < invalid_from)
    if u:
        far = np.abs(np.arange(D)[:, None, None] - k0[None]) > 1
        valid = valid & ~(E & far & (V * (100 - u) < b[None] * 100)).any(axis=0)
    qa = np.where(valid, 16 * (d0 + k0) + delta, 0)
    assert qa.max(initial=0) <= 65535
    return qa.astype(np.uint16), np.where(valid, d0 + k0, 0).astype(np.uint16), valid


def view16_literal(V: np.ndarray, E: np.ndarray, d0: int = 0, u: int = 0, invalid_from: int = 0):
    """The same, as the per-pixel loop of the contract (small sizes only)."""
    D, H, W = V.shape
    q = np.zeros((H, W), np.uint16)
    da = np.zeros((H, W), np.uint16)
    valid = np.zeros((H, W), bool)
    for y in range(H):
        for x in range(W):
            ks = [k for k in range(D) if E[k, y, x]]
            if not ks:
                continue
            km = ks[-1]
            assert ks == list(range(km + 1))
            v = [int(V[k, y, x]) for k in ks]
            b = min(v)
            k0 = v.index(b)
            delta = 0
            if 1 <= k0 < km:
                a, c = v[k0 - 1], v[k0 + 1]
                den = a + c - 2 * b
                delta = (16 * (a - c) + den) // (2 * den)
            ok = not (invalid_from and b >= invalid_from)
            if u and any(abs(k - k0) > 1 and v[k] * (100 - u) < b * 100 for k in ks):
                ok = False
            if ok:
                q[y, x], da[y, x], valid[y, x] = 16 * (d0 + k0) + delta, d0 + k0, True
    return q, da, valid


def subpix(V: np.ndarray, rule: str = "reference", d0: int = 0, u: int = 0, invalid_from: int = 0, lr: bool = False,
           right_pairs: int = 1, view_fn=view16):
    """(q uint16, right-view q uint16, mask uint8) of a cost volume V [D, H, W]."""
    V = np.asarray(V, np.int64)
    D, H, W = V.shape
    q, dl, valid = view_fn(V, _e3(exists(rule, D, W, d0), H), d0, u, invalid_from)
    qr, dr, _ = view_fn(*right_volume(V, rule, d0, right_pairs), d0, u, 0)
    if lr:
        occ = subpix_ref.lr_occluded(dl, dr)
        q = np.where(occ, 0, q).astype(np.uint16)
        valid = ~occ
    return q, qr, valid.astype(np.uint8)


# ---- one pair, every path, the volumes computed once ----
class Reference:
    """The expected results of the matching calls on one pair under (rule, d0): agg 'sgm' or 'box', cost 'ad' or
    'census'; p1 / p2 0 = auto, per cost."""

    def __init__(self, L, R, r, D, rule="reference", d0=0, p1=0, p2=0, paths=4):
        _rule(rule, d0)
        self.L, self.R, self.r, self.D, self.rule, self.d0 = L, R, r, D, rule, d0
        self.p1, self.p2, self.paths = p1, p2, paths

    @functools.lru_cache(maxsize=None)
    def cost(self, kind):
        return cost(self.L, self.R, self.r, self.D, kind, self.d0)

    def penalties(self, kind):
        a1, a2 = auto_penalties(self.r, kind)
        return self.p1 or a1, self.p2 or a2

    @functools.lru_cache(maxsize=None)
    def volume(self, agg, kind, paths=None):
        """(V with SENTINEL where the pair does not exist, invalid_from, right_pairs)."""
        if agg == "sgm":
            return aggregate(self.cost(kind), *self.penalties(kind), paths or self.paths, self.rule, self.d0), 0, 1
        if kind == "census":
            return box_volume(self.cost(kind), self.rule, self.d0), 0, 1
        return self.cost(kind), 50 * (2 * self.r + 1) ** 2, 2   # the AD box volume: the sub-pixel calls alone

    @functools.lru_cache(maxsize=None)
    def maps(self, agg, kind, paths=None):
        V, _, rp = self.volume(agg, kind, paths)
        return maps8(V, self.rule, self.d0, rp)

    @functools.lru_cache(maxsize=None)
    def subpix(self, agg, kind, u=0, lr=False, paths=None):
        V, invalid_from, rp = self.volume(agg, kind, paths)
        return subpix(V, self.rule, self.d0, u, invalid_from, lr, rp)


def bad_rate(disp: np.ndarray, gt: np.ndarray, cols=slice(None)) -> float:
    """sgm_ref.bad_rate on a range of columns."""
    return sgm_ref.bad_rate(disp[:, cols], gt[:, cols])
