"""fp64 numpy restatement of the guided filter's cost q(d), with the scale of its fp32 error.

guided_cost() restates the formulas of csrc/bm_guided.hip's header from integer integral images:
    N, SI, SII, Sp, SIp   clipped-window count and sums, p = |L(x) - R(x - d)|, p = 0 for x < d
    a = (N SIp - SI Sp) / (N SII - SI^2 + eps N^2),   b = (Sp - a SI) / N
    q = (box(a) I + box(b)) / N
and returns beside q the magnitude M of what the kernel's fp32 path sums,
    M = (I box_ext(|a|) + box_ext(|b| + |a| SI / N)) / N,
box_ext being the clipped window sum of radius r + 8: the kernel's float running sums restart every
8 rows (S2V) and every SW2 <= 8 columns (S2H), so a sum has seen its own window and at most 7 rows or
columns of history.  A kernel cost is accepted within cost_bound(r, M).

roundings(r), the C of  |q_gpu - q64| <= 2^-14 + C 2^-24 M,  from the kernel stage by stage
(u = 2^-24, first order; every integer up to the numerators N SIp - SI Sp and N SII - SI^2 is exact):
  stats  den = float(N SII - SI^2) + (eps * float(N)) * float(N): one conversion, two products and one
         add of non-negative terms, then invden = 1 / den: 5 roundings relative to den.
  S1H    a = float(num) * invden: a conversion and a product, so |da| <= 7 u |a|.
         b = fma(-a, float(SI), float(Sp)) * invN: float(SI) and float(Sp) are exact; the fma, 1 / N and the
         product round, so |db| <= 3 u |b| + 7 u |a| SI / N.  This is where M's |a| SI / N comes from.
  S2V    a running sum per A column: 2r warm-up adds, then at most 8 adds and 7 subtracts before it
         restarts: 2r + 15 roundings, each at most u times the sum of |terms| seen so far (box_ext).
  S2H    the same along the row over a segment of SW2 <= 8 outputs: 2r + 15.
  S2H    N q = fma(sum a, I, sum b): 1 (I is exact, also as the f16 of the right-view kernels).
  key    scale = 2^14 / float(N) (2^22 / N for the right keys): 1; (N q) * scale: 1.
That is 7 + 2 (2r + 15) + 3 on the a terms and 3 + 2 (2r + 15) + 3 on the b terms, 2 (2r + 15) + 10 at
most, with correctly rounded divisions (the build does not relax them).  The bound keeps
2 (2r + 15) + 12: the two roundings more cover the three divisions at 1 ulp instead of 1/2 and the
second-order terms, and the count was not lowered to what the code needs at the least.
The key's truncation (toward zero for the left keys, toward -inf below 2^-22 for the right keys) adds
less than 2^-14.
"""
import numpy as np

INT32_MAX = 0x7FFFFFFF
KEY_SCALE = float(1 << 14)
TRUNC = 2.0 ** -14
U32 = 2.0 ** -24
HISTORY = 8            # box_ext radius beyond r (S2V restarts every 8 rows, SW2 <= 8)
Q_CLAMP = 511.0        # keys clamp at |q| >= 512


def roundings(r):
    return 2 * (2 * r + 15) + 12


def cost_bound(r, M):
    return TRUNC + roundings(r) * U32 * M


def box_int(a, r):
    """Clipped-window sums of an integer plane, exactly, from its integral image."""
    a = np.asarray(a, np.int64)
    H, W = a.shape
    ii = np.zeros((H + 1, W + 1), np.int64)
    ii[1:, 1:] = a.cumsum(0).cumsum(1)
    y0, y1 = np.clip(np.arange(H) - r, 0, H), np.clip(np.arange(H) + r + 1, 0, H)
    x0, x1 = np.clip(np.arange(W) - r, 0, W), np.clip(np.arange(W) + r + 1, 0, W)
    return ii[y1][:, x1] - ii[y0][:, x1] - ii[y1][:, x0] + ii[y0][:, x0]


def box_f64(a, r):
    """Clipped-window sums of a float plane: 2r + 1 shifted adds per axis (no prefix-sum cancellation)."""
    a = np.asarray(a, np.float64)
    H, W = a.shape
    p = np.zeros((H + 2 * r, W), np.float64)
    p[r:r + H] = a
    v = np.zeros((H, W), np.float64)
    for k in range(2 * r + 1):
        v += p[k:k + H]
    p = np.zeros((H, W + 2 * r), np.float64)
    p[:, r:r + W] = v
    out = np.zeros((H, W), np.float64)
    for k in range(2 * r + 1):
        out += p[:, k:k + W]
    return out


def window_sums(L, R, r, d):
    """(N, SI, SII, Sp, SIp) as int64 planes; p = |L(x) - R(x - d)|, 0 for x < d."""
    I = np.asarray(L, np.int64)
    H, W = I.shape
    p = np.zeros((H, W), np.int64)
    if d < W:
        p[:, d:] = np.abs(I[:, d:] - np.asarray(R, np.int64)[:, :W - d])
    return (box_int(np.ones((H, W), np.int64), r), box_int(I, r), box_int(I * I, r), box_int(p, r),
            box_int(I * p, r))


def guided_cost(L, R, r, d, eps):
    """(q, M): the fp64 cost of disparity d at every pixel and the fp32 path's magnitude (module docstring)."""
    N, SI, SII, Sp, SIp = window_sums(L, R, r, d)
    Nf = N.astype(np.float64)
    a = (N * SIp - SI * Sp).astype(np.float64) / ((N * SII - SI * SI).astype(np.float64) + float(eps) * Nf * Nf)
    b = (Sp - a * SI) / Nf
    I = np.asarray(L, np.float64)
    q = (box_f64(a, r) * I + box_f64(b, r)) / Nf
    M = (I * box_f64(np.abs(a), r + HISTORY) + box_f64(np.abs(b) + np.abs(a) * SI / Nf, r + HISTORY)) / Nf
    return q, M


def decode(keys):
    """Guided keys -> (cost = the signed field keys >> 8 over 2^14, d field, empty = INT32_MAX)."""
    k = np.asarray(keys)
    assert k.dtype == np.int32
    return (k >> 8).astype(np.float64) / KEY_SCALE, (k & 0xFF).astype(np.int64), k == INT32_MAX


# ---- the texture classes of the cost tests (tests/test_guided_cost_ref.py, tests/test_gpu_guided_cost.py) ----
EPS_DEFAULT = 1e-4 * 255 * 255
OWN_CLASSES = ("art", "synth", "fuzz", "binary")      # the project's own inputs: also held to TOL / 2
EPS_SWEEP_CLASSES = ("synth", "bright", "step")       # also run at eps = 1.0 and 5000.0


def texture_classes(gray, oracle, W, H):
    """name -> (L, R), uint8 [H, W], deterministic in (W, H)."""
    from fuzz_util import fuzz_pair
    rng = np.random.default_rng(1000 * W + H)
    out = {}
    A1, A5 = gray["Art_/view1"], gray["Art_/view5"]
    y0, x0 = (A1.shape[0] - H) // 2, (A1.shape[1] - W) // 2
    out["art"] = (A1[y0:y0 + H, x0:x0 + W], A5[y0:y0 + H, x0:x0 + W])
    out["synth"] = oracle.synth_pair(W * 5 + H, W, H, 64)
    out["fuzz"] = fuzz_pair(rng, W, H)
    Lb = np.where(rng.random((H, W)) < 0.5, 0, 255).astype(np.uint8)
    flip = rng.random((H, W)) < 0.05
    out["binary"] = (Lb, np.where(flip, 255 - np.roll(Lb, -7, axis=1), np.roll(Lb, -7, axis=1)).astype(np.uint8))
    out["bright"] = (rng.integers(250, 256, (H, W), dtype=np.uint8), rng.integers(0, 6, (H, W), dtype=np.uint8))
    step = np.where(np.arange(W)[None, :] < W // 2, 255, 0).repeat(H, 0).astype(np.uint8)
    out["step"] = (step ^ rng.integers(0, 2, (H, W), dtype=np.uint8),
                   (255 - step) ^ rng.integers(0, 2, (H, W), dtype=np.uint8))
    return {k: (np.ascontiguousarray(l), np.ascontiguousarray(r)) for k, (l, r) in out.items()}


def eps_values(name):
    return (EPS_DEFAULT, 1.0, 5000.0) if name in EPS_SWEEP_CLASSES else (EPS_DEFAULT,)


def tol_half_applies(name, eps):
    """The project's own input classes at eps = 1e-4 255^2 and 5000: the tie-aware TOL needs err <= TOL / 2 there."""
    return name in OWN_CLASSES and eps in (EPS_DEFAULT, 5000.0)


def cost_shapes():
    """(r, W, H, disparities): two tiles and 5 columns wide, a second tile row, for every radius; one wider frame."""
    out = []
    for r in range(8):
        TW = 64 - 4 * r
        W = 2 * TW + 5
        out.append((r, W, 41, (0, 1, 2, 31, 32, 33, 63, 64, 65, W - 1, W)))
    out.append((5, 300, 33, (127, 128, 255)))
    return out
