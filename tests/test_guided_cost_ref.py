"""tests/guided_cost_ref.py against the fp64 oracle, and its error bound against an fp32 emulation (no GPU).

The emulation runs the restated formulas with fp32 intermediates in one plain summation order (2r + 1
sequential adds per axis).  It is not a model of the kernel: it shows, before a GPU sees the bound, that
|q32 - q64| <= C 2^-24 M has the right form and room on every texture class of the GPU cost test.
"""
import numpy as np
import pytest

import guided_cost_ref as G
from guided_check import TOL

f32 = np.float32


def _box_f32(a, r):
    H, W = a.shape
    p = np.zeros((H + 2 * r, W), f32)
    p[r:r + H] = a
    v = np.zeros((H, W), f32)
    for k in range(2 * r + 1):
        v = v + p[k:k + H]
    p = np.zeros((H, W + 2 * r), f32)
    p[:, r:r + W] = v
    out = np.zeros((H, W), f32)
    for k in range(2 * r + 1):
        out = out + p[:, k:k + W]
    assert out.dtype == f32
    return out


def emulate_fp32(L, R, r, d, eps):
    N, SI, SII, Sp, SIp = G.window_sums(L, R, r, d)
    Nf = N.astype(f32)
    den = (N * SII - SI * SI).astype(f32) + f32(eps) * Nf * Nf
    a = (N * SIp - SI * Sp).astype(f32) * (f32(1) / den)
    b = (Sp.astype(f32) - a * SI.astype(f32)) * (f32(1) / Nf)
    q = (_box_f32(a, r) * np.asarray(L, f32) + _box_f32(b, r)) * (f32(1) / Nf)
    assert q.dtype == f32
    return q.astype(np.float64)


@pytest.mark.parametrize("r", [0, 2, 5, 7])
def test_restatement_equals_oracle(oracle, r):
    """q of every d, the x < d zone and d > W - x included, on a ragged frame; D > W: the last d have p = 0."""
    W, H, D = 53, 29, 60
    L, R = oracle.synth_pair(77 + r, W, H, 32)
    for eps in (G.EPS_DEFAULT, 1.0):
        _, q, _ = oracle.guided_disp(L, R, r, D, eps, want_q=True)
        for d in range(D):
            got, M = G.guided_cost(L, R, r, d, eps)
            assert np.abs(got - q[d]).max() <= 1e-9, (r, eps, d)
            assert (M >= np.abs(got) - 1e-9).all(), (r, eps, d)   # M bounds |q| term by term


def test_fp32_emulation_inside_the_bound(oracle, gray, capsys):
    rows, worst_own = [], 0.0
    for r, W, H, ds in G.cost_shapes():
        tex = G.texture_classes(gray, oracle, W, H)
        assert set(tex) == set(G.OWN_CLASSES) | {"bright", "step"}
        for name, (L, R) in tex.items():
            for eps in G.eps_values(name):
                err_max, ratio_max = 0.0, 0.0
                for d in ds:
                    q, M = G.guided_cost(L, R, r, d, eps)
                    assert (np.abs(q) < G.Q_CLAMP).all()
                    err = np.abs(emulate_fp32(L, R, r, d, eps) - q)
                    assert (err <= G.roundings(r) * G.U32 * M).all(), (r, W, name, eps, d)
                    err_max = max(err_max, float(err.max()))
                    ratio_max = max(ratio_max, float((err[M > 0] / (G.U32 * M[M > 0])).max(initial=0.0)))
                rows.append((r, W, name, eps, err_max, ratio_max))
                if G.tol_half_applies(name, eps):
                    worst_own = max(worst_own, err_max)
    with capsys.disabled():
        print()
        for r, W in dict.fromkeys((r, W) for r, W, *_ in rows):
            mine = [x for x in rows if x[:2] == (r, W)]
            e, k = max(mine, key=lambda x: x[4]), max(mine, key=lambda x: x[5])
            print(f"fp32 emulation r={r} W={W}: max err {e[4]:.3e} ({e[2]}, eps {e[3]:g})  "
                  f"max err/(2^-24 M) {k[5]:.2f} ({k[2]}, eps {k[3]:g})  (C = {G.roundings(r)})")
        print(f"fp32 emulation, the project's own classes: max err {worst_own:.3e} (TOL / 2 = {TOL / 2:.1e})")
    # the project's own classes: what the tie-aware TOL needs of the costs (this emulation measured 2.3e-4)
    assert worst_own <= TOL / 2, worst_own


def test_decode_round_trip():
    fields = [-3, 0, 1, 819199, 819200, -(1 << 23), (1 << 23) - 1]
    ds = [0, 1, 77, 254]
    keys = np.array([[(f << 8) | d for d in ds] for f in fields], np.int64)
    assert keys.min() == -(1 << 31) and keys.max() < G.INT32_MAX
    keys = np.concatenate([keys, np.full((1, len(ds)), G.INT32_MAX, np.int64)]).astype(np.int32)
    cost, d, empty = G.decode(keys)
    assert np.array_equal(empty, np.repeat([[False]] * len(fields) + [[True]], len(ds), axis=1))
    assert np.array_equal(d[:-1], np.tile(ds, (len(fields), 1)))
    assert np.array_equal(cost[:-1], np.repeat(np.array(fields, np.float64)[:, None] / 16384.0, len(ds), axis=1))
    assert cost[0, 0] == -3 / 16384.0 and cost[5, 0] == -512.0 and cost[6, 0] == 512.0 - 2.0 ** -14
    # a cost of exactly q (no truncation) round-trips through the kernel's (int)(q * 2^14) << 8 | d
    q = np.array([-1.25, 0.0, 49.99993896484375, 50.0])
    k = ((q * 16384.0).astype(np.int64) << 8 | 9).astype(np.int32)
    assert np.array_equal(G.decode(k)[0], q) and (G.decode(k)[1] == 9).all()
