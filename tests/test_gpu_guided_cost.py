"""The guided kernel's costs, not only its choices, against the fp64 restatement (tests/guided_cost_ref.py).

A one-disparity slice (valid_mode 2: no threshold, the best cost starts at +inf) returns trunc(q(d) 2^14) of
every valid pixel, from the left-only kernel (guided_slice_keys_device) and from the fused right-view
kernels (slice_keys_lr_device, whose right key of u carries C_R(u, d) = q(u + d, d)).  So the whole cost
volume of every kernel variant is compared with fp64:
    every case                 |q_gpu - q64| <= 2^-14 + C 2^-24 M    (C, M: guided_cost_ref's docstring)
    the project's own classes  |q_gpu - q64| <= TOL / 2 + 2^-14      (art, synth, fuzz, binary at eps =
                               1e-4 255^2 and 5000): with a cost error e the kernel's winner is within 2 e of
                               the oracle's best, so guided_check's tie-aware TOL is sound where e <= TOL / 2.
Each test prints its largest error and largest (err - 2^-14) / (2^-24 M), to be read against C, per
(r, kernel variant, texture class).
"""
import numpy as np
import pytest

import guided_cost_ref as G
from guided_check import TOL

pytestmark = pytest.mark.gpu

# the fused right-view kernel's build per radius (bm_guided.hip: kGuidedRoles, LEAN = the wave roles with I as f16
# pairs read by v_fma_mix_f32; r = 3 runs it at 2 waves/SIMD, r = 2, 6, 7 run without the roles, f32 fma)
LR_VARIANT = {0: "lean", 1: "lean", 2: "no roles", 3: "lean, 2 waves", 4: "lean", 5: "lean", 6: "no roles",
              7: "no roles"}
SHAPES = G.cost_shapes()
SHAPE_IDS = [f"r{r}-W{W}" for r, W, _, _ in SHAPES]


@pytest.fixture(scope="module")
def torch():
    import torch as t
    assert t.cuda.is_available()
    return t


@pytest.fixture(scope="module")
def matcher():
    import gpu_stereo_matching_amd as sm
    m = sm.BlockMatcher(0, 512, 256, 256)
    yield m
    m.set_guided_eps(G.EPS_DEFAULT)
    m.close()


_TEX, _REF = {}, {}


def _textures(gray, oracle, W, H):
    if (W, H) not in _TEX:
        _TEX[W, H] = G.texture_classes(gray, oracle, W, H)
    return _TEX[W, H]


def _reference(L, R, r, W, H, name, eps, d):
    """(q, M) of one case, computed once for the left-only and the fused tests and never written to."""
    key = (r, W, H, name, eps, d)
    if key not in _REF:
        q, M = G.guided_cost(L, R, r, d, eps)
        q.setflags(write=False)
        M.setflags(write=False)
        _REF[key] = (q, M)
    return _REF[key]


class _Report:
    """Largest error and largest excess ratio per (variant, class); failures collected, asserted at the end."""

    def __init__(self, r):
        self.r, self.rows, self.fails, self.skipped = r, {}, [], 0

    def cost(self, variant, name, eps, d, got, q, M, where):
        """got, q, M: the pixels of `where` (a mask over the frame, for the messages' counts only)."""
        clamped = np.abs(q) >= G.Q_CLAMP
        self.skipped += int(clamped.sum())
        got, q, M = got[~clamped], q[~clamped], M[~clamped]
        err = np.abs(got - q)
        excess = np.maximum(err - G.TRUNC, 0.0)
        ratio = np.where(M > 0, excess / np.where(M > 0, G.U32 * M, 1.0), np.where(excess > 0, np.inf, 0.0))
        row = self.rows.setdefault((variant, name), [0.0, 0.0])
        row[0] = max(row[0], float(err.max(initial=0.0)))
        row[1] = max(row[1], float(ratio.max(initial=0.0)))
        bad = err > G.cost_bound(self.r, M)
        if bad.any():
            self.fails.append(f"{variant} {name} eps={eps:g} d={d}: {int(bad.sum())} of {int(where.sum())} costs "
                              f"outside 2^-14 + C 2^-24 M (max err {err.max():.3e}, ratio {ratio.max():.1f})")
        if G.tol_half_applies(name, eps):
            bad = err > TOL / 2 + G.TRUNC
            if bad.any():
                self.fails.append(f"{variant} {name} eps={eps:g} d={d}: {int(bad.sum())} costs outside TOL / 2 + 2^-14 "
                                  f"(max err {err.max():.3e})")

    def check(self, cond, msg):
        if not cond:
            self.fails.append(msg)

    def finish(self, W):
        print()
        for (variant, name), (e, k) in self.rows.items():
            print(f"guided cost r={self.r} W={W} {variant:24s} {name:6s}: max err {e:.3e}  "
                  f"max (err - 2^-14)/(2^-24 M) {k:6.2f}  (C = {G.roundings(self.r)})")
        assert self.skipped <= 0, f"{self.skipped} pixels with |q64| >= 511 (clamped keys) were left out"
        assert not self.fails, f"{len(self.fails)} failing cases:\n" + "\n".join(self.fails[:40])


def _check_left(rep, variant, name, eps, d, keys, q, M, W):
    cost, dfield, empty = G.decode(keys)
    want_empty = np.broadcast_to(d > W - np.arange(W)[None, :], keys.shape)
    rep.check(np.array_equal(empty, want_empty), f"{variant} {name} eps={eps:g} d={d}: empty keys are not d > W - x")
    ok = ~empty & ~want_empty
    rep.check((dfield[ok] == d).all(), f"{variant} {name} eps={eps:g} d={d}: a d field is not d")
    rep.cost(variant, name, eps, d, cost[ok], q[ok], M[ok], ok)


def _check_right(rep, variant, name, eps, d, rkeys, q, M, W):
    cost, dfield, empty = G.decode(rkeys)
    n = max(W - d, 0)                                   # right pixels u with u + d < W
    want_empty = np.broadcast_to(np.arange(W)[None, :] >= n, rkeys.shape)
    rep.check(np.array_equal(empty, want_empty), f"{variant} {name} eps={eps:g} d={d}: empty keys are not u + d >= W")
    ok = ~empty & ~want_empty
    rep.check((dfield[ok] == d).all(), f"{variant} {name} eps={eps:g} d={d}: a d field is not d")
    # C_R(y, u, d) = q(y, u + d, d)
    qs, Ms = np.zeros_like(q), np.zeros_like(M)
    qs[:, :n], Ms[:, :n] = q[:, d:d + n], M[:, d:d + n]
    rep.cost(variant, name, eps, d, cost[ok], qs[ok], Ms[ok], ok)


def _cases(gray, oracle, W, H, ds):
    """(name, eps, L, R, the d that give a slice): d_lo > min(W, 255) has no valid pixel and no launch."""
    ds = [d for d in ds if d <= min(W, 255)]
    for name, (L, R) in _textures(gray, oracle, W, H).items():
        for eps in G.eps_values(name):
            yield name, eps, L, R, ds


@pytest.mark.parametrize("r,W,H,ds", SHAPES, ids=SHAPE_IDS)
def test_left_costs_left_only_kernel(matcher, oracle, gray, torch, r, W, H, ds):
    """guided_fused_kernel<R, false>: empty exactly where d > W - x, the d field d elsewhere, the cost within the
    bounds of the module docstring, at both image borders, the tile seam, the second tile row and the first d
    after a right-band restage (32, 64)."""
    rep = _Report(r)
    n_left_out = 0
    for name, eps, L, R, dd in _cases(gray, oracle, W, H, ds):
        n_left_out += len(ds) - len(dd)
        matcher.set_guided_eps(eps)
        Lt, Rt = torch.from_numpy(L).cuda(), torch.from_numpy(R).cuda()
        keys = torch.stack([matcher.guided_slice_keys_device(Lt, Rt, r, d, d + 1) for d in dd]).cpu().numpy()
        for d, k in zip(dd, keys):
            q, M = _reference(L, R, r, W, H, name, eps, d)
            _check_left(rep, "left-only", name, eps, d, k, q, M, W)
    assert n_left_out <= 0, f"{n_left_out} slices past min(W, 255) were left out"
    rep.finish(W)


@pytest.mark.parametrize("r,W,H,ds", SHAPES, ids=SHAPE_IDS)
def test_left_and_right_costs_fused_kernel(matcher, oracle, gray, torch, r, W, H, ds):
    """guided_fused_kernel<R, true> at every radius, so every right-view build: its left keys as above; its right
    key of u is empty exactly where u + d >= W and carries d and C_R(u, d) = q(u + d, d) elsewhere."""
    rep = _Report(r)
    n_left_out = 0
    vl, vr = f"fused left ({LR_VARIANT[r]})", f"fused right ({LR_VARIANT[r]})"
    for name, eps, L, R, dd in _cases(gray, oracle, W, H, ds):
        n_left_out += len(ds) - len(dd)
        matcher.set_guided_eps(eps)
        Lt, Rt = torch.from_numpy(L).cuda(), torch.from_numpy(R).cuda()
        parts = [matcher.slice_keys_lr_device(Lt, Rt, r, d, d + 1, agg="guided") for d in dd]
        lk = torch.stack([p[0] for p in parts]).cpu().numpy()
        rk = torch.stack([p[1] for p in parts]).cpu().numpy()
        for d, kl, kr in zip(dd, lk, rk):
            q, M = _reference(L, R, r, W, H, name, eps, d)
            _check_left(rep, vl, name, eps, d, kl, q, M, W)
            _check_right(rep, vr, name, eps, d, kr, q, M, W)
    assert n_left_out <= 0, f"{n_left_out} slices past min(W, 255) were left out"
    rep.finish(W)


def _slice_is_min_of_singles(full, singles, what):
    """Integer rule, no tolerance: the slice's cost field is the smallest single-d cost field, and its d field is
    a d that attains it (INT32_MAX: no valid d, field 2^23 - 1, above every real field)."""
    ffield, fd = full.astype(np.int64) >> 8, full.astype(np.int64) & 0xFF
    sfield = singles.astype(np.int64) >> 8
    empty = singles == G.INT32_MAX
    assert (((singles & 0xFF) == np.arange(len(singles))[:, None, None]) | empty).all(), what
    sfield[empty] = 1 << 24
    assert not (full == G.INT32_MAX).any(), what            # d = 0 is valid everywhere
    best = sfield.min(axis=0)
    assert np.array_equal(ffield, best), f"{what}: {int((ffield != best).sum())} cost fields are not the minimum"
    assert (fd < len(singles)).all(), what
    at = np.take_along_axis(sfield, fd[None], axis=0)[0]
    assert np.array_equal(at, best), f"{what}: {int((at != best).sum())} d fields do not attain the minimum"


@pytest.mark.parametrize("r", [2, 5])
def test_slice_equals_its_disparities(matcher, oracle, gray, torch, r):
    """q(d) is the same float alone or pipelined behind d - 1 and across two right-band restages (D = 70), so
    the truncated fields agree exactly: left-only kernel, and both views of the fused one."""
    D, H = 70, 41
    W = 2 * (64 - 4 * r) + 5
    matcher.set_guided_eps(G.EPS_DEFAULT)
    for name in ("art", "synth"):
        L, R = _textures(gray, oracle, W, H)[name]
        Lt, Rt = torch.from_numpy(L).cuda(), torch.from_numpy(R).cuda()
        full = matcher.guided_slice_keys_device(Lt, Rt, r, 0, D).cpu().numpy()
        singles = torch.stack([matcher.guided_slice_keys_device(Lt, Rt, r, d, d + 1) for d in range(D)]).cpu().numpy()
        _slice_is_min_of_singles(full, singles, f"left-only r={r} {name}")
        fl, fr = (t.cpu().numpy() for t in matcher.slice_keys_lr_device(Lt, Rt, r, 0, D, agg="guided"))
        parts = [matcher.slice_keys_lr_device(Lt, Rt, r, d, d + 1, agg="guided") for d in range(D)]
        sl = torch.stack([p[0] for p in parts]).cpu().numpy()
        sr = torch.stack([p[1] for p in parts]).cpu().numpy()
        assert np.array_equal(sl, singles), f"fused left r={r} {name}: single-d keys differ from the left-only kernel's"
        _slice_is_min_of_singles(fl, sl, f"fused left r={r} {name}")
        _slice_is_min_of_singles(fr, sr, f"fused right r={r} {name}")


@pytest.mark.parametrize("r", [6, 7])
def test_map_where_sip_passes_2_23(matcher, oracle, gray, r):
    """The disparity map where the window's sum of I p needs 24 bits (r >= 6, bright guide, large costs): with
    that sum read as a signed 24-bit operand the costs came out near -512 and won the WTA.  With
    |q_gpu(d) - q64(d)| <= e(d) = C 2^-24 M(d), the kernel's choice g satisfies q64(g) - e(g) <= q64(d) + e(d) for
    every valid d and q64(g) - e(g) < 50; it may report no match only if no valid d has q64 + e < 50."""
    W, H, D = 2 * (64 - 4 * r) + 5, 41, 32
    matcher.set_guided_eps(G.EPS_DEFAULT)
    xs = np.arange(W)[None, None, :]
    for name in ("bright", "step"):
        L, R = _textures(gray, oracle, W, H)[name]
        assert int(G.window_sums(L, R, r, 0)[4].max()) >= 1 << 23
        got = matcher.match(L, R, r, D, agg="guided").astype(np.int64)
        qe = [_reference(L, R, r, W, H, name, G.EPS_DEFAULT, d) for d in range(D)]
        q = np.stack([x[0] for x in qe])
        e = np.stack([x[1] for x in qe]) * (G.roundings(r) * G.U32)
        valid = np.arange(D)[:, None, None] <= W - xs
        lo, hi = np.where(valid, q - e, np.inf), np.where(valid, q + e, np.inf)
        assert (got < D).all()
        lo_g = np.take_along_axis(lo, got[None], axis=0)[0]
        ok = (lo_g <= hi.min(axis=0)) & (lo_g < 50.0)
        ok |= (got == 0) & (hi.min(axis=0) >= 50.0)
        assert ok.all(), f"{name}: {int((~ok).sum())} of {ok.size} disparities the fp64 costs cannot explain"
        if name == "bright":               # past the p = 0 zone of x < d every cost is near 250: no match
            assert (got[:, D - 1 + 2 * r:] == 0).all()


def test_keys_to_disp_threshold_edge(matcher, torch):
    """q < 50 is strict: field 819199 keeps its d, 819200 gives 0; negative costs keep theirs; the clamp's
    ends and INT32_MAX; a second block (x >= 256) and its ragged tail."""
    fields = [819199, 819200, 0, -1, -(1 << 23), (1 << 23) - 1]
    ds = [0, 1, 100, 254, 255]
    combos = [((f << 8) | d, d if f < 819200 else 0) for f in fields for d in ds] + [(G.INT32_MAX, 0)]
    W, H = 257, len(combos)
    idx = (np.arange(W)[None, :] + np.arange(H)[:, None]) % len(combos)   # every combo reaches column 256
    keys = np.array([c[0] for c in combos], np.int64)[idx].astype(np.int32)
    want = np.array([c[1] for c in combos], np.uint8)[idx]
    assert len(np.unique(idx[:, 256])) == len(combos) and keys.min() == -(1 << 31) and keys.max() == G.INT32_MAX
    got = matcher.guided_keys_to_disp_device(torch.from_numpy(keys).cuda()).cpu().numpy()
    assert np.array_equal(got, want), f"{int((got != want).sum())} pixels differ"
