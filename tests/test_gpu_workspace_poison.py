"""No call may depend on what it finds in the handle's workspaces (SM_PARAM_WORKSPACE_POISON).

Every matching, volume, post-filter and helper call of the C API works through five grow-only device buffers the
handle shares between all paths (`lr`, `rpart`, `vol`, `spk`, `boxq`, csrc/sm_handle.h), and the host calls stage
their frames in `d_left` / `d_right` / `d_disp`.  With the switch on, WsScope::get fills each buffer a call takes
(capacity and slack) and upload_pair the frame buffers with one byte before the call's first kernel.  Each row below
is one small call per user of a workspace, at the smallest shape at which its path still has partial tiles, run under
0x00 (beats every MIN, equals a fresh allocation), 0xFF (breaks every sum and every "empty = 0") and 0x5A (neither).

A row asserts that its outputs equal the reference the call's own test file uses, bit for bit (the float guided rows:
guided_check's tie-aware rules, as tests/test_gpu_guided.py), and equal, bit for bit, the same call on a fresh handle
that was never poisoned.  Rows that go through plan_box_pass also assert, through tests/native/box_plan_shim.cpp, that
the plan takes the branch the row is there for.

Every `ws.get(` site of csrc/ and the rows that reach it (a site missing here has no row):

    sm_capi.hip      run_box_pass   rpart  fused right-view partials   tile-lr-r2, tile-lr-r8, median-lr-r5,
                                                                       dslice-box-lr
    sm_capi.hip      run_box_pass   vol    strip right keys / V planes strip-lr-r16, strip-lr-r20 (+ -median),
                                                                       slice-keys-lr-r16, wide-match-r40, wide-lr-r40
    sm_capi.hip      run_box_pass   boxq   the queue's grab counter    matrix-queue
    sm_capi.hip      run_staged     vol    AD / SAD volumes, raw map   staged-b3-g2, staged-b3-g2-median
    sm_capi.hip      run_device_body vol   literal scratch             device-cu
    sm_capi.hip      run_device_body lr    median / right / mirror     median-lr-r5, strip-lr-r16-median, mirrored-lr,
                                                                       guided-lr-r5, sgm-ad-4-lr ...
    sm_capi.hip      run_device_body rpart guided right partials       guided-lr-r5
    sm_capi_volume   run_volume     vol    cost volumes, S, keys       sgm-*, box-census*, subpix-*, in-view-min-disp
    sm_capi_volume   run_volume     lr     SubpixMedianWs              subpix-* (median 1), subpix-device-b2-median,
                                                                       in-view-min-disp
    sm_capi_volume   volume_wta_subpix_device lr (median)              wta-subpix-median
    sm_capi_volume   volume_wta_subpix_device lr (d0 planes)           wta-subpix
    sm_capi_aux      reproject_u16  vol                                reproject
    sm_capi_aux      ad_volume_u8   vol                                ad-volume
    sm_capi_aux      census_volume_device vol                          census-volume-device
    sm_capi_aux      census_volume_u8 vol                              census-volume
    sm_capi_aux      sad_volume_device vol                             sad-volume-device
    sm_capi_aux      run_all_sad    vol    r <= 7: AD + SAD volumes    all-sad-r2, all-sad-device-r2
    sm_capi_aux      run_all_sad    vol    direct kernel, host out     all-sad-r9
    sm_capi_slice    slice_keys_pass rpart guided right partials       guided-slice-keys-lr, dslice-guided-lr
    sm_capi_speckle  run_speckle    spk    labels and counts           speckle-device-u8, speckle-device-u16,
                                                                       match-speckle-fill
    sm_capi_group    dslice_member_upload vol / rpart / rpart(guided)  test_group_dslice_members (wide-lr, box-lr,
                                                                       guided-lr; RCCL, one member)
    upload_pair      d_left / d_right / d_disp                         every host row; frames-320x64-then-37x11

The rows without a workspace of their own (census, census-device, all-sad-device-r9, guided-slice-keys, dslice-box,
dslice-guided) are the calls the same entry points serve beside them."""
import ctypes
import functools
import os
import shutil
import subprocess

import numpy as np
import pytest

import census_ref
import fill_ref
import median16_ref
import pairs_ref
import sgm_paths_ref
import sgm_ref
import speckle_ref
import subpix_ref
from conftest import GOLDEN
from guided_check import (TOL, check_guided_lr, guided_reference, tie_aware_check, tie_aware_lr_check)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = 1e-4 * 255 * 255
POISONS = [0x00, 0xFF, 0x5A]
# the handle: the widest row is the wide path's 333 columns, the tallest the literal grid's 256 rows
CAP = (333, 256, 64)

NONE, MAP, KEYS = 0, 1, 2                           # RightWant
TILE, STRIP, WIDE, DIRECT = 0, 1, 2, 3              # BoxLeft
R_NONE, FUSED, MIRRORED = 0, 1, 2                   # BoxRight


@pytest.fixture(scope="module")
def sm_mod():
    import gpu_stereo_matching_amd as sm
    return sm


def _new_handle(sm_mod):
    m = sm_mod.BlockMatcher(0, *CAP)
    m.set_guided_eps(EPS)
    return m


@pytest.fixture(scope="module")
def matcher(sm_mod):
    m = _new_handle(sm_mod)
    yield m
    m.close()


@pytest.fixture(scope="module")
def shims(tmp_path_factory):
    """plan_box_pass and box_queue_candidate of csrc/bm_box_plan.h, built with the host compiler alone."""
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "a host C++ compiler builds tests/native/box_plan_shim.cpp"
    d = tmp_path_factory.mktemp("poison_plan")
    libs = []
    for name in ("box_plan_shim", "box_queue_shim"):
        out = str(d / f"lib{name}.so")
        subprocess.run([cxx, "-O2", "-std=c++17", "-shared", "-fPIC", "-o", out,
                        os.path.join(ROOT, "tests", "native", name + ".cpp")], check=True)
        libs.append(ctypes.CDLL(out))
    plan_lib, queue_lib = libs
    plan_lib.box_plan.argtypes = [ctypes.c_int] * 8 + [ctypes.POINTER(ctypes.c_ulonglong)]
    plan_lib.box_plan.restype = None
    queue_lib.box_queue_candidate.argtypes = [ctypes.c_int] * 11

    def plan(W, H, pitch, radius, d_lo, d_hi, batch, want):
        o = (ctypes.c_ulonglong * 5)()
        plan_lib.box_plan(W, H, pitch, radius, d_lo, d_hi, batch, want, o)
        return dict(left=o[0], right=o[1], rpart=o[2], vol=o[3], mirror=o[4])

    return plan, queue_lib.box_queue_candidate


# ---- inputs and references, computed once and shared by the patterns ----
def _oracle():
    from oracle import oracle as O
    O.build()
    return O


@functools.lru_cache(maxsize=None)
def _pair(W, H, D, seed=0, flip=False):
    """oracle.synth_pair with +-4 noise on the right image, as test_gpu_subpix._pair; flip: upside down."""
    O = _oracle()
    seed = seed or (W * 131 + H * 17 + D)
    L, R = O.synth_pair(seed, W, H, D)
    R = np.clip(R.astype(np.int64) + np.random.default_rng(seed).integers(-4, 5, R.shape), 0, 255).astype(np.uint8)
    if flip:
        L, R = L[::-1].copy(), R[::-1].copy()
    L.setflags(write=False)
    R.setflags(write=False)
    return L, R


@functools.lru_cache(maxsize=None)
def _clean_pair(W, H, D, seed):
    L, R = _oracle().synth_pair(seed, W, H, max(D, 16))
    L.setflags(write=False)
    R.setflags(write=False)
    return L, R


def _t(a):
    import torch
    a = np.array(a)   # a writable copy
    if a.dtype == np.uint16:
        a = a.view(np.int16)
    return torch.from_numpy(a).cuda()


def _h(t, dtype=None):
    import torch
    torch.cuda.synchronize()
    a = t.cpu().numpy()
    return a.view(dtype) if dtype is not None else a


def _same(got, want, what):
    got = got if isinstance(got, tuple) else (got,)
    want = want if isinstance(want, tuple) else (want,)
    assert len(got) == len(want), what
    for i, (g, w) in enumerate(zip(got, want)):
        g, w = np.asarray(g), np.asarray(w)
        assert g.shape == w.shape, f"{what}: output {i} is {g.shape}, want {w.shape}"
        assert np.array_equal(g, w), f"{what}: output {i}, {int((g != w).sum())} of {g.size} elements differ"


class Row:
    """name; run(m) -> a tuple of host arrays; check(O, got): the reference's assertions; plan(shims): the box plan's
    branch (optional)."""

    def __init__(self, name, build, plan=None):
        self.name, self.plan, self._build, self._built = name, plan, build, None

    def _get(self, i):   # inputs are made at the row's first use, not when the module is imported
        if self._built is None:
            self._built = self._build()
        return self._built[i]

    def run(self, m):
        return self._get(0)(m)

    def check(self, O, got):
        return self._get(1)(O, got)

    def __repr__(self):
        return self.name


ROWS = []


def _row(name, plan=None):
    def deco(build):
        ROWS.append(Row(name, build, plan))
        return build
    return deco


def _plan_is(args, left, right, rpart=False, vol=False, mirror=0):
    def check(shims):
        p = shims[0](*args)
        assert (p["left"], p["right"], p["mirror"]) == (left, right, mirror), (args, p)
        assert (p["rpart"] > 0) == rpart and (p["vol"] > 0) == vol, (args, p)
    return check


# ---- box rows ----
def _box_lr_row(W, H, r, D, seed=0):
    if W < 16:   # narrower than synth_pair's shifts: random frames, as tests/test_gpu_literal.py
        rng = np.random.default_rng(seed)
        L, R = (rng.integers(0, 256, (H, W), dtype=np.uint8) for _ in range(2))
    else:
        L, R = _pair(W, H, max(D, 16), seed)

    def run(m):
        return m.match_lr(L, R, r, D)

    def check(O, got):
        _, rd, chk, mask = O.box_lr(L, R, r, D)
        _same(got, (chk, rd, mask), f"match_lr {W}x{H} r={r} D={D}")
    return run, check


def _box_lr_median_row(W, H, r, D):
    L, R = _pair(W, H, max(D, 16))

    def run(m):
        return m.match_lr(L, R, r, D, median=True)

    def check(O, got):
        d, cost = O.box_disp(L, R, r, D, want_cost=True)
        chk, mask = O.lr_check(O.median(d, 3), O.median(O.right_wta(cost), 3))
        _same((got[0], got[2]), (chk, mask), f"match_lr median {W}x{H} r={r} D={D}")
    return run, check


# tiles are 64 - 2r columns by 32 rows: both edges partial; r = 8 runs the u32 window halves
for _r in (2, 8):
    _row(f"tile-lr-r{_r}", _plan_is((97, 41, 97, _r, 0, 32, 1, MAP), TILE, FUSED, rpart=True))(
        functools.partial(_box_lr_row, 97, 41, _r, 32))
_row("median-lr-r5", _plan_is((97, 41, 97, 5, 0, 32, 1, MAP), TILE, FUSED, rpart=True))(
    functools.partial(_box_lr_median_row, 97, 41, 5, 32))
# the strip pass's right keys in `vol` (reduced with an atomic MIN over the 0xFF fill of run_box_pass)
for _r in (16, 20):
    _row(f"strip-lr-r{_r}", _plan_is((120, 60, 120, _r, 0, 24, 1, MAP), STRIP, FUSED, vol=True))(
        functools.partial(_box_lr_row, 120, 60, _r, 24))
    _row(f"strip-lr-r{_r}-median", _plan_is((120, 60, 120, _r, 0, 24, 1, MAP), STRIP, FUSED, vol=True))(
        functools.partial(_box_lr_median_row, 120, 60, _r, 24))
# the mirrored pair's planes in `lr`: a frame neither the strip kernel nor the wide path takes
_row("mirrored-lr", _plan_is((3, 5, 3, 16, 0, 4, 1, MAP), DIRECT, MIRRORED, mirror=2))(
    functools.partial(_box_lr_row, 3, 5, 16, 4, 77))
_row("wide-lr-r40", _plan_is((333, 150, 333, 40, 0, 16, 1, MAP), WIDE, FUSED, vol=True))(
    functools.partial(_box_lr_row, 333, 150, 40, 16))


@_row("wide-match-r40", _plan_is((333, 150, 333, 40, 0, 16, 1, NONE), WIDE, R_NONE, vol=True))
def _wide_match():
    L, R = _pair(333, 150, 16)
    return (lambda m: (m.match(L, R, 40, 16),)), \
        (lambda O, got: _same(got, O.box_disp(L, R, 40, 16), "match r=40"))


@_row("slice-keys-lr-r16", _plan_is((120, 60, 120, 16, 3, 24, 1, KEYS), WIDE, FUSED, vol=True))
def _slice_keys_lr():
    L, R = _pair(120, 60, 24)

    def run(m):
        lk, rk = m.slice_keys_lr_device(_t(L), _t(R), 16, 3, 24)
        return _h(lk, np.uint32), _h(rk, np.uint32)

    def check(O, got):
        _same(got, (O.box_keys_slice(L, R, 16, 3, 24), O.box_right_keys_slice(L, R, 16, 3, 24)), "slice keys r=16")
    return run, check


def _queue_plan(shims):
    _plan_is((130, 70, 130, 3, 0, 32, 1, NONE), TILE, R_NONE)(shims)
    # box kernel 2 (matrix), workgroups 0, queue workgroups 3, on any device size: the launch takes the counter
    for cus in (1, 256, 304):
        assert shims[1](130, 70, 3, 0, 32, 1, 0, cus, 2, 0, 3) == 1


@_row("matrix-queue", _queue_plan)
def _matrix_queue():
    L, R = _pair(130, 70, 32)

    def run(m):
        m.set_box_kernel(2)
        m.set_box_queue_workgroups(3)
        try:
            Lt, Rt = _t(L), _t(R)
            a = m.match_device(Lt, Rt, 3, 32)
            b = m.match_device(Lt, Rt, 3, 32)     # twice in a row: the counter the first launch left
            return _h(a), _h(b)
        finally:
            m.set_box_kernel(0)
            m.set_box_queue_workgroups(0)

    def check(O, got):
        want = O.box_disp(L, R, 3, 32)
        _same(got, (want, want), "matrix kernel with the queue")
    return run, check


def _staged_row(median):
    pairs = [_pair(97, 41, 32, seed=600 + b) for b in range(3)]

    def run(m):
        from gpu_stereo_matching_amd import _capi
        _capi.check(m._lib.sm_set_param_f(m._h, _capi.SM_PARAM_STAGED_GROUP, 2.0))
        try:
            Lt, Rt = _t(np.stack([p[0] for p in pairs])), _t(np.stack([p[1] for p in pairs]))
            return (_h(m.match_device(Lt, Rt, 3, 32, agg="box-staged", median=median)),)
        finally:
            _capi.check(m._lib.sm_set_param_f(m._h, _capi.SM_PARAM_STAGED_GROUP, 8.0))

    def check(O, got):
        want = [O.box_disp(L, R, 3, 32) for L, R in pairs]
        if median:
            want = [O.median(w, 3) for w in want]
        _same(got, np.stack(want), "box-staged, 3 frames in groups of 2")
    return run, check


_row("staged-b3-g2")(functools.partial(_staged_row, False))
_row("staged-b3-g2-median")(functools.partial(_staged_row, True))


@_row("device-cu")
def _device_cu():
    L, R = _pair(320, 256, 16)
    return (lambda m: (m.match(L, R, 3, 16, agg="device-cu"),)), \
        (lambda O, got: _same(got, O.device_cu_literal_integral(L, R, 3, 16), "device-cu"))


# ---- guided rows (float: guided_check's rules, and bit equality with the fresh handle) ----
class _Replay:
    """What check_guided_lr asks of a matcher, answered with maps already computed."""

    def __init__(self, left, lr):
        self.left, self.lr = left, lr

    def match(self, *a, **k):
        return self.left

    def match_lr(self, *a, **k):
        return self.lr


GW, GH, GD, GR = 97, 40, 32, 5


@_row("guided-lr-r5")
def _guided_lr():
    L, R = _clean_pair(GW, GH, GD, GW * 3 + GH)

    def run(m):
        return (m.match(L, R, GR, GD, agg="guided"),) + tuple(m.match_lr(L, R, GR, GD, agg="guided"))

    def check(O, got):
        check_guided_lr(_Replay(got[0], got[1:]), O, L, R, GR, GD, EPS)
    return run, check


def _slice_contract(parts, cuts, W):
    xs = np.arange(W)[None, :]
    for (a, b), pk in zip(zip(cuts, cuts[1:]), parts):
        empty = pk == 0x7FFFFFFF
        d = pk & 0xFF
        assert ((d >= a) & (d < b) & (d <= W - xs))[~empty].all(), (a, b)
        assert (empty == (a > W - xs)).all(), (a, b)


@_row("guided-slice-keys")
def _guided_slice_keys():
    L, R = _clean_pair(GW, GH, GD, GW * 7 + GH)
    cuts = (0, 12, 13, 32)

    def run(m):
        import torch
        Lt, Rt = _t(L), _t(R)
        parts = [m.guided_slice_keys_device(Lt, Rt, GR, a, b) for a, b in zip(cuts, cuts[1:])]
        k = parts[0].clone()
        for p in parts[1:]:
            k = torch.minimum(k, p)
        got = m.guided_keys_to_disp_device(k)
        return tuple(_h(p) for p in parts) + (_h(got),)

    def check(O, got):
        _slice_contract(got[:-1], cuts, GW)
        disp_o, q, best = O.guided_disp(L, R, GR, GD, EPS, want_q=True)
        ok, _ = tie_aware_check(got[-1], q, {"disp": disp_o, "best": best}, GD, GW)
        assert ok.all(), f"{int((~ok).sum())} pixels outside the tie-aware tolerance"
    return run, check


@_row("guided-slice-keys-lr")
def _guided_slice_keys_lr():
    L, R = _clean_pair(GW, GH, GD, GW * 7 + GH)
    cuts = (0, 12, 32)

    def run(m):
        import torch
        Lt, Rt = _t(L), _t(R)
        parts = [m.slice_keys_lr_device(Lt, Rt, GR, a, b, agg="guided") for a, b in zip(cuts, cuts[1:])]
        lk, rk = parts[0][0].clone(), parts[0][1].clone()
        for a, b in parts[1:]:
            lk, rk = torch.minimum(lk, a), torch.minimum(rk, b)
        left, right = m.guided_keys_to_disp_device(lk), m.right_keys_to_disp_device(rk)
        chk = m.lr_check_device(left, right)
        return tuple(_h(k) for p in parts for k in p) + (_h(left), _h(right), _h(chk))

    def check(O, got):
        left, right, chk = got[-3:]
        ref = guided_reference(O, L, R, GR, GD, EPS)
        ok, _ = tie_aware_check(left, ref["q"], ref, GD, GW)
        assert ok.all(), f"left: {int((~ok).sum())} pixels outside the tie-aware tolerance"
        ys, us = np.mgrid[0:GH, 0:GW]
        assert (right < GD).all()
        ok_r = (right == ref["rdisp"]) | (ref["cr"][right.astype(np.int64), ys, us] <= ref["best_r"] + TOL)
        assert ok_r.all(), f"right: {int((~ok_r).sum())} pixels outside the tie-aware tolerance"
        assert np.array_equal(chk, O.lr_check(left, right)[0])
        assert tie_aware_lr_check(chk, ref, GD, GW).all()
    return run, check


# ---- the passes that keep a cost volume: 96 x 40, D = 32, r = 2 (test_gpu_median16.py's pair) ----
PW, PH, PD, PR = 96, 40, 32, 2
PATHS = [("box", "ad"), ("box", "census"), ("sgm", "ad"), ("sgm", "census")]


@functools.lru_cache(maxsize=None)
def _maps8(agg, cost, paths):
    """(left, right, checked, mask) of the 8-bit calls, by the reference of the call's own test file."""
    O = _oracle()
    L, R = _pair(PW, PH, PD)
    if cost == "census":
        return census_ref.census_lr(O, L, R, PR, PD, agg)
    if paths == 4:
        return sgm_ref.sgm_lr(O, L, R, PR, PD, *sgm_ref.auto_penalties(PR))
    return sgm_paths_ref.sgm_lr(O, L, R, PR, PD, *sgm_ref.auto_penalties(PR), paths=paths)


@functools.lru_cache(maxsize=None)
def _volume(agg, cost, flip=False):
    return subpix_ref.volume(_oracle(), *_pair(PW, PH, PD, flip=flip), PR, PD, agg, cost)


@functools.lru_cache(maxsize=None)
def _views(agg, cost, flip=False):
    """Both views' unchecked 1/16-px maps, and the LR-checked call's (q, right q, mask)."""
    V, inv, rp = _volume(agg, cost, flip)
    q, qr, _ = subpix_ref.subpix(V, 0, inv, False, rp)
    return q, qr, subpix_ref.subpix(V, 0, inv, True, rp)


def _volume8_row(agg, cost, paths, lr):
    L, R = _pair(PW, PH, PD)

    def run(m):
        m.set_sgm_paths(paths)
        try:
            return tuple(m.match_lr(L, R, PR, PD, agg=agg, cost=cost)) if lr else \
                (m.match(L, R, PR, PD, agg=agg, cost=cost),)
        finally:
            m.set_sgm_paths(4)

    def check(O, got):
        dl, dr, checked, mask = _maps8(agg, cost, paths)
        _same(got, (checked, dr, mask) if lr else (dl,), f"{agg}/{cost} {paths} paths lr={lr}")
    return run, check


def _subpix_row(agg, cost, lr):
    L, R = _pair(PW, PH, PD)

    def run(m):
        m.set_subpix_median(1)
        try:
            return m.match_subpix(L, R, PR, PD, agg=agg, cost=cost, lr_check=lr, return_right=True, return_mask=True)
        finally:
            m.set_subpix_median(0)

    def check(O, got):
        q, qr, _ = _views(agg, cost)
        _same(got, median16_ref.subpix_median(q, qr, 1, lr), f"match_subpix {agg}/{cost} median 1 lr={lr}")
    return run, check


for _agg, _cost, _paths in (("sgm", "ad", 4), ("sgm", "ad", 8), ("sgm", "census", 4), ("box", "census", 4)):
    for _lr in (False, True):
        _name = f"{_agg}-{_cost}" + (f"-{_paths}" if _agg == "sgm" and _cost == "ad" else "") + ("-lr" if _lr else "")
        _row(_name)(functools.partial(_volume8_row, _agg, _cost, _paths, _lr))
for _agg, _cost in PATHS:
    for _lr in (False, True):
        _row(f"subpix-{_agg}-{_cost}" + ("-lr" if _lr else ""))(functools.partial(_subpix_row, _agg, _cost, _lr))


def _subpix_device_row(median):
    def run(m):
        import torch
        Lt = _t(np.stack([_pair(PW, PH, PD)[0], _pair(PW, PH, PD, flip=True)[0]]))
        Rt = _t(np.stack([_pair(PW, PH, PD)[1], _pair(PW, PH, PD, flip=True)[1]]))
        rt = torch.empty((2, PH, PW), dtype=torch.int16, device="cuda")
        mt = torch.empty((2, PH, PW), dtype=torch.uint8, device="cuda")
        m.set_subpix_median(median)
        try:
            out = m.match_subpix_device(Lt, Rt, PR, PD, agg="sgm", cost="ad", lr_check=True, right_t16=rt, mask_t=mt)
            return _h(out, np.uint16), _h(rt, np.uint16), _h(mt)
        finally:
            m.set_subpix_median(0)

    def check(O, got):
        for b, flip in enumerate((False, True)):
            q, qr, checked = _views("sgm", "ad", flip)
            want = median16_ref.subpix_median(q, qr, median, True) if median else checked
            _same(tuple(g[b] for g in got), want, f"match_subpix_device frame {b} median {median}")
    return run, check


_row("subpix-device-b2")(functools.partial(_subpix_device_row, 0))
_row("subpix-device-b2-median")(functools.partial(_subpix_device_row, 1))


def _wta_row(median):
    def run(m):
        import torch
        V, inv, rp = _volume("sgm", "ad")
        assert inv == 0 and rp == 1
        vt = _t(np.where(subpix_ref.left_exists(*V.shape), V, 0).astype(np.int32))
        rt = torch.empty((PH, PW), dtype=torch.int16, device="cuda")
        mt = torch.empty((PH, PW), dtype=torch.uint8, device="cuda")
        m.set_subpix_median(median)
        try:
            qt = m.volume_wta_subpix_device(vt, 0, True, right_t16=rt, mask_t=mt)
            return _h(qt, np.uint16), _h(rt, np.uint16), _h(mt)
        finally:
            m.set_subpix_median(0)

    def check(O, got):
        q, qr, checked = _views("sgm", "ad")
        _same(got, median16_ref.subpix_median(q, qr, median, True) if median else checked,
              f"volume_wta_subpix_device median {median}")
    return run, check


_row("wta-subpix")(functools.partial(_wta_row, 0))
_row("wta-subpix-median")(functools.partial(_wta_row, 1))


@_row("in-view-min-disp")
def _in_view():
    """pairs='in-view', set_min_disp(20), median 2: the case of test_gpu_median16.py."""
    L, R = _pair(PW, PH, PD)

    def run(m):
        m.set_min_disp(20)
        m.set_subpix_median(2)
        try:
            return m.match_subpix(L, R, PR, PD, agg="sgm", cost="census", lr_check=True, return_right=True,
                                  return_mask=True, pairs="in-view")
        finally:
            m.set_subpix_median(0)
            m.set_min_disp(0)

    def check(O, got):
        q, qr, _ = _in_view_ref()
        want = median16_ref.subpix_median(q, qr, 2, True)
        assert want[2].any() and not want[2].all() and q.max() > 16 * 32
        _same(got, want, "in-view, minimum disparity 20")
    return run, check


@functools.lru_cache(maxsize=None)
def _in_view_ref():
    L, R = _pair(PW, PH, PD)
    return pairs_ref.Reference(L, R, PR, PD, "in-view", 20).subpix("sgm", "census", 0, False)


# ---- helper calls: 97 x 41, D = 32 ----
HW, HH, HD = 97, 41, 32


@_row("reproject")
def _reproject():
    from gpu_stereo_matching_amd import calib
    K1, K2, d1, d2, Rm, T = calib.load_data_batch(os.path.join(GOLDEN, "Calib_Data_OpenCV.yml"))
    Q = np.asarray(calib.stereo_rectify(K1, d1, K2, d2, (320, 200), Rm, T)[4], np.float64).reshape(4, 4)
    W, H = 300, 7
    rng = np.random.default_rng(4)
    q = rng.integers(1, 4089, (H, W)).astype(np.uint16)
    q[rng.random((H, W)) < 0.2] = 0
    xs, ys = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64))
    vec = np.stack([xs, ys, q.astype(np.float64) / 16.0, np.ones_like(xs)], axis=-1) @ Q.T
    want = np.where((q > 0)[..., None], vec[..., :3] / np.where(vec[..., 3:] == 0, 1.0, vec[..., 3:]), 0.0)

    def check(O, got):
        # the kernel evaluates in double and rounds once to fp32 (2^-24): rtol as tests/test_gpu_subpix.py
        assert got[0].dtype == np.float32 and got[0].shape == (H, W, 3)
        assert np.allclose(got[0], want, rtol=1e-5, atol=0.0) and not got[0][q == 0].any()
    return (lambda m: (m.reproject(q, Q),)), check


def _all_sad_row(r, device):
    L, R = _pair(HW, HH, HD)

    def run(m):
        return (_h(m.all_sad_device(_t(L), _t(R), r, HD)),) if device else (m.all_sad(L, R, r, HD),)
    return run, (lambda O, got: _same(got, O.get_all_sad(L, R, r, HD), f"all_sad r={r} device={device}"))


for _r in (2, 9):
    _row(f"all-sad-r{_r}")(functools.partial(_all_sad_row, _r, False))
    _row(f"all-sad-device-r{_r}")(functools.partial(_all_sad_row, _r, True))


@_row("sad-volume-device")
def _sad_volume():
    L, R = _pair(HW, HH, HD)
    return (lambda m: (_h(m.sad_volume_device(_t(L), _t(R), 4, HD), np.uint16).astype(np.int32),)), \
        (lambda O, got: _same(got, O.box_cost(L, R, 4, HD).astype(np.int32), "sad_volume_device"))


@_row("ad-volume")
def _ad_volume():
    L, R = _pair(HW, HH, HD)
    return (lambda m: (m.ad_volume(L, R, HD),)), (lambda O, got: _same(got, O.precal(L, R, HD), "ad_volume"))


@_row("census")
def _census():
    L, _ = _pair(HW, HH, HD)
    return (lambda m: (m.census(np.array(L)),)), (lambda O, got: _same(got, census_ref.census(L), "census"))


@_row("census-device")
def _census_device():
    L, _ = _pair(HW, HH, HD)
    return (lambda m: (_h(m.census_device(_t(L)), np.uint64),)), \
        (lambda O, got: _same(got, census_ref.census(L), "census_device"))


@_row("census-volume")
def _census_volume():
    L, R = _pair(HW, HH, HD)
    return (lambda m: (m.census_volume(L, R, HD),)), \
        (lambda O, got: _same(got, census_ref.hamming_volume(L, R, HD), "census_volume"))


@_row("census-volume-device")
def _census_volume_device():
    L, R = _pair(HW, HH, HD)
    return (lambda m: (_h(m.census_volume_device(_t(L), _t(R), HD)),)), \
        (lambda O, got: _same(got, census_ref.hamming_volume(L, R, HD), "census_volume_device"))


# ---- speckle and fill ----
def _speckle_tiles():
    import re
    txt = open(os.path.join(ROOT, "gpu_stereo_matching_amd", "csrc", "bm_speckle_plan.h")).read()
    return tuple(int(re.search(r"constexpr int %s = (\d+);" % n, txt).group(1)) for n in ("kSpeckleTileW", "kSpeckleTileH"))


def _speckle_row(dtype, max_diff):
    tw, th = _speckle_tiles()
    W, H = 2 * tw + 3, 2 * th + 1      # two tiles and a ragged third each way: every kind of seam
    assert W <= CAP[0] and H <= CAP[1]

    def quantised(seed):
        rng = np.random.default_rng(seed)
        v = rng.choice(np.array([0, 8, 9, 10, 11, 12]), size=(H, W))
        if dtype == np.uint16:
            v = np.where(v > 0, v * 16 + rng.integers(0, 16, (H, W)), 0)
        return v.astype(dtype)

    frames = np.stack([quantised(40 + b) for b in range(2)])
    masks = np.random.default_rng(9).integers(0, 2, frames.shape).astype(np.uint8)

    def run(m):
        t, mk = _t(frames), _t(masks)
        m.speckle_filter_device(t, 7, max_diff, mask=mk)
        return _h(t, dtype), _h(mk)

    def check(O, got):
        want = [speckle_ref.speckle(frames[b], 7, max_diff, masks[b]) for b in range(2)]
        assert any((w[0] != f).any() for w, f in zip(want, frames))
        _same(got, (np.stack([w[0] for w in want]), np.stack([w[1] for w in want])), f"speckle {np.dtype(dtype).name}")
    return run, check


_row("speckle-device-u8")(functools.partial(_speckle_row, np.uint8, 1))
_row("speckle-device-u16")(functools.partial(_speckle_row, np.uint16, 16))


@_row("match-speckle-fill")
def _match_speckle_fill():
    L, R = _pair(PW, PH, PD)

    def run(m):
        m.set_speckle(20, 1)
        m.set_fill(12)
        try:
            return (m.match(L, R, PR, PD),)
        finally:
            m.set_fill(0)
            m.set_speckle()

    def check(O, got):
        dl = O.box_disp(L, R, PR, PD)
        un = speckle_ref.speckle(dl, 20, 1, None)[0]
        want = fill_ref.fill(un, 12)
        assert (un != dl).any() and (want != un).any()
        _same(got, want, "match, speckle 20 / 1, fill 12")
    return run, check


# ---- the d-slice rehearsal, 3 members ----
DW, DH, DD, DR = 97, 31, 37, 4


def _dslice_row(agg, lr):
    L, R = _clean_pair(DW, DH, DD, 31)

    def run(m):
        return (m.dslice_rehearse(L, R, DR, DD, 3, agg=agg, lr_check=lr),)

    def check(O, got):
        if agg == "box":
            _same(got, O.box_lr(L, R, DR, DD)[2] if lr else O.box_disp(L, R, DR, DD), f"dslice box lr={lr}")
            return
        ref = guided_reference(O, L, R, DR, DD, EPS)
        ok = tie_aware_lr_check(got[0], ref, DD, DW) if lr else tie_aware_check(got[0], ref["q"], ref, DD, DW)[0]
        assert ok.all(), f"dslice guided lr={lr}: {int((~ok).sum())} pixels without a tie-aware justification"
    return run, check


for _agg in ("box", "guided"):
    for _lr in (False, True):
        _row(f"dslice-{_agg}" + ("-lr" if _lr else ""),
             _plan_is((DW, DH, DW, DR, 0, 12, 1, KEYS), TILE, FUSED, rpart=True) if (_agg, _lr) == ("box", True)
             else None)(functools.partial(_dslice_row, _agg, _lr))


# ---- the frame buffers: a frame of the handle's width, then a much smaller one in the same buffers ----
@_row("frames-320x64-then-37x11")
def _frames():
    big, small = _pair(320, 64, 32), _pair(37, 11, 16)

    def run(m):
        return (m.match(*big, 5, 32), m.match(*small, 2, 16)) + tuple(m.match_lr(*small, 2, 16))

    def check(O, got):
        _, rd, chk, mask = O.box_lr(*small, 2, 16)
        _same(got, (O.box_disp(*big, 5, 32), O.box_disp(*small, 2, 16), chk, rd, mask), "frame buffers")
    return run, check


# ---- the tests ----
_FRESH = {}


def _fresh(sm_mod, row):
    """The row on a handle of its own that was never poisoned, once."""
    if row.name not in _FRESH:
        m = _new_handle(sm_mod)
        try:
            _FRESH[row.name] = tuple(np.array(g) for g in row.run(m))
        finally:
            m.close()
    return _FRESH[row.name]


def _check_row(sm_mod, m, oracle, shims, row, poison):
    if row.plan:
        row.plan(shims)
    m.set_workspace_poison(poison)
    try:
        got = row.run(m)
    finally:
        m.set_workspace_poison(None)
    got = got if isinstance(got, tuple) else (got,)
    row.check(oracle, got)
    _same(got, _fresh(sm_mod, row), f"{row.name} under 0x{poison:02X} against a fresh unpoisoned handle")


def test_the_table_names_each_row_once():
    names = [r.name for r in ROWS]
    assert len(set(names)) == len(names)


@pytest.mark.parametrize("poison", POISONS, ids=lambda p: f"0x{p:02X}")
@pytest.mark.parametrize("row", ROWS, ids=repr)
def test_row(sm_mod, matcher, oracle, shims, row, poison):
    _check_row(sm_mod, matcher, oracle, shims, row, poison)


def test_whole_table_in_reverse_order_on_a_fresh_handle(sm_mod, oracle, shims):
    """Every buffer is first allocated small, grows, and is then reused oversized, under 0xFF."""
    m = _new_handle(sm_mod)
    try:
        for row in reversed(ROWS):
            _check_row(sm_mod, m, oracle, shims, row, 0xFF)
    finally:
        m.close()


def test_parameter(sm_mod, matcher, oracle, shims):
    """-1, 257 and 1.5 are refused and leave the state in force (the error text names it); 0 restores the default."""
    from gpu_stereo_matching_amd import _capi
    lib, h = matcher._lib, matcher._h
    set_raw = lambda v: lib.sm_set_param_f(h, _capi.SM_PARAM_WORKSPACE_POISON, float(v))   # noqa: E731
    row = next(r for r in ROWS if r.name == "sgm-ad-4-lr")
    try:
        for state in (0, 0x5A + 1, 256, 1):
            assert set_raw(state) == _capi.SM_OK
            for bad in (-1, 257, 1.5):
                assert set_raw(bad) == _capi.SM_ERR_INVALID_ARG
                msg = lib.sm_last_error_string().decode()
                assert "SM_PARAM_WORKSPACE_POISON" in msg and msg.endswith(f"it stays {state}"), msg
            got = row.run(matcher)
            row.check(oracle, got)
            _same(got, _fresh(sm_mod, row), f"state {state}")
        for bad in (-1, 256, 0.5, float("nan")):
            with pytest.raises(sm_mod.SMError, match="SM_PARAM_WORKSPACE_POISON") as e:
                matcher.set_workspace_poison(bad)
            assert e.value.code == _capi.SM_ERR_INVALID_ARG
        matcher.set_workspace_poison(255)
        assert set_raw(1000) == _capi.SM_ERR_INVALID_ARG and lib.sm_last_error_string().decode().endswith("it stays 256")
        matcher.set_workspace_poison(None)
        assert set_raw(-5) == _capi.SM_ERR_INVALID_ARG and lib.sm_last_error_string().decode().endswith("it stays 0")
    finally:
        assert set_raw(0) == _capi.SM_OK


# ---- the group's d-slice members (sm_capi_group.hip), through RCCL with one member on the one GPU ----
GROUP_ROWS = [("wide-lr", 120, 60, 40, 16, "box"), ("box-lr", DW, DH, DR, DD, "box"), ("guided-lr", DW, DH, 3, 32, "guided")]


def _group_run(g, poison):
    from gpu_stereo_matching_amd import _capi
    _capi.check(g._lib.sm_group_set_param_f(g._g, _capi.SM_PARAM_WORKSPACE_POISON, 0.0 if poison is None else poison + 1.0))
    try:
        return [g.match_dslice(*_clean_pair(W, H, D, 5), r, D, agg=agg, lr_check=True)
                for _, W, H, r, D, agg in GROUP_ROWS]
    finally:
        _capi.check(g._lib.sm_group_set_param_f(g._g, _capi.SM_PARAM_WORKSPACE_POISON, 0.0))


@pytest.fixture(scope="module")
def group_fresh(sm_mod):
    with sm_mod.BlockMatcherGroup([0], 128, 64, 64) as g:
        g.set_guided_eps(EPS)
        return _group_run(g, None)


def test_group_dslice_members(sm_mod, oracle, shims, group_fresh):
    """Phase 1 sizes the member's workspaces in a scope of its own, phase 2 takes them again: vol (the wide path's
    planes), rpart (the fused right view's partials) and rpart (guided), each with the LR check."""
    _plan_is((120, 60, 120, 40, 0, 16, 1, KEYS), WIDE, FUSED, vol=True)(shims)
    _plan_is((DW, DH, DW, DR, 0, DD, 1, KEYS), TILE, FUSED, rpart=True)(shims)
    with sm_mod.BlockMatcherGroup([0], 128, 64, 64) as g:
        g.set_guided_eps(EPS)
        for poison in POISONS:
            got = _group_run(g, poison)
            for (name, W, H, r, D, agg), out, fresh in zip(GROUP_ROWS, got, group_fresh):
                L, R = _clean_pair(W, H, D, 5)
                if agg == "box":
                    _same(out, oracle.box_lr(L, R, r, D)[2], f"group {name} under 0x{poison:02X}")
                else:
                    ok = tie_aware_lr_check(out, guided_reference(oracle, L, R, r, D, EPS), D, W)
                    assert ok.all(), f"group {name}: {int((~ok).sum())} pixels without a tie-aware justification"
                _same(out, fresh, f"group {name} under 0x{poison:02X} against the unpoisoned group")
