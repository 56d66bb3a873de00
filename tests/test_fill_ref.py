"""CPU tests of the row fill (SM_PARAM_FILL_GAP, sm_fill_invalid_*): the numpy reference against the literal loop
of the definition, the rule's own properties, the quality it buys on two Middlebury pairs, and the host-only parts
of the C ABI."""
import ctypes
import os

import numpy as np
import pytest

import census_ref
import fill_ref
import sgm_ref
import speckle_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
FILL_ALL = 1 << 24      # the largest max_gap: every run of any frame


def _random_map(seed, dtype, share):
    """A seeded map up to 37 x 9 with about `share` of its pixels invalid, in clumps and singly."""
    rng = np.random.default_rng(seed)
    H, W = int(rng.integers(1, 10)), int(rng.integers(1, 38))
    top = 255 if dtype == np.uint8 else 65535
    v = rng.integers(1, top + 1, (H, W))
    holes = rng.random((H, W)) < share / 2
    holes |= np.roll(holes, 1, axis=1) & (rng.random((H, W)) < 0.8)      # runs, some wrapped to column 0
    return np.where(holes, 0, v).astype(dtype)


@pytest.mark.parametrize("seed", range(24))
def test_reference_equals_literal_loop(seed):
    dtype = np.uint16 if seed % 2 else np.uint8
    img = _random_map(seed, dtype, (0.05, 0.3, 0.95)[seed % 3])
    W = img.shape[1]
    for gap in (1, 2, W - 1, W, FILL_ALL):
        got, want = fill_ref.fill(img, gap), fill_ref.fill_literal(img, gap)
        assert got.dtype == img.dtype and np.array_equal(got, want), (seed, gap)
        assert np.array_equal(got[img != 0], img[img != 0])               # valid pixels never change
    assert np.array_equal(fill_ref.fill(img, 0), img)
    full = fill_ref.fill(img, W)
    assert np.array_equal(full, fill_ref.fill(img, FILL_ALL))              # any gap >= W fills every run
    rows_with_a_pixel = (img != 0).any(axis=1)
    assert full[rows_with_a_pixel].all() and not full[~rows_with_a_pixel].any()


def test_the_rule_by_hand():
    a = np.array([[0, 0, 5, 0, 3, 0, 0, 0, 9, 0]], np.uint8)
    assert fill_ref.fill(a, 1).tolist() == [[0, 0, 5, 3, 3, 0, 0, 0, 9, 9]]
    assert fill_ref.fill(a, 2).tolist() == [[5, 5, 5, 3, 3, 0, 0, 0, 9, 9]]
    assert fill_ref.fill(a, 3).tolist() == [[5, 5, 5, 3, 3, 3, 3, 3, 9, 9]]
    # the whole element decides, not its low byte
    b = np.array([[0x00FF, 0, 0x0100, 0, 0xFFFF, 0, 0x0001]], np.uint16)
    assert fill_ref.fill(b, 1).tolist() == [[0x00FF, 0x00FF, 0x0100, 0x0100, 0xFFFF, 0x0001, 0x0001]]
    # only the first / only the last pixel valid; no pixel valid
    c = np.zeros((3, 6), np.uint8)
    c[0, 0], c[1, 5] = 7, 8
    assert fill_ref.fill(c, 5).tolist() == [[7] * 6, [8] * 6, [0] * 6]
    assert np.array_equal(fill_ref.fill(c, 4), c)


def test_idempotent_and_order_free():
    for seed in range(6):
        img = _random_map(seed, np.uint8, 0.3)
        once = fill_ref.fill(img, 3)
        # what a second pass fills are the longer runs, from the same neighbours: filling in two passes of the
        # same gap changes nothing more, because a filled run's neighbours were valid before
        assert np.array_equal(fill_ref.fill(once, 3), once)
        assert np.array_equal(fill_ref.fill(img[:, ::-1], 3)[:, ::-1], once)   # left and right are symmetric


@pytest.fixture(scope="module")
def pipeline(oracle, gray):
    """(name, cost) -> (raw SGM map, LR-checked map, + speckle(200, 1)) of the reference pipeline at r = 2, D = 80,
    auto penalties; computed once for the module."""
    out = {}
    for name in ("Books", "Art"):
        L, R = gray[name + "/view1"], gray[name + "/view5"]
        for cost in ("ad", "census"):
            if cost == "ad":
                dl, _, checked, mask = sgm_ref.sgm_lr(oracle, L, R, 2, 80, *sgm_ref.auto_penalties(2))
            else:
                dl, _, checked, mask = census_ref.census_lr(oracle, L, R, 2, 80, "sgm")
            out[name, cost] = dl, checked, speckle_ref.speckle(checked, 200, 1, mask)[0]
    return out


def test_quality_on_books_and_art(pipeline):
    """463 x 370, r = 2, D = 80, auto penalties, speckle(200, 1), every run filled (max_gap = 2^24); bad =
    |d - gt| > 1 over gt > 0 with gt = disp1.png / 3, a hole counting as an error.  Measured:
                      SGM map   + LR check   + speckle   + row fill   holes before the fill
      Books, AD        0.3971     0.4084      0.4092      0.2895       0.271
      Books, census    0.3285     0.3428      0.3431      0.2414       0.238
      Art,   AD        0.5309     0.5511      0.5586      0.4293       0.398
      Art,   census    0.4398     0.4684      0.4724      0.3592       0.341"""
    gts = np.load(os.path.join(GOLDEN, "middlebury_gt.npz"))
    want = {("Books", "ad"): 0.2895, ("Books", "census"): 0.2414, ("Art", "ad"): 0.4293, ("Art", "census"): 0.3592}
    for (name, cost), (raw, checked, spk) in pipeline.items():
        gt = gts[name + "/disp1"].astype(np.float64) / 3.0
        filled = fill_ref.fill(spk, FILL_ALL)
        b = [sgm_ref.bad_rate(m, gt) for m in (raw, checked, spk, filled)]
        print(f"{name} {cost} r=2 D=80 bad-pixel rate: SGM {b[0]:.4f}, + LR check {b[1]:.4f}, + speckle {b[2]:.4f}, "
              f"+ row fill {b[3]:.4f}; holes before the fill {np.mean(spk == 0):.3f}")
        assert b[3] < b[1] and b[3] < b[0], (name, cost, b)
        assert round(b[3], 4) == want[name, cost], (name, cost, b)
        rows = (spk != 0).any(axis=1)
        assert filled[rows].all()                                       # no hole is left in a row that had a pixel
        assert np.array_equal(filled[spk != 0], spk[spk != 0])


# ---- the C ABI without a device ----
def test_symbols_and_constants():
    import gpu_stereo_matching_amd as sm
    from gpu_stereo_matching_amd import _capi
    lib = _capi.load()
    hdr = open(os.path.join(ROOT, "include", "sm_hip.h")).read()
    for n in ("sm_fill_invalid_device", "sm_fill_invalid_u8", "sm_fill_invalid_u16"):
        assert hasattr(lib, n) and n in _capi.EXPORTED and n + "(" in hdr, n
    assert _capi.SM_PARAM_FILL_GAP == 11 and "SM_PARAM_FILL_GAP = 11" in hdr
    for n in ("set_fill", "fill_invalid", "fill_invalid_device"):
        assert hasattr(sm.BlockMatcher, n), n
    assert hasattr(sm.BlockMatcherGroup, "set_fill")


def test_invalid_arguments_without_a_device():
    from gpu_stereo_matching_amd import _capi
    lib = _capi.load()
    INVALID = _capi.SM_ERR_INVALID_ARG
    err = lib.sm_last_error_string
    buf = (ctypes.c_uint8 * 4096)()
    m = ctypes.addressof(buf)

    def dev(elem=1, W=8, H=8, pitch=8, batch=1, stride=64, gap=1, ptr=m):
        return lib.sm_fill_invalid_device(None, ptr, elem, W, H, pitch, batch, stride, gap, None)

    # the arguments' own rules come first and need no handle; a call that passes them reports the null handle
    assert dev() == INVALID and b"null handle" in err()
    for kw, word in (({"elem": 0}, b"elem_bytes"), ({"elem": 3}, b"elem_bytes"), ({"elem": 4}, b"elem_bytes"),
                     ({"W": 0}, b"frame size"), ({"H": -1}, b"frame size"), ({"batch": 0}, b"batch"),
                     ({"pitch": 7}, b"pitch"), ({"gap": -1}, b"max_gap"), ({"gap": (1 << 24) + 1}, b"max_gap"),
                     ({"ptr": None}, b"null map"), ({"batch": 2, "stride": 63}, b"strides overlap"),
                     ({"H": 1 << 30, "batch": 2, "stride": 1 << 33}, b"2^31"),
                     ({"W": (1 << 30) + 1, "pitch": (1 << 30) + 1}, b"2^30")):
        assert dev(**kw) == INVALID and word in err() and b"fill" in err(), kw
    assert dev(gap=0) == INVALID and b"null handle" in err()       # max_gap 0 is legal, and still needs a handle
    assert dev(gap=1 << 24) == INVALID and b"null handle" in err()
    assert dev(elem=2, pitch=9) == INVALID and b"null handle" in err()
    assert dev(batch=2, stride=64) == INVALID and b"null handle" in err()
    for fn in (lib.sm_fill_invalid_u8, lib.sm_fill_invalid_u16):
        host = lambda W=8, H=8, pitch=8, gap=1, ptr=m: fn(None, ptr, W, H, pitch, gap)   # noqa: E731
        assert host() == INVALID and b"null handle" in err()
        assert host(gap=0) == INVALID and b"null handle" in err()
        for kw, word in (({"W": 0}, b"frame size"), ({"H": 0}, b"frame size"), ({"pitch": 7}, b"pitch"),
                         ({"gap": -1}, b"max_gap"), ({"gap": (1 << 24) + 1}, b"max_gap"), ({"ptr": None}, b"null map")):
            assert host(**kw) == INVALID and word in err() and b"fill" in err(), kw
    assert lib.sm_set_param_f(None, _capi.SM_PARAM_FILL_GAP, 1.0) == INVALID
    assert lib.sm_group_set_param_f(None, _capi.SM_PARAM_FILL_GAP, 1.0) == INVALID
