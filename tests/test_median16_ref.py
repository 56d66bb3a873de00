"""CPU tests of the 16-bit median's reference (tests/median16_ref.py) and of what sm_median_u16_device and
SM_PARAM_SUBPIX_MEDIAN decide without a device: the exported symbols and the argument rules."""
import ctypes

import numpy as np
import pytest

import median16_ref
import subpix_ref


@pytest.mark.parametrize("r", [1, 2, 3])
def test_equals_the_8bit_oracle_on_8bit_values(oracle, r):
    """uint8 data held in uint16: the ctmf restatement of the 8-bit path gives the same map."""
    rng = np.random.default_rng(r)
    for H, W in ((37, 53), (1, 9), (5, 2), (2, 2)):
        a8 = rng.integers(0, 256, (H, W)).astype(np.uint8)
        a8[rng.random((H, W)) < 0.3] = 0
        got = median16_ref.median(a8.astype(np.uint16), r)
        assert got.dtype == np.uint16
        assert np.array_equal(got, oracle.median(a8, r).astype(np.uint16)), (H, W)


@pytest.mark.parametrize("r", [1, 2, 3])
@pytest.mark.parametrize("shape", [(9, 11), (1, 11), (9, 1), (2, 3), (3, 2), (1, 1)])
def test_equals_the_sorted_window_loop(r, shape):
    """Full-range uint16, including frames with H or W smaller than r."""
    rng = np.random.default_rng(shape[0] * 100 + shape[1] + r)
    a = rng.integers(0, 65536, shape).astype(np.uint16)
    a[rng.random(shape) < 0.2] = 0
    a[rng.random(shape) < 0.1] = 0xFFFF
    assert np.array_equal(median16_ref.median(a, r), median16_ref.median_literal(a, r))
    two = np.where(rng.random(shape) < 0.5, 0x00FF, 0x0100).astype(np.uint16)   # order differs between the bytes
    assert np.array_equal(median16_ref.median(two, r), median16_ref.median_literal(two, r))


def test_rounding_and_check_rule():
    """(q + 8) >> 4 rounds half up in 32 bits, and the check runs on the filtered, rounded maps."""
    q = np.array([[0, 7, 8, 23, 24, 65528, 65535]], np.uint16)
    assert median16_ref.rounded(q).tolist() == [[0, 0, 1, 1, 2, 4096, 4096]]
    # a constant pair of maps: the median changes nothing, d = 2 everywhere, so x < 2 is occluded and the rest agrees
    ql = np.full((5, 9), 2 * 16 + 7, np.uint16)      # rounds to 2
    qr = np.full((5, 9), 3 * 16 - 8, np.uint16)      # 2.5 px rounds up to 3: |2 - 3| <= 1
    qm, qrm, mask = median16_ref.subpix_median(ql, qr, 1, True)
    assert np.array_equal(qrm, qr)
    assert not qm[:, :2].any() and (qm[:, 2:] == 39).all() and np.array_equal(mask, (qm != 0).astype(np.uint8))
    # 3.5 px in the right view rounds to 4, |2 - 4| > 1: all occluded; a floor in place of the rounding sees 3 and
    # keeps the pixels
    qr2 = np.full((5, 9), 3 * 16 + 8, np.uint16)
    assert not median16_ref.subpix_median(ql, qr2, 1, True)[0].any()
    assert not subpix_ref.lr_occluded(ql >> 4, qr2 >> 4)[:, 2:].any()
    # without the check the mask is the filtered map's validity, and an isolated hole is closed
    ql[2, 4] = 0
    qm, _, mask = median16_ref.subpix_median(ql, qr, 1, False)
    assert (qm == 39).all() and mask.all()


def _lib():
    from gpu_stereo_matching_amd import _capi
    return _capi, _capi.load()


def test_symbols_exported_and_declared():
    import os
    import re
    _capi, lib = _lib()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    txt = open(os.path.join(root, "include", "sm_hip.h")).read()
    declared = set(re.findall(r"SM_API\s+[\w\s\*]+?\b(sm_\w+)\s*\(", txt))
    assert declared == set(_capi.EXPORTED)
    for name in ("sm_median_u16_device", "sm_median_u16"):
        assert name in declared and hasattr(lib, name), name
    assert _capi.SM_PARAM_SUBPIX_MEDIAN == 15
    assert re.search(r"SM_PARAM_SUBPIX_MEDIAN\s*=\s*15\b", txt)


def test_argument_rules_without_a_device():
    """Every refusal names what was wrong, before the handle is looked at (fake non-null addresses: never read)."""
    _capi, lib = _lib()
    INVALID = _capi.SM_ERR_INVALID_ARG
    SRC, DST = 0x1000, 0x9000

    def dev(radius=1, width=64, height=8, pitch=64, batch=1, fs=512, src=SRC, dst=DST, dpitch=64, dfs=512):
        return lib.sm_median_u16_device(None, src, width, height, pitch, batch, fs, radius, dst, dpitch, dfs, None)

    def err():
        return lib.sm_last_error_string()

    for radius in (0, 4, -1):
        assert dev(radius=radius) == INVALID and b"radius %d" % radius in err() and b"[1, 3]" in err()
    assert dev(width=0) == INVALID and b"frame size" in err()
    assert dev(height=0) == INVALID and b"frame size" in err()
    assert dev(batch=0) == INVALID and b"batch 0" in err()
    assert dev(pitch=63) == INVALID and b"pitch 63 < width 64" in err() and b"dst_pitch" not in err()
    assert dev(dpitch=63) == INVALID and b"dst_pitch 63 < width 64" in err()
    assert dev(src=None) == INVALID and b"null source" in err()
    assert dev(dst=None) == INVALID and b"null destination" in err()
    assert dev(dst=SRC) == INVALID and b"same map" in err()
    assert dev(batch=2, fs=511) == INVALID and b"frame strides overlap" in err()
    assert dev(batch=2, dfs=511) == INVALID and b"frame strides overlap" in err()
    assert dev(batch=2) == INVALID and b"null handle" in err()
    assert dev() == INVALID and b"null handle" in err()
    # the host call: the same rules
    assert lib.sm_median_u16(None, SRC, 64, 8, 64, 0, DST, 64) == INVALID and b"radius 0" in err()
    assert lib.sm_median_u16(None, SRC, 64, 8, 64, 4, DST, 64) == INVALID and b"radius 4" in err()
    assert lib.sm_median_u16(None, SRC, 64, 8, 60, 1, DST, 64) == INVALID and b"pitch 60 < width 64" in err()
    assert lib.sm_median_u16(None, SRC, 64, 8, 64, 1, SRC, 64) == INVALID and b"same map" in err()
    assert lib.sm_median_u16(None, SRC, 64, 8, 64, 1, DST, 64) == INVALID and b"null handle" in err()
    # the parameter needs a handle
    assert lib.sm_set_param_f(None, _capi.SM_PARAM_SUBPIX_MEDIAN, ctypes.c_float(1.0)) == INVALID
    assert b"null handle" in err()


def test_sm_median_flag_points_to_the_parameter():
    _capi, lib = _lib()
    rc = lib.sm_match_subpix_device(None, None, None, 64, 8, 64, 1, 512, 2, 16, _capi.SM_AGG_SGM | _capi.SM_MEDIAN,
                                    None, 64, 512, None, None, None)
    msg = lib.sm_last_error_string()
    assert rc == _capi.SM_ERR_INVALID_ARG
    assert b"SM_MEDIAN" in msg and b"8-bit" in msg and b"SM_PARAM_SUBPIX_MEDIAN" in msg
