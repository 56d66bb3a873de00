"""CPU tests of the guided cost volume: the workspace arithmetic, the argument checks that need no device, the
symbols, and a model showing that the shapes of tests/test_gpu_guided_volume.py reach every compiled path of the
volume kernel.

The model restates the kernel's selection (guided_volume_shapes.tile_paths): guided_fused_kernel<R | 16, false> is
compiled for R = 0..7, and in each S1V with and without the column mask and S2H with and without the validity test,
both chosen per tile; the right band is restaged when D > 32.
"""
import ctypes
import os
import re

import guided_volume_shapes as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("sm_guided_volume_device", "sm_guided_volume_i32", "sm_guided_workspace_bytes")


def _lib():
    from gpu_stereo_matching_amd import _capi
    return _capi, _capi.load()


def _align256(v):
    return (v + 255) & ~255


def test_workspace_bytes_arithmetic():
    import gpu_stereo_matching_amd as sm
    for W, H, D, r in ((1920, 1080, 128, 5), (3840, 2160, 192, 5), (45, 33, 64, 1), (1, 1, 1, 0), (131, 40, 32, 7),
                       (4096, 7, 256, 0)):
        P = W * H
        assert sm.guided_workspace_bytes(W, H, D, r) == _align256(4 * P * D) + _align256(4 * P), (W, H, D, r)
    assert sm.guided_workspace_bytes(1920, 1080, 128, 5) == 4 * 1920 * 1080 * 128 + 4 * 1920 * 1080   # both 256-B multiples
    # the radius does not enter the size; it is checked
    assert sm.guided_workspace_bytes(64, 64, 16, 0) == sm.guided_workspace_bytes(64, 64, 16, 7)


def test_workspace_bytes_argument_checks():
    capi, L = _lib()
    n = ctypes.c_size_t(123)
    bad = ((0, 8, 8, 1, b"width"), (4097, 8, 8, 1, b"width"), (8, 0, 8, 1, b"height"), (8, 8, 0, 1, b"num_disp"),
           (8, 8, 257, 1, b"num_disp"), (8, 8, 8, -1, b"radius"), (8, 8, 8, 8, b"radius"))
    for W, H, D, r, word in bad:
        n.value = 123
        assert L.sm_guided_workspace_bytes(W, H, D, r, ctypes.byref(n)) == capi.SM_ERR_INVALID_ARG, (W, H, D, r)
        assert word in L.sm_last_error_string(), (W, H, D, r, L.sm_last_error_string())
        assert n.value == 0
    assert L.sm_guided_workspace_bytes(8, 8, 8, 1, None) == capi.SM_ERR_INVALID_ARG
    assert b"null" in L.sm_last_error_string()


def test_volume_calls_check_their_arguments_without_a_device():
    capi, L = _lib()
    # without a handle there is no SM_PARAM_GUIDED_SUBPIX: the sub-pixel calls refuse SM_AGG_GUIDED as before
    assert L.sm_match_subpix_device(None, None, None, 64, 8, 64, 1, 512, 2, 16, capi.SM_AGG_GUIDED, None, 64, 512,
                                    None, None, None) == capi.SM_ERR_INVALID_ARG
    assert b"no cost volume" in L.sm_last_error_string() and b"SM_PARAM_GUIDED_SUBPIX" in L.sm_last_error_string()
    assert L.sm_guided_volume_device(None, None, None, 8, 8, 8, 1, 8, None, None) == capi.SM_ERR_INVALID_ARG
    assert b"null handle" in L.sm_last_error_string()
    assert L.sm_guided_volume_i32(None, None, None, 8, 8, 8, 1, 8, None) == capi.SM_ERR_INVALID_ARG
    assert b"null handle" in L.sm_last_error_string()


def test_symbols():
    capi, L = _lib()
    assert capi.SM_PARAM_GUIDED_SUBPIX == 17
    assert "SM_PARAM_GUIDED_SUBPIX = 17" in open(os.path.join(ROOT, "include", "sm_hip.h")).read()
    header = open(os.path.join(ROOT, "include", "sm_hip.h")).read()
    for name in NEW:
        assert name in capi.EXPORTED
        assert re.search(r"SM_API\s+int\s+" + name + r"\s*\(", header), name
        assert getattr(L, name).argtypes is not None and getattr(L, name).restype is ctypes.c_int


def test_shapes_reach_every_compiled_path_of_the_volume_kernel():
    reached = {}
    for r, W, H, D, _ in S.volume_shapes():
        assert 0 <= r <= S.MAX_RADIUS and 1 <= D <= S.MAX_DISP and W <= 512 and H <= 256
        reached.setdefault(r, set()).update(S.tile_paths(r, W, H, D))
    for r in range(S.MAX_RADIUS + 1):
        got = reached.get(r, set())
        for nomask in (False, True):
            assert any(p[0] == nomask for p in got), f"r={r}: no tile with S1V nomask={nomask}"
        for lim in (False, True):
            assert any(p[1] == lim for p in got), f"r={r}: no tile with S2H lim={lim}"
        assert any(p[2] for p in got) and any(not p[2] for p in got), f"r={r}: with and without a right-band restage"
    shapes = S.volume_shapes()
    # the issue's cases are there
    assert any(W < D and W % S.tile_w(r) for r, W, H, D, _ in shapes)
    assert any(D == 1 for _, _, _, D, _ in shapes) and any((W, H, D) == (64, 8, 256) for _, W, H, D, _ in shapes)
    assert any(H > S.TILE_H for _, _, H, _, _ in shapes) and any(H < S.TILE_H for _, _, H, _, _ in shapes)
    assert any(D > W + 1 for _, W, _, D, _ in shapes)      # a plane where no pair exists


def test_model_selection_on_known_tiles():
    """tile_paths on frames worked out by hand from the kernel's conditions."""
    # r = 5: TW = 44.  W = 137, D = 8: tile 1 has px0 = 34 >= 7, px0 + 63 = 97 < 137 (no mask), x0 + TW - 1 = 87,
    # 7 <= 137 - 87 (no limit); tile 0 has px0 < 0 (mask); tile 3 (x0 = 132) has 7 > 137 - 175 (limit)
    assert S.tile_paths(5, 137, 9, 8) == {(False, False, False), (True, False, False), (False, True, False)}
    # D = 256 on a 64-wide frame at r = 3 (TW = 52): both tiles masked and limited, restaged
    assert S.tile_paths(3, 64, 8, 256) == {(False, True, True)}
