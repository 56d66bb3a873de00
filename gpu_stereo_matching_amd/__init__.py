"""MI355X-native stereo block matching (gfx950 HIP kernels behind a C ABI).

Host-side mirror of the reference's GPU proxy API (ningw42/GPU_Stereo_Matching):

    void blockMatching_gpu(Mat &h_left, Mat &h_right, Mat &h_disparity,
                           int SADWindowSize, int searchRange);      // Device.cuh:50

``blockMatching_gpu(h_left, h_right, SADWindowSize, searchRange)`` takes two uint8 gray
images (numpy, HxW) and returns the uint8 disparity map, with the reference's argument
meaning (SADWindowSize = window radius r, window (2r+1)^2; searchRange = number of
disparities) and output convention (0 where no window SAD is below 50*(2r+1)^2).

``BlockMatcher`` is the handle-based interface (buffers allocated once, device-resident
batched calls on torch tensors, LR check, guided aggregation, d-slice keys for multi-GPU).
All compute runs in ``libsm_hip.so``; there is no CPU fallback.
"""
from __future__ import annotations

import ctypes
from typing import Optional, Sequence, Tuple

import numpy as np

from . import _capi
from ._capi import SMError, SM_AGG_BOX, SM_AGG_GUIDED, SM_LR_CHECK, SM_MEDIAN, SM_STAGED, SM_DEVICE_CU_GRID, SM_AGG_SGM, SM_COST_CENSUS, SM_PAIRS_IN_VIEW  # noqa: F401
from .synth import synth_pair  # noqa: F401
from .gray import bgr_to_gray  # noqa: F401

__all__ = [
    "BlockMatcher", "BlockMatcherGroup", "blockMatching_gpu", "block_matching_gpu", "SMError", "synth_pair", "bgr_to_gray",
    "SM_AGG_BOX", "SM_AGG_GUIDED", "SM_AGG_SGM", "SM_COST_CENSUS", "SM_PAIRS_IN_VIEW", "SM_LR_CHECK", "SM_MEDIAN", "version", "host_empty",
    "sgm_penalties", "sgm_workspace_bytes", "census_workspace_bytes", "speckle_workspace_bytes", "to_float",
]

DEFAULT_GUIDED_EPS = 1e-4 * 255.0 * 255.0


def version() -> str:
    return _capi.load().sm_version().decode()


def _as_u8_image(a, name: str) -> np.ndarray:
    a = np.asarray(a)
    if a.dtype != np.uint8 or a.ndim != 2:
        raise ValueError(f"{name}: expected a 2-D uint8 (CV_8UC1) image, got {a.dtype} {a.shape}")
    return a if a.flags.c_contiguous else np.ascontiguousarray(a)


def _flags(agg: str, lr_check: bool, median: bool = False, cost: str = "ad", pairs: str = "reference") -> int:
    """cost: 'ad' (absolute gray difference) or 'census' (SM_COST_CENSUS: Hamming distance of 9 x 7 census words;
    agg 'box' or 'sgm', radius <= 7; the library rejects the other combinations with a reason).
    agg: 'box' (fused), 'box-staged' (through the AD / SAD volumes in HBM), 'guided', 'sgm' (four-path
    semi-global matching on the box SAD volume, radius <= 7), or 'device-cu' (Device.cu's literal output with
    its fixed launch geometry: SM_DEVICE_CU_GRID, box only).
    pairs: 'reference' (a pair (x, d) exists iff x + d <= W, the reference's rule) or 'in-view' (SM_PAIRS_IN_VIEW:
    x - d >= 0, stereo geometry, with the handle's minimum disparity; the calls that keep a cost volume, i.e. agg
    'sgm', cost 'census' and the sub-pixel calls; the library refuses it elsewhere with a reason)."""
    if agg not in ("box", "guided", "box-staged", "device-cu", "sgm"):
        raise ValueError("agg must be 'box', 'box-staged', 'guided', 'sgm' or 'device-cu'")
    if cost not in ("ad", "census"):
        raise ValueError("cost must be 'ad' or 'census'")
    if pairs not in ("reference", "in-view"):
        raise ValueError("pairs must be 'reference' or 'in-view'")
    f = {"box": SM_AGG_BOX, "guided": SM_AGG_GUIDED, "box-staged": SM_AGG_BOX | SM_STAGED,
         "device-cu": SM_DEVICE_CU_GRID, "sgm": SM_AGG_SGM}[agg]
    return f | (SM_LR_CHECK if lr_check else 0) | (SM_MEDIAN if median else 0) \
        | (SM_COST_CENSUS if cost == "census" else 0) | (SM_PAIRS_IN_VIEW if pairs == "in-view" else 0)


def sgm_penalties(radius: int, p1: int = 0, p2: int = 0, width: int = 1, cost: str = "ad",
                  pairs: str = "reference") -> Tuple[int, int]:
    """The (P1, P2) an 'sgm' match at `radius` uses for the parameter values p1, p2 (0 = auto: 8 win^2 and
    32 win^2; with cost='census' 10 win^2 and 120 win^2), through the library's own argument check
    (sm_sgm_check, host-only); raises SMError where the match would (P1 > P2, 255 win^2 + P2 > 65535, or
    62 win^2 + P2 > 65535 with the census cost, radius > 7, width > 4096)."""
    a, b = ctypes.c_int(), ctypes.c_int()
    _capi.check(_capi.load().sm_sgm_check(width, radius, _flags("sgm", False, False, cost, pairs), p1, p2,
                                          ctypes.byref(a),
                                          ctypes.byref(b)))
    return a.value, b.value


def sgm_workspace_bytes(width: int, height: int, num_disp: int, radius: int, p2: int = 0) -> int:
    """Bytes of device workspace one 'sgm' frame takes on its handle (sm_sgm_workspace_bytes, host-only)."""
    n = ctypes.c_size_t()
    _capi.check(_capi.load().sm_sgm_workspace_bytes(width, height, num_disp, radius, p2, ctypes.byref(n)))
    return n.value


def census_workspace_bytes(width: int, height: int, num_disp: int, radius: int, agg: str = "box") -> int:
    """Bytes of device workspace one cost='census' frame takes on its handle for agg 'box' or 'sgm'
    (sm_census_workspace_bytes, host-only), the two census images included."""
    if agg not in ("box", "sgm"):
        raise ValueError("agg must be 'box' or 'sgm'")
    n = ctypes.c_size_t()
    _capi.check(_capi.load().sm_census_workspace_bytes(width, height, num_disp, radius, _flags(agg, False, False, "census"),
                                                       ctypes.byref(n)))
    return n.value


def guided_workspace_bytes(width: int, height: int, num_disp: int, radius: int) -> int:
    """Bytes of the volume workspace one agg='guided' frame of the sub-pixel calls takes on its handle
    (sm_guided_workspace_bytes, host-only): the uint32 costs and the LR check's planes."""
    n = ctypes.c_size_t()
    _capi.check(_capi.load().sm_guided_workspace_bytes(width, height, num_disp, radius, ctypes.byref(n)))
    return n.value


def speckle_workspace_bytes(width: int, height: int, batch: int = 1) -> int:
    """Bytes of device workspace the speckle filter takes on its handle for `batch` frames (uint32 labels and
    counts, 8 B per pixel of the up to 8 frames in flight; sm_speckle_workspace_bytes, host-only)."""
    n = ctypes.c_size_t()
    _capi.check(_capi.load().sm_speckle_workspace_bytes(width, height, batch, ctypes.byref(n)))
    return n.value


def to_float(disp16):
    """A 1/16-px map (numpy uint16, or a torch int16 tensor holding the same bit patterns) as float32 pixels:
    q / 16, 0 where the pixel is invalid."""
    if isinstance(disp16, np.ndarray):
        return disp16.astype(np.float32) * np.float32(0.0625)
    import torch
    return disp16.to(torch.float32) * 0.0625


def _check_out(out_t, shape, dtype, device, name: str = "out_t"):
    """A caller-supplied output tensor: the C ABI writes prod(shape) elements through its raw pointer."""
    if out_t.dtype != dtype or tuple(out_t.shape) != tuple(shape) or not out_t.is_contiguous() \
            or out_t.device != device:
        raise ValueError(f"{name} must be a contiguous {dtype} tensor of shape {tuple(shape)} on {device}")


def _check_device_pair(left_t, right_t, keys_t=None):
    """[H, W] uint8 contiguous device frames of one shape (and an int32 [H, W] key map when given):
    the C ABI takes raw pointers and cannot check what they point at."""
    import torch
    if left_t.dtype != torch.uint8 or right_t.dtype != torch.uint8:
        raise ValueError("expected uint8 tensors")
    if left_t.shape != right_t.shape or left_t.dim() != 2:
        raise ValueError("left/right must be equal [H, W] tensors")
    if not (left_t.is_cuda and right_t.is_cuda and left_t.is_contiguous() and right_t.is_contiguous()):
        raise ValueError("expected contiguous device tensors")
    if keys_t is not None and (keys_t.dtype != torch.int32 or tuple(keys_t.shape) != tuple(left_t.shape)
                               or not keys_t.is_contiguous() or keys_t.device != left_t.device):
        raise ValueError("keys_t must be a contiguous int32 [H, W] tensor on the frames' device")


class _PinnedBlock:
    """Owner of one sm_host_alloc block; freed when the last array viewing it goes away."""

    def __init__(self, nbytes: int):
        self._lib = _capi.load()
        p = ctypes.c_void_p()
        _capi.check(self._lib.sm_host_alloc(nbytes, ctypes.byref(p)))
        self.ptr = p.value
        self.nbytes = nbytes

    def __del__(self):
        if getattr(self, "ptr", None):
            self._lib.sm_host_free(ctypes.c_void_p(self.ptr))
            self.ptr = None


def host_empty(shape, dtype=np.uint8) -> np.ndarray:
    """An uninitialised numpy array in page-locked host memory (``sm_host_alloc``): frames and maps
    kept here go to / from HBM as direct DMA in ``BlockMatcher.match`` and friends."""
    dt = np.dtype(dtype)
    n = int(np.prod(shape)) * dt.itemsize
    blk = _PinnedBlock(max(n, 1))
    buf = (ctypes.c_uint8 * max(n, 1)).from_address(blk.ptr)
    buf._sm_owner = blk  # the ctypes buffer keeps the block alive, and the array keeps the buffer
    return np.frombuffer(buf, dtype=dt, count=n // dt.itemsize).reshape(shape)


class BlockMatcher:
    """One device handle: pre-allocated buffers + a HIP stream (``sm_create``)."""

    def __init__(self, device: int = 0, max_width: int = 1920, max_height: int = 1080, max_disp: int = 256):
        self._lib = _capi.load()
        h = ctypes.c_void_p()
        _capi.check(self._lib.sm_create(device, max_width, max_height, max_disp, ctypes.byref(h)))
        self._h = h
        self.device = device
        self.max_width, self.max_height, self.max_disp = max_width, max_height, max_disp

    # -- lifetime ---------------------------------------------------------------------
    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            self._lib.sm_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def set_guided_eps(self, eps: float):
        _capi.check(self._lib.sm_set_param_f(self._h, _capi.SM_PARAM_GUIDED_EPS, float(eps)))

    def set_workspace_poison(self, byte=None):
        """A debugging aid (SM_PARAM_WORKSPACE_POISON): with byte in 0..255 every call first fills the handle's shared
        workspaces it takes, and the frame buffers a host call uploads into, with that byte, so that no result can
        depend on what an earlier call left there; one fill of each workspace per call.  None (the default) turns it
        off.  Results are the same under every byte; other values are refused and change nothing."""
        # (the parameter's 0 is "off" and v = byte + 1 otherwise; a negative byte must not arrive as 0)
        v = 0.0 if byte is None else float(byte) + 1.0 if byte >= 0 else -1.0
        _capi.check(self._lib.sm_set_param_f(self._h, _capi.SM_PARAM_WORKSPACE_POISON, v))

    def set_sgm_penalties(self, p1: int = 0, p2: int = 0):
        """Penalties of agg='sgm' (SM_PARAM_SGM_P1 / _P2): integers, 0 = auto (8 win^2 / 32 win^2 of the
        call's window).  P1 <= P2 and 255 win^2 + P2 <= 65535 are checked by the matching call."""
        _capi.check(self._lib.sm_set_param_f(self._h, _capi.SM_PARAM_SGM_P1, float(int(p1))))
        _capi.check(self._lib.sm_set_param_f(self._h, _capi.SM_PARAM_SGM_P2, float(int(p2))))

    def set_sgm_paths(self, paths: int = 4):
        """Scan directions agg='sgm' sums (SM_PARAM_SGM_PATHS): 4 (the default: along rows and columns) or 8, with
        the four diagonals too, as libSGM's SCAN_8PATH and StereoSGBM's MODE_HH.  Four more path passes per frame;
        the penalties, their bound and the workspace are the same.  Other values raise SMError."""
        _capi.check(self._lib.sm_set_param_f(self._h, _capi.SM_PARAM_SGM_PATHS, float(paths)))

    def set_min_disp(self, d0: int = 0):
        """StereoSGBM's minDisparity for the pairs='in-view' calls (SM_PARAM_MIN_DISP): an integer 0..4095, default 0.
        Those calls search d0 .. d0 + num_disp - 1 and return the absolute disparity (8-bit maps need
        d0 + num_disp - 1 <= 255, the 1/16-px maps <= 4095).  With d0 > 0 every other matching call is refused."""
        _capi.check(self._lib.sm_set_param_f(self._h, _capi.SM_PARAM_MIN_DISP, float(d0)))

    def set_box_kernel(self, kernel: int = 0):
        """Which kernel the plain box pass runs (SM_PARAM_BOX_KERNEL): 0 auto by launch size, 1 the VALU kernels,
        2 the matrix-pipe kernel, at every launch size; same maps and keys.  2 outside its scope (lr_check,
        radius 0, radius >= 8) runs the VALU kernels."""
        _capi.check(self._lib.sm_set_param_f(self._h, _capi.SM_PARAM_BOX_KERNEL, float(kernel)))

    def set_box_workgroups(self, n=0):
        """Workgroups of a matrix-pipe box launch (SM_PARAM_BOX_WORKGROUPS): 0 auto, n >= 1 that many, each walking
        a contiguous range of tiles and keeping the right band along a row; at most one per tile, so n >= tiles is one
        tile per workgroup.  Same maps and keys at every n; the VALU kernels ignore it."""
        _capi.check(self._lib.sm_set_param_f(self._h, _capi.SM_PARAM_BOX_WORKGROUPS, float(n)))

    def set_box_queue_workgroups(self, n=0):
        """Workgroups of a matrix-pipe box launch that draws its tiles from a queue (SM_PARAM_BOX_QUEUE_WORKGROUPS,
        with set_box_workgroups(0)): 0 auto, one per resident slot where the launch is large enough, n >= 1 that many
        at any launch size, also more than there are tiles.  Same maps and keys at every n."""
        _capi.check(self._lib.sm_set_param_f(self._h, _capi.SM_PARAM_BOX_QUEUE_WORKGROUPS, float(n)))

    def set_speckle(self, size: int = 0, range: int = 1):  # noqa: A002  (StereoSGBM's name)
        """StereoSGBM's speckleWindowSize / speckleRange (SM_PARAM_SPECKLE_SIZE / _RANGE): with size > 0 the
        whole-frame matching calls (match, match_lr, match_bgr, match_device, match_subpix[_device]) end with the
        speckle filter: regions of at most `size` pixels whose neighbours differ by at most `range` whole
        disparities become 0 (and leave the valid mask).  The defaults turn it off.  The row-band, d-slice and
        slice-key calls refuse a handle whose size is not 0."""
        _capi.check(self._lib.sm_set_param_f(self._h, _capi.SM_PARAM_SPECKLE_SIZE, float(int(size))))
        _capi.check(self._lib.sm_set_param_f(self._h, _capi.SM_PARAM_SPECKLE_RANGE, float(int(range))))

    def speckle_filter(self, map, max_size: int, max_diff: int, mask=None):  # noqa: A002
        """OpenCV's filterSpeckles(map, 0, max_size, max_diff) on a host map (sm_speckle_filter_u8 / _u16): a 2-D
        uint8 or uint16 array in which 0 is invalid.  Returns (filtered copy, mask): the mask is a copy of `mask`
        (uint8, the map's shape) cleared where pixels were removed, or None when no mask was given."""
        m = np.array(map, copy=True, order="C")
        if m.dtype not in (np.uint8, np.uint16) or m.ndim != 2:
            raise ValueError(f"map: expected a 2-D uint8 or uint16 map, got {m.dtype} {m.shape}")
        H, W = m.shape
        k = None
        if mask is not None:
            k = np.array(mask, copy=True, order="C")
            if k.dtype != np.uint8 or k.shape != m.shape:
                raise ValueError("mask must be a uint8 array of the map's shape")
        fn = self._lib.sm_speckle_filter_u8 if m.dtype == np.uint8 else self._lib.sm_speckle_filter_u16
        _capi.check(fn(self._h, m.ctypes.data, W, H, W, int(max_size), int(max_diff),
                       k.ctypes.data if k is not None else None, W))
        return m, k

    def speckle_filter_device(self, map_t, max_size: int, max_diff: int, mask=None, stream=None):
        """Device form of :meth:`speckle_filter` (sm_speckle_filter_device), in place and async on `stream`: map_t a
        uint8 or int16 (uint16 bit patterns) cuda tensor [H, W] or [B, H, W] with contiguous rows (row and frame
        strides are passed on); mask: an optional contiguous uint8 tensor of the map's shape, cleared where pixels
        are removed.  Returns map_t."""
        import torch
        if map_t.dtype not in (torch.uint8, torch.int16, torch.uint16) or map_t.dim() not in (2, 3) \
                or not map_t.is_cuda or map_t.stride(-1) != 1:
            raise ValueError("map_t must be a uint8 or int16 [H, W] or [B, H, W] device tensor with contiguous rows")
        if map_t.device.index != self.device:
            raise ValueError(f"the map must be on cuda:{self.device}, the handle's device")
        B = 1 if map_t.dim() == 2 else map_t.shape[0]
        H, W = map_t.shape[-2:]
        if mask is not None:
            _check_out(mask, map_t.shape, torch.uint8, map_t.device, "mask")
        fs = map_t.stride(0) if map_t.dim() == 3 else map_t.stride(-2) * H
        _capi.check(self._lib.sm_speckle_filter_device(
            self._h, map_t.data_ptr(), map_t.element_size(), W, H, map_t.stride(-2), B, fs, int(max_size),
            int(max_diff), mask.data_ptr() if mask is not None else None, self._stream_ptr(stream)))
        return map_t

    def set_fill(self, max_gap: int = 0):
        """The row fill as the matching calls' last step (SM_PARAM_FILL_GAP): with max_gap > 0 every call that
        returns a map (match, match_lr, match_bgr, match_device, match_subpix[_device], and the group's row bands)
        ends by filling each run of at most `max_gap` invalid pixels in a row with the smaller of its two
        neighbours, after the median, the LR check and the speckle filter, on the final left map only.  The mask
        and the right map stay: mask == 0 and disp != 0 marks the filled pixels.  The default turns it off.  The
        d-slice and slice-key calls refuse a handle whose gap is not 0."""
        _capi.check(self._lib.sm_set_param_f(self._h, _capi.SM_PARAM_FILL_GAP, float(int(max_gap))))

    def fill_invalid(self, map, max_gap: int):  # noqa: A002
        """The row fill on a host map (sm_fill_invalid_u8 / _u16): a 2-D uint8 or uint16 array in which 0 is
        invalid.  Returns the filled copy: every run of at most `max_gap` zeros in a row holds min(left, right) of
        its valid neighbours in that row (whole 16-bit values on a uint16 map), or the one neighbour it has at a
        border; longer runs, valid pixels and rows without a valid pixel are unchanged."""
        m = np.array(map, copy=True, order="C")
        if m.dtype not in (np.uint8, np.uint16) or m.ndim != 2:
            raise ValueError(f"map: expected a 2-D uint8 or uint16 map, got {m.dtype} {m.shape}")
        H, W = m.shape
        fn = self._lib.sm_fill_invalid_u8 if m.dtype == np.uint8 else self._lib.sm_fill_invalid_u16
        _capi.check(fn(self._h, m.ctypes.data, W, H, W, int(max_gap)))
        return m

    def fill_invalid_device(self, map_t, max_gap: int, stream=None):
        """Device form of :meth:`fill_invalid` (sm_fill_invalid_device), in place and async on `stream`: map_t a
        uint8 or int16 (uint16 bit patterns) cuda tensor [H, W] or [B, H, W] with contiguous rows (row and frame
        strides are passed on, so a view cut out of a larger tensor works).  Returns map_t."""
        import torch
        if map_t.dtype not in (torch.uint8, torch.int16, torch.uint16) or map_t.dim() not in (2, 3) \
                or not map_t.is_cuda or map_t.stride(-1) != 1:
            raise ValueError("map_t must be a uint8 or int16 [H, W] or [B, H, W] device tensor with contiguous rows")
        if map_t.device.index != self.device:
            raise ValueError(f"the map must be on cuda:{self.device}, the handle's device")
        B = 1 if map_t.dim() == 2 else map_t.shape[0]
        H, W = map_t.shape[-2:]
        fs = map_t.stride(0) if map_t.dim() == 3 else map_t.stride(-2) * H
        _capi.check(self._lib.sm_fill_invalid_device(
            self._h, map_t.data_ptr(), map_t.element_size(), W, H, map_t.stride(-2), B, fs, int(max_gap),
            self._stream_ptr(stream)))
        return map_t

    def dslice_rehearse(self, left, right, radius: int, num_disp: int, members: int, agg: str = "box",
                        lr_check: bool = False, pairs: str = "reference") -> np.ndarray:
        """The d-slice split of BlockMatcherGroup.match_dslice with `members` members, run one after
        another on this device (sm_dslice_rehearse_u8): same slice plan, padding and finalisation, with
        the RCCL MIN reduce-scatter replaced by an elementwise MIN of the members' key maps.  lr_check:
        the right view's keys take a second MIN and the map is LR-checked (StereoDisparity.cpp:136-147)."""
        if agg not in ("box", "guided"):
            raise ValueError("agg must be 'box' or 'guided'")
        L = _as_u8_image(left, "left")
        R = _as_u8_image(right, "right")
        if L.shape != R.shape:
            raise ValueError("left/right sizes differ")
        H, W = L.shape
        out = np.empty((H, W), np.uint8)
        _capi.check(self._lib.sm_dslice_rehearse_u8(self._h, L.ctypes.data, R.ctypes.data, W, H, W, radius, num_disp,
                                                    _flags(agg, lr_check, False, pairs=pairs), members,
                                                    out.ctypes.data, W))
        return out

    # -- host-pointer path (blockMatching_gpu replacement) -------------------------------
    def match(self, left, right, radius: int, num_disp: int, agg: str = "box", lr_check: bool = False,
              median: bool = False, out: Optional[np.ndarray] = None, cost: str = "ad",
              pairs: str = "reference") -> np.ndarray:
        """median=True: 7x7 median of the WTA map(s) (STMatching MeanFilter(disp, disp, 3)), before the LR check.
        out: optional contiguous uint8 [H, W] host buffer (e.g. pinned memory) to write the map into.
        cost: 'ad' or 'census' (SM_COST_CENSUS, with agg 'box' or 'sgm').
        pairs: 'reference' or 'in-view' (SM_PAIRS_IN_VIEW, with agg 'sgm' or cost 'census'; see set_min_disp)."""
        L = _as_u8_image(left, "left")
        R = _as_u8_image(right, "right")
        if L.shape != R.shape:
            raise ValueError("left/right sizes differ")
        H, W = L.shape
        if out is None:
            out = np.empty((H, W), np.uint8)
        elif out.dtype != np.uint8 or out.shape != (H, W) or not out.flags.c_contiguous:
            raise ValueError("out must be a contiguous uint8 array of the frame's shape")
        _capi.check(self._lib.sm_block_match_u8(self._h, L.ctypes.data, R.ctypes.data, W, H, W, radius, num_disp,
                                                _flags(agg, lr_check, median, cost, pairs), out.ctypes.data, W))
        return out

    def match_lr(self, left, right, radius: int, num_disp: int, agg: str = "box", median: bool = False,
                 cost: str = "ad", pairs: str = "reference") -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
        """(checked disparity, right-view disparity, valid mask)."""
        L = _as_u8_image(left, "left")
        R = _as_u8_image(right, "right")
        H, W = L.shape
        out = np.empty((H, W), np.uint8)
        rd = np.empty((H, W), np.uint8)
        mask = np.empty((H, W), np.uint8)
        _capi.check(self._lib.sm_block_match_lr_u8(self._h, L.ctypes.data, R.ctypes.data, W, H, W, radius, num_disp,
                                                   _flags(agg, True, median, cost, pairs), out.ctypes.data,
                                                   rd.ctypes.data,
                                                   mask.ctypes.data, W))
        return out, rd, mask

    def match_bgr(self, left_bgr, right_bgr, radius: int, num_disp: int, agg: str = "box",
                  lr_check: bool = False, cost: str = "ad", pairs: str = "reference") -> np.ndarray:
        """imread -> cvtColor(BGR2GRAY) -> blockMatching_gpu in one call (Caller.cpp:12-19): HxWx3/4
        uint8 BGR(A) frames in, uint8 disparity out; the gray conversion runs on the GPU."""
        Lb = np.ascontiguousarray(left_bgr, dtype=np.uint8)
        Rb = np.ascontiguousarray(right_bgr, dtype=np.uint8)
        if Lb.ndim != 3 or Lb.shape[2] not in (3, 4) or Lb.shape != Rb.shape:
            raise ValueError("expected two equal HxWx3 or HxWx4 uint8 BGR(A) frames")
        H, W, C = Lb.shape
        out = np.empty((H, W), np.uint8)
        _capi.check(self._lib.sm_block_match_bgr_u8(self._h, Lb.ctypes.data, Rb.ctypes.data, W, H, W * C, C, radius,
                                                    num_disp, _flags(agg, lr_check, False, cost, pairs),
                                                    out.ctypes.data, W))
        return out

    def segment_tree(self, left_bgr, right_bgr, max_level: int = 60, scale: int = 4, sigma: float = 0.1,
                     method: int = 0) -> np.ndarray:
        """STMatching's segment-tree stereo on HxWx3 uint8 BGR frames, `method` as STMatching/main.cpp's
        7th argument (defaults as its :49-52):
          0 = ST-1 (stereo_disparity_normal, StereoDisparity.cpp:57-89): colour + gradient cost over
              d < max_level -> tree aggregation on the left view's colour tree -> WTA -> 7x7 median -> x scale;
          1 = ST-2 (stereo_disparity_iteration, :91-160): first-pass left / right maps on colour trees of
              each view, the left-right check, then a colour + depth tree on the left view.
        Cost, filter, WTA, median, LR check and the trees' BFS on the GPU; segment_graph's passes on the
        host (sequential, as the reference's)."""
        Lb = np.ascontiguousarray(left_bgr, dtype=np.uint8)
        Rb = np.ascontiguousarray(right_bgr, dtype=np.uint8)
        if Lb.ndim != 3 or Lb.shape[2] != 3 or Lb.shape != Rb.shape:
            raise ValueError("expected two equal HxWx3 uint8 BGR frames")
        if method not in (0, 1):
            raise ValueError(f"method must be 0 (ST-1) or 1 (ST-2), got {method}")
        H, W, _ = Lb.shape
        out = np.empty((H, W), np.uint8)
        fn = self._lib.sm_segment_tree_refined_bgr_u8 if method else self._lib.sm_segment_tree_match_bgr_u8
        _capi.check(fn(self._h, Lb.ctypes.data, Rb.ctypes.data, W, H, 3 * W, max_level, scale, sigma,
                       out.ctypes.data, W))
        return out

    def segment_tree_stats(self) -> Tuple[float, float, int]:
        """(tree-build ms, whole-call ms, BFS levels of the last tree) of the last segment_tree call."""
        t, a, n = ctypes.c_float(), ctypes.c_float(), ctypes.c_int()
        _capi.check(self._lib.sm_last_segment_tree_stats(self._h, ctypes.byref(t), ctypes.byref(a), ctypes.byref(n)))
        return t.value, a.value, n.value

    def segment_tree_arrays(self, width: int, height: int) -> dict:
        """The last segment_tree call's last tree in BFS order (sm_last_segment_tree_arrays): rank, parent,
        first, child, lev (levels + 1 offsets) and pdist, for a width x height frame."""
        P = int(width) * int(height)
        ints = np.empty(5 * P + 2, np.int32)
        pdist = np.empty(P, np.uint8)
        n = ctypes.c_int()
        _capi.check(self._lib.sm_last_segment_tree_arrays(self._h, ints.ctypes.data, ints.size, pdist.ctypes.data,
                                                          pdist.size, ctypes.byref(n)))
        return {"rank": ints[:P].copy(), "parent": ints[P:2 * P].copy(), "first": ints[2 * P:3 * P].copy(),
                "child": ints[3 * P:4 * P].view(np.uint32).copy(), "lev": ints[4 * P:4 * P + n.value + 1].copy(),
                "pdist": pdist}

    def cvt_color(self, bgr) -> np.ndarray:
        """cvtColor_gpu (Device.cuh:52) on host memory: HxWx3|4 uint8 BGR(A) -> gray, OpenCV 2.4 weights."""
        B = np.ascontiguousarray(bgr, dtype=np.uint8)
        if B.ndim != 3 or B.shape[2] not in (3, 4):
            raise ValueError("expected an HxWx3 or HxWx4 uint8 BGR(A) image")
        H, W, C = B.shape
        out = np.empty((H, W), np.uint8)
        _capi.check(self._lib.sm_bgr_to_gray_u8(self._h, B.ctypes.data, W, H, W * C, C, out.ctypes.data, W))
        return out

    def remap(self, src, mapx, mapy) -> np.ndarray:
        """remap_gpu (Device.cuh:51) on host memory: uint8 [H, W] with CV_32FC1 maps [H, W]."""
        S = _as_u8_image(src, "src")
        mx = np.ascontiguousarray(mapx, dtype=np.float32)
        my = np.ascontiguousarray(mapy, dtype=np.float32)
        if mx.shape != S.shape or my.shape != S.shape:
            raise ValueError("maps must match the image shape")
        H, W = S.shape
        out = np.empty((H, W), np.uint8)
        _capi.check(self._lib.sm_remap_u8(self._h, S.ctypes.data, W, H, W, mx.ctypes.data, my.ctypes.data, W,
                                          out.ctypes.data, W))
        return out

    def ad_volume(self, left, right, num_disp: int) -> np.ndarray:
        """PreCal (BlockMatching.cpp:89-109) on the GPU: uint8 [num_disp, H, W], d-major, 0 where x < d."""
        L = _as_u8_image(left, "left")
        R = _as_u8_image(right, "right")
        H, W = L.shape
        out = np.empty((num_disp, H, W), np.uint8)
        _capi.check(self._lib.sm_ad_volume_u8(self._h, L.ctypes.data, R.ctypes.data, W, H, W, num_disp,
                                              out.ctypes.data))
        return out

    def guided_volume(self, left, right, radius: int, num_disp: int) -> np.ndarray:
        """The guided-filtered cost volume (sm_guided_volume_i32): int32 [num_disp, H, W], d-major,
        trunc(q(d) * 2^14) with q clamped to [-512, 512), the cost field of a one-disparity guided slice key;
        INT32_MAX where d > W - x.  One pass over all d; the handle's guided eps applies."""
        L = _as_u8_image(left, "left")
        R = _as_u8_image(right, "right")
        if L.shape != R.shape:
            raise ValueError("left/right sizes differ")
        H, W = L.shape
        out = np.empty((num_disp, H, W), np.int32)
        _capi.check(self._lib.sm_guided_volume_i32(self._h, L.ctypes.data, R.ctypes.data, W, H, W, radius, num_disp,
                                                   out.ctypes.data))
        return out

    def guided_volume_device(self, left_t, right_t, radius: int, num_disp: int, out_t=None, stream=None):
        """Device form of :meth:`guided_volume` (sm_guided_volume_device): [H, W] uint8 cuda tensors whose rows may
        be strided (stride(1) == 1, one row stride for both); int32 [num_disp, H, W] out, async on `stream`."""
        import torch
        if left_t.dtype != torch.uint8 or right_t.dtype != torch.uint8 or left_t.dim() != 2 \
                or left_t.shape != right_t.shape or not (left_t.is_cuda and right_t.is_cuda) \
                or left_t.stride(1) != 1 or right_t.stride(1) != 1 or left_t.stride(0) != right_t.stride(0):
            raise ValueError("expected two [H, W] uint8 device tensors of one shape and row stride")
        if left_t.device != right_t.device or left_t.device.index != self.device:
            raise ValueError(f"frames must be on cuda:{self.device}, the handle's device")
        H, W = left_t.shape
        if out_t is None:
            out_t = torch.empty((num_disp, H, W), dtype=torch.int32, device=left_t.device)
        _check_out(out_t, (num_disp, H, W), torch.int32, left_t.device)
        _capi.check(self._lib.sm_guided_volume_device(self._h, left_t.data_ptr(), right_t.data_ptr(), W, H,
                                                      left_t.stride(0), radius, num_disp, out_t.data_ptr(),
                                                      self._stream_ptr(stream)))
        return out_t

    def census_volume(self, left, right, num_disp: int) -> np.ndarray:
        """The Hamming volume of the census cost (sm_census_volume_u8): uint8 [num_disp, H, W], d-major,
        popcount(censusL(y, x) ^ censusR(y, x - d)) for x >= d, 0 where x < d."""
        L = _as_u8_image(left, "left")
        R = _as_u8_image(right, "right")
        if L.shape != R.shape:
            raise ValueError("left/right sizes differ")
        H, W = L.shape
        out = np.empty((num_disp, H, W), np.uint8)
        _capi.check(self._lib.sm_census_volume_u8(self._h, L.ctypes.data, R.ctypes.data, W, H, W, num_disp,
                                                  out.ctypes.data))
        return out

    def census_volume_device(self, left_t, right_t, num_disp: int, out_t=None, stream=None):
        """Device form of :meth:`census_volume`: [H, W] uint8 cuda tensors whose rows may be strided
        (stride(1) == 1, stride(0) >= W); uint8 [num_disp, H, W] out, async on `stream`."""
        import torch
        H, W = left_t.shape
        if left_t.stride(1) != 1 or right_t.stride(1) != 1 or left_t.stride(0) != right_t.stride(0) \
                or left_t.shape != right_t.shape:
            raise ValueError("expected two [H, W] uint8 tensors of one shape and row stride")
        if out_t is None:
            out_t = torch.empty((num_disp, H, W), dtype=torch.uint8, device=left_t.device)
        _check_out(out_t, (num_disp, H, W), torch.uint8, left_t.device)
        _capi.check(self._lib.sm_census_volume_device(self._h, left_t.data_ptr(), right_t.data_ptr(), W, H,
                                                      left_t.stride(0), num_disp, out_t.data_ptr(),
                                                      self._stream_ptr(stream)))
        return out_t

    def census_device(self, img_t, out_t=None, stream=None):
        """The 9 x 7 census words of an [H, W] uint8 cuda tensor (rows may be strided: stride(1) == 1) as an int64
        [H, W] tensor holding the uint64 bit patterns (62 bits used, so never negative); async on `stream`."""
        import torch
        if img_t.dtype != torch.uint8 or img_t.dim() != 2 or not img_t.is_cuda or img_t.stride(1) != 1:
            raise ValueError("expected an [H, W] uint8 device tensor with unit column stride")
        H, W = img_t.shape
        if out_t is None:
            out_t = torch.empty((H, W), dtype=torch.int64, device=img_t.device)
        _check_out(out_t, (H, W), torch.int64, img_t.device)
        _capi.check(self._lib.sm_census_device(self._h, img_t.data_ptr(), W, H, img_t.stride(0), out_t.data_ptr(),
                                               self._stream_ptr(stream)))
        return out_t

    def census(self, img) -> np.ndarray:
        """The census words of a host image: uint64 [H, W] (sm_census_device around an upload and a download)."""
        import torch
        I = _as_u8_image(img, "img")
        t = torch.from_numpy(I).to(f"cuda:{self.device}")
        return self.census_device(t).cpu().numpy().view(np.uint64)

    def all_sad(self, left, right, radius: int, num_disp: int) -> np.ndarray:
        """getAllSAD (BlockMatching.cpp:191-261) on the GPU: uint8 [H, W, num_disp] (pixel-major
        ``data_dm[p * D + d]``), each window SAD truncated to uchar, 255 where x + d > W."""
        L = _as_u8_image(left, "left")
        R = _as_u8_image(right, "right")
        H, W = L.shape
        out = np.empty((H, W, num_disp), np.uint8)
        _capi.check(self._lib.sm_all_sad_u8(self._h, L.ctypes.data, R.ctypes.data, W, H, W, radius, num_disp,
                                            out.ctypes.data))
        return out

    def all_sad_device(self, left_t, right_t, radius: int, num_disp: int, out_t=None, stream=None):
        """Device form of :meth:`all_sad`: uint8 [H, W, num_disp] CUDA tensor, async on `stream`."""
        import torch
        H, W = left_t.shape
        if out_t is None:
            out_t = torch.empty((H, W, num_disp), dtype=torch.uint8, device=left_t.device)
        _check_out(out_t, (H, W, num_disp), torch.uint8, left_t.device)
        _capi.check(self._lib.sm_all_sad_device(self._h, left_t.data_ptr(), right_t.data_ptr(), W, H, W, radius,
                                                num_disp, out_t.data_ptr(), self._stream_ptr(stream)))
        return out_t

    def sad_volume_device(self, left_t, right_t, radius: int, num_disp: int, out_t=None, stream=None):
        """u16 SAD volume [num_disp, H, W]: zero-padded (2r+1)^2 window sums of the AD planes."""
        import torch
        H, W = left_t.shape
        if out_t is None:
            out_t = torch.empty((num_disp, H, W), dtype=torch.int16, device=left_t.device)
        _capi.check(self._lib.sm_sad_volume_device(self._h, left_t.data_ptr(), right_t.data_ptr(), W, H, W, radius,
                                                   num_disp, out_t.data_ptr(), self._stream_ptr(stream)))
        return out_t

    def ad_volume_device(self, left_t, right_t, num_disp: int, out_t=None, stream=None):
        import torch
        H, W = left_t.shape
        if out_t is None:
            out_t = torch.empty((num_disp, H, W), dtype=torch.uint8, device=left_t.device)
        _capi.check(self._lib.sm_ad_volume_device(self._h, left_t.data_ptr(), right_t.data_ptr(), W, H, W, num_disp,
                                                  out_t.data_ptr(), self._stream_ptr(stream)))
        return out_t

    def bgr_to_gray_device(self, bgr_t, out_t=None, stream=None):
        """[H, W, 3|4] uint8 cuda tensor -> [H, W] gray (OpenCV 2.4 fixed point), async on `stream`."""
        import torch
        H, W, C = bgr_t.shape
        if out_t is None:
            out_t = torch.empty((H, W), dtype=torch.uint8, device=bgr_t.device)
        _capi.check(self._lib.sm_bgr_to_gray_device(self._h, bgr_t.data_ptr(), W, H, W * C, C, out_t.data_ptr(), W,
                                                    self._stream_ptr(stream)))
        return out_t

    def remap_device(self, src_t, mapx_t, mapy_t, out_t=None, stream=None):
        """Rectification remap (Device.cu:127-167): src [H, W] uint8, maps [H, W] float32 (CV_32FC1)."""
        import torch
        H, W = src_t.shape
        if out_t is None:
            out_t = torch.empty_like(src_t)
        _capi.check(self._lib.sm_remap_u8_device(self._h, src_t.data_ptr(), W, H, W, mapx_t.data_ptr(),
                                                 mapy_t.data_ptr(), W, out_t.data_ptr(), W, self._stream_ptr(stream)))
        return out_t

    @staticmethod
    def _map_args(K, dist, R, P):
        K = np.ascontiguousarray(K, np.float64).reshape(9)
        d = np.ascontiguousarray(dist if dist is not None else [], np.float64).ravel()
        R = np.ascontiguousarray(R, np.float64).reshape(9)
        P = np.ascontiguousarray(P, np.float64).reshape(12)
        return K, d, R, P

    def init_rectify_map(self, K, dist, R, P, width: int, height: int):
        """initUndistortRectifyMap(K, dist, R, P, (width, height), CV_32FC1) computed on the GPU
        (Utility.cpp:232-233): float32 (mapx, mapy) host arrays [height, width]."""
        K, d, R, P = self._map_args(K, dist, R, P)
        mx = np.empty((height, width), np.float32)
        my = np.empty((height, width), np.float32)
        vp = ctypes.c_void_p
        _capi.check(self._lib.sm_init_rectify_map(self._h, K.ctypes.data_as(vp), d.ctypes.data_as(vp) if d.size else None,
                                                  d.size, R.ctypes.data_as(vp), P.ctypes.data_as(vp), width, height,
                                                  mx.ctypes.data, my.ctypes.data, width))
        return mx, my

    def init_rectify_map_device(self, K, dist, R, P, width: int, height: int, mapx_t=None, mapy_t=None, stream=None):
        """Device form of :meth:`init_rectify_map`: float32 [height, width] CUDA tensors."""
        import torch
        K, d, R, P = self._map_args(K, dist, R, P)
        if mapx_t is None:
            mapx_t = torch.empty((height, width), dtype=torch.float32, device=f"cuda:{self.device}")
        if mapy_t is None:
            mapy_t = torch.empty((height, width), dtype=torch.float32, device=f"cuda:{self.device}")
        vp = ctypes.c_void_p
        _capi.check(self._lib.sm_init_rectify_map_device(
            self._h, K.ctypes.data_as(vp), d.ctypes.data_as(vp) if d.size else None, d.size, R.ctypes.data_as(vp),
            P.ctypes.data_as(vp), width, height, mapx_t.data_ptr(), mapy_t.data_ptr(), mapx_t.stride(0),
            self._stream_ptr(stream)))
        return mapx_t, mapy_t

    def median_device(self, src_t, radius: int = 3, out_t=None, stream=None):
        """(2r+1)^2 median, replicate borders (ctmf, STMatching/ctmf.c), r in 1..3; src [H, W] uint8."""
        import torch
        H, W = src_t.shape
        if out_t is None:
            out_t = torch.empty_like(src_t)
        _capi.check(self._lib.sm_median_u8_device(self._h, src_t.data_ptr(), W, H, W, radius, out_t.data_ptr(), W,
                                                  self._stream_ptr(stream)))
        return out_t

    def set_stage_timing(self, on) -> None:
        """Record the host calls' upload / match / download split: True always, False never (stage_ms()
        then reads 0), "auto" (the default) from the first stage_ms() call on.  Each recording costs two
        hipEvent markers between the stages, ~10 us per 1080p call."""
        v = 2.0 if on == "auto" else (1.0 if on else 0.0)
        _capi.check(self._lib.sm_set_param_f(self._h, _capi.SM_PARAM_STAGE_TIMING, v))

    def stage_ms(self) -> Tuple[float, float, float]:
        """(upload, match, download) ms of the last host call (Device.cu:218,238/257,292).  With the
        default "auto" timing the first read arms the recording for the calls after it."""
        u, m, d = ctypes.c_float(), ctypes.c_float(), ctypes.c_float()
        _capi.check(self._lib.sm_last_stage_ms(self._h, ctypes.byref(u), ctypes.byref(m), ctypes.byref(d)))
        return u.value, m.value, d.value

    def staged_kernel_ms(self) -> Tuple[float, float, float]:
        """(AD volume, SAD volume, WTA) kernel ms per frame of the last launch group (up to 8 frames) of the
        last 'box-staged' pass."""
        a, b, c = ctypes.c_float(), ctypes.c_float(), ctypes.c_float()
        _capi.check(self._lib.sm_last_staged_kernel_ms(self._h, ctypes.byref(a), ctypes.byref(b), ctypes.byref(c)))
        return a.value, b.value, c.value

    # -- device-resident path (torch tensors in HBM) ------------------------------------
    @staticmethod
    def _stream_ptr(stream):
        if stream is None:
            import torch
            stream = torch.cuda.current_stream()
        return ctypes.c_void_p(stream.cuda_stream)

    def match_device(self, left_t, right_t, radius: int, num_disp: int, out_t=None, agg: str = "box",
                     lr_check: bool = False, stream=None, median: bool = False, cost: str = "ad",
                     pairs: str = "reference"):
        """left_t/right_t: uint8 cuda tensors [H, W] or [B, H, W] (contiguous). Async on `stream`.
        cost='census': the frames of a batch run one after another through the handle's volume workspace."""
        import torch
        if left_t.dtype != torch.uint8 or right_t.dtype != torch.uint8:
            raise ValueError("expected uint8 tensors")
        if left_t.shape != right_t.shape or left_t.dim() not in (2, 3):
            raise ValueError("left/right must be equal [H,W] or [B,H,W]")
        if not (left_t.is_cuda and right_t.is_cuda and left_t.is_contiguous() and right_t.is_contiguous()):
            raise ValueError("expected contiguous device tensors")
        if left_t.device != right_t.device or left_t.device.index != self.device:
            raise ValueError(f"frames must be on cuda:{self.device}, the handle's device")
        B = 1 if left_t.dim() == 2 else left_t.shape[0]
        H, W = left_t.shape[-2:]
        if out_t is None:
            out_t = torch.empty_like(left_t)
        _check_out(out_t, left_t.shape, torch.uint8, left_t.device)
        _capi.check(self._lib.sm_match_device(self._h, left_t.data_ptr(), right_t.data_ptr(), W, H, W, B, H * W,
                                              radius, num_disp, _flags(agg, lr_check, median, cost, pairs),
                                              out_t.data_ptr(), W,
                                              H * W, self._stream_ptr(stream)))
        return out_t

    # -- sub-pixel maps (1/16 px, uint16), uniqueness filter, reprojection ------------------
    def set_uniqueness(self, u: int = 0):
        """Uniqueness ratio of the sub-pixel calls (SM_PARAM_UNIQUENESS): an integer 0..99, 0 = off.  A pixel is
        invalid when a disparity more than 1 away from its best costs less than best * 100 / (100 - u)."""
        _capi.check(self._lib.sm_set_param_f(self._h, _capi.SM_PARAM_UNIQUENESS, float(u)))

    def set_guided_subpix(self, on: bool = True):
        """SM_PARAM_GUIDED_SUBPIX: on, match_subpix and match_subpix_device take agg='guided' and build the guided
        cost volume per frame; off (the default) they refuse it, as they did before that volume existed."""
        _capi.check(self._lib.sm_set_param_f(self._h, _capi.SM_PARAM_GUIDED_SUBPIX, 1.0 if on else 0.0))

    def set_subpix_median(self, radius=0):
        """The 16-bit median of the sub-pixel calls (SM_PARAM_SUBPIX_MEDIAN): with radius 1..3, match_subpix,
        match_subpix_device and volume_wta_subpix_device filter both views' 1/16-px maps with the (2r+1)^2 median
        before the LR check, which then runs on the filtered maps rounded to whole disparities; the right-view map
        they return is the filtered one.  0 (the default) turns it off; other values are refused.  Every other call
        ignores it."""
        _capi.check(self._lib.sm_set_param_f(self._h, _capi.SM_PARAM_SUBPIX_MEDIAN, float(radius)))

    def median16(self, map, radius: int) -> np.ndarray:  # noqa: A002
        """The (2r+1)^2 median of a host uint16 map (sm_median_u16), replicate borders, radius 1..3, over the whole
        16-bit value (0 is a value like any other).  Returns a new array."""
        m = np.ascontiguousarray(map)
        if m.dtype != np.uint16 or m.ndim != 2:
            raise ValueError(f"map: expected a 2-D uint16 map, got {m.dtype} {m.shape}")
        H, W = m.shape
        out = np.empty((H, W), np.uint16)
        _capi.check(self._lib.sm_median_u16(self._h, m.ctypes.data, W, H, W, int(radius), out.ctypes.data, W))
        return out

    def median16_device(self, src_t, radius: int, out_t=None, stream=None):
        """Device form of :meth:`median16` (sm_median_u16_device), async on `stream`, not in place: src_t an int16
        (uint16 bit patterns) cuda tensor [H, W] or [B, H, W] with contiguous rows (row and frame strides are passed
        on, so a view cut out of a larger tensor works); out_t: an int16 tensor of the same shape with contiguous
        rows, allocated when None.  Returns out_t."""
        import torch
        if src_t.dtype not in (torch.int16, torch.uint16) or src_t.dim() not in (2, 3) or not src_t.is_cuda \
                or src_t.stride(-1) != 1:
            raise ValueError("src_t must be an int16 [H, W] or [B, H, W] device tensor with contiguous rows")
        if src_t.device.index != self.device:
            raise ValueError(f"the map must be on cuda:{self.device}, the handle's device")
        if out_t is None:
            out_t = torch.empty(tuple(src_t.shape), dtype=src_t.dtype, device=src_t.device)
        if out_t.dtype != src_t.dtype or out_t.shape != src_t.shape or out_t.stride(-1) != 1 \
                or out_t.device != src_t.device:
            raise ValueError("out_t must be a tensor of src_t's dtype and shape with contiguous rows")
        B = 1 if src_t.dim() == 2 else src_t.shape[0]
        H, W = src_t.shape[-2:]
        fs = src_t.stride(0) if src_t.dim() == 3 else src_t.stride(-2) * H
        ofs = out_t.stride(0) if out_t.dim() == 3 else out_t.stride(-2) * H
        _capi.check(self._lib.sm_median_u16_device(
            self._h, src_t.data_ptr(), W, H, src_t.stride(-2), B, fs, int(radius), out_t.data_ptr(),
            out_t.stride(-2), ofs, self._stream_ptr(stream)))
        return out_t

    def match_subpix(self, left, right, radius: int, num_disp: int, agg: str = "sgm", cost: str = "ad",
                     lr_check: bool = False, return_right: bool = False, return_mask: bool = False,
                     pairs: str = "reference"):
        """uint16 [H, W] disparity in 1/16 px (sm_block_match_subpix_u16): 16 * d + a parabola fit through the
        costs next to the best d, 0 where the pixel is invalid (uniqueness, the AD box threshold) or occluded
        (lr_check).  agg 'box', 'sgm' or, after set_guided_subpix(), 'guided' (the guided volume in one pass, invalid
        where q >= 50; cost 'ad', reference pairs and uniqueness 0 only), cost 'ad' or 'census', radius <= 7.  pairs='in-view': SM_PAIRS_IN_VIEW with
        the handle's minimum disparity, values up to 16 * 4095 + 8.  return_right / return_mask: a tuple
        (map[, right-view map][, uint8 valid mask])."""
        L = _as_u8_image(left, "left")
        R = _as_u8_image(right, "right")
        if L.shape != R.shape:
            raise ValueError("left/right sizes differ")
        H, W = L.shape
        out = np.empty((H, W), np.uint16)
        rd = np.empty((H, W), np.uint16) if return_right else None
        mask = np.empty((H, W), np.uint8) if return_mask else None
        _capi.check(self._lib.sm_block_match_subpix_u16(
            self._h, L.ctypes.data, R.ctypes.data, W, H, W, radius, num_disp,
            _flags(agg, lr_check, False, cost, pairs), out.ctypes.data, rd.ctypes.data if return_right else None,
            mask.ctypes.data if return_mask else None, W))
        res = (out,) + ((rd,) if return_right else ()) + ((mask,) if return_mask else ())
        return res[0] if len(res) == 1 else res

    def match_subpix_device(self, left_t, right_t, radius: int, num_disp: int, out_t=None, agg: str = "sgm",
                            cost: str = "ad", lr_check: bool = False, right_t16=None, mask_t=None, stream=None,
                            pairs: str = "reference"):
        """Device form of :meth:`match_subpix` (sm_match_subpix_device), async on `stream`.  left_t / right_t: uint8
        cuda tensors [H, W] or [B, H, W] of one layout whose rows are contiguous (row and frame strides are passed
        on).  The map comes back as an int16 tensor holding the uint16 bit patterns (at most 4088, so the values
        read the same); out_t may be any int16 tensor of the frames' shape with contiguous rows.  right_t16 (int16)
        and mask_t (uint8): optional contiguous tensors of the frames' shape for the right-view map and the mask."""
        import torch
        if left_t.dtype != torch.uint8 or right_t.dtype != torch.uint8:
            raise ValueError("expected uint8 tensors")
        if left_t.shape != right_t.shape or left_t.dim() not in (2, 3) or left_t.stride() != right_t.stride():
            raise ValueError("left/right must be equal [H,W] or [B,H,W] tensors of one layout")
        if not (left_t.is_cuda and right_t.is_cuda) or left_t.stride(-1) != 1:
            raise ValueError("expected device tensors with contiguous rows")
        if left_t.device != right_t.device or left_t.device.index != self.device:
            raise ValueError(f"frames must be on cuda:{self.device}, the handle's device")
        B = 1 if left_t.dim() == 2 else left_t.shape[0]
        H, W = left_t.shape[-2:]
        if out_t is None:
            out_t = torch.empty(tuple(left_t.shape), dtype=torch.int16, device=left_t.device)
        if out_t.dtype != torch.int16 or out_t.shape != left_t.shape or out_t.stride(-1) != 1 \
                or out_t.device != left_t.device:
            raise ValueError("out_t must be an int16 tensor of the frames' shape with contiguous rows")
        if right_t16 is not None:
            _check_out(right_t16, left_t.shape, torch.int16, left_t.device, "right_t16")
        if mask_t is not None:
            _check_out(mask_t, left_t.shape, torch.uint8, left_t.device, "mask_t")
        fs = left_t.stride(0) if left_t.dim() == 3 else left_t.stride(-2) * H
        ofs = out_t.stride(0) if out_t.dim() == 3 else out_t.stride(-2) * H
        _capi.check(self._lib.sm_match_subpix_device(
            self._h, left_t.data_ptr(), right_t.data_ptr(), W, H, left_t.stride(-2), B, fs, radius, num_disp,
            _flags(agg, lr_check, False, cost, pairs), out_t.data_ptr(), out_t.stride(-2), ofs,
            right_t16.data_ptr() if right_t16 is not None else None,
            mask_t.data_ptr() if mask_t is not None else None, self._stream_ptr(stream)))
        return out_t

    def volume_wta_subpix_device(self, vol_t, invalid_from: int = 0, lr_check: bool = False, out_t=None,
                                 right_t16=None, mask_t=None, stream=None, pairs: str = "reference"):
        """The sub-pixel WTA on a caller's cost volume (sm_volume_wta_subpix_device): vol_t a contiguous
        [D, H, W] cuda tensor of int16 (uint16 bit patterns) or int32 (uint32, costs < 2^24); the left view is
        invalid where its best cost is >= invalid_from (0 = no threshold); the handle's uniqueness applies.
        pairs='in-view': plane k of vol_t is the disparity set_min_disp's d0 + k, under SM_PAIRS_IN_VIEW.
        Returns the int16 [H, W] map (uint16 bit patterns)."""
        import torch
        if vol_t.dtype not in (torch.int16, torch.int32) or vol_t.dim() != 3 or not vol_t.is_cuda \
                or not vol_t.is_contiguous():
            raise ValueError("vol_t must be a contiguous int16 or int32 [D, H, W] device tensor")
        D, H, W = vol_t.shape
        if out_t is None:
            out_t = torch.empty((H, W), dtype=torch.int16, device=vol_t.device)
        _check_out(out_t, (H, W), torch.int16, vol_t.device)
        if right_t16 is not None:
            _check_out(right_t16, (H, W), torch.int16, vol_t.device, "right_t16")
        if mask_t is not None:
            _check_out(mask_t, (H, W), torch.uint8, vol_t.device, "mask_t")
        _capi.check(self._lib.sm_volume_wta_subpix_device(
            self._h, vol_t.data_ptr(), vol_t.element_size(), W, H, D, int(invalid_from),
            _flags("box", lr_check, pairs=pairs), out_t.data_ptr(), W,
            right_t16.data_ptr() if right_t16 is not None else None,
            mask_t.data_ptr() if mask_t is not None else None, self._stream_ptr(stream)))
        return out_t

    def reproject(self, disp16, Q) -> np.ndarray:
        """reprojectImageTo3D of a 1/16-px uint16 map (sm_reproject_u16): float32 [H, W, 3] points (X, Y, Z) / w of
        Q (x, y, q / 16, 1), (0, 0, 0) where q == 0.  Q: the 4 x 4 matrix of ``calib.stereo_rectify``."""
        d = np.ascontiguousarray(disp16)
        if d.dtype != np.uint16 or d.ndim != 2:
            raise ValueError(f"disp16: expected a 2-D uint16 map, got {d.dtype} {d.shape}")
        Q = np.ascontiguousarray(Q, np.float64).reshape(16)
        H, W = d.shape
        out = np.empty((H, W, 3), np.float32)
        _capi.check(self._lib.sm_reproject_u16(self._h, d.ctypes.data, W, H, W, Q.ctypes.data, out.ctypes.data, 3 * W))
        return out

    def reproject_device(self, disp_t16, Q, out_t=None, stream=None):
        """Device form of :meth:`reproject`: disp_t16 an int16 [H, W] cuda tensor with contiguous rows (uint16 bit
        patterns, as match_subpix_device returns), the points a float32 [H, W, 3] tensor; async on `stream`."""
        import torch
        if disp_t16.dtype != torch.int16 or disp_t16.dim() != 2 or not disp_t16.is_cuda or disp_t16.stride(-1) != 1:
            raise ValueError("disp_t16 must be an int16 [H, W] device tensor with contiguous rows")
        Q = np.ascontiguousarray(Q, np.float64).reshape(16)
        H, W = disp_t16.shape
        if out_t is None:
            out_t = torch.empty((H, W, 3), dtype=torch.float32, device=disp_t16.device)
        _check_out(out_t, (H, W, 3), torch.float32, disp_t16.device)
        _capi.check(self._lib.sm_reproject_device(self._h, disp_t16.data_ptr(), W, H, disp_t16.stride(0),
                                                  Q.ctypes.data, out_t.data_ptr(), 3 * W, self._stream_ptr(stream)))
        return out_t

    def slice_keys_device(self, left_t, right_t, radius: int, d_lo: int, d_hi: int, keys_t=None, stream=None):
        """Packed (SAD<<8|d) keys of the d-slice [d_lo, d_hi) as an int32 tensor (bit pattern of uint32)."""
        import torch
        H, W = left_t.shape[-2:]
        if keys_t is None:
            keys_t = torch.empty((H, W), dtype=torch.int32, device=left_t.device)
        _check_device_pair(left_t, right_t, keys_t)
        _capi.check(self._lib.sm_slice_keys_device(self._h, left_t.data_ptr(), right_t.data_ptr(), W, H, W, radius,
                                                   d_lo, d_hi, keys_t.data_ptr(), self._stream_ptr(stream)))
        return keys_t

    def keys_to_disp_device(self, keys_t, radius: int, out_t=None, stream=None):
        import torch
        H, W = keys_t.shape[-2:]
        if keys_t.dtype != torch.int32 or not keys_t.is_cuda or not keys_t.is_contiguous():
            raise ValueError("keys_t must be a contiguous int32 device tensor")
        if out_t is None:
            out_t = torch.empty((H, W), dtype=torch.uint8, device=keys_t.device)
        _check_out(out_t.view(-1) if out_t.is_contiguous() else out_t, (H * W,), torch.uint8, keys_t.device)
        _capi.check(self._lib.sm_keys_to_disp_device(self._h, keys_t.data_ptr(), W, H, radius, out_t.data_ptr(), W,
                                                     self._stream_ptr(stream)))
        return out_t

    def guided_slice_keys_device(self, left_t, right_t, radius: int, d_lo: int, d_hi: int, keys_t=None,
                                 stream=None):
        """Guided-aggregation d-slice keys ((int32)(q * 2^14) << 8 | d, INT32_MAX where no d of the slice
        is valid) as an int32 [H, W] tensor; disjoint slices combine with a signed elementwise min."""
        import torch
        H, W = left_t.shape[-2:]
        if keys_t is None:
            keys_t = torch.empty((H, W), dtype=torch.int32, device=left_t.device)
        _check_device_pair(left_t, right_t, keys_t)
        _capi.check(self._lib.sm_guided_slice_keys_device(self._h, left_t.data_ptr(), right_t.data_ptr(), W, H, W,
                                                          radius, d_lo, d_hi, keys_t.data_ptr(),
                                                          self._stream_ptr(stream)))
        return keys_t

    def slice_keys_lr_device(self, left_t, right_t, radius: int, d_lo: int, d_hi: int, agg: str = "box",
                             keys_t=None, right_keys_t=None, stream=None, pairs: str = "reference"):
        """Left AND right-view d-slice keys of [d_lo, d_hi) from one fused pass (sm_slice_keys_lr_device): int32
        [H, W] tensors holding the bit patterns of box uint32 keys (combine with an unsigned MIN) or guided
        int32 keys (signed MIN).  The right view's key of u is its best (cost << 8 | d) over the slice's d with
        u + d < W, C_R(u, d) = C_L(u + d, d) (StereoHelper.cpp:156-180)."""
        import torch
        if agg not in ("box", "guided"):
            raise ValueError("agg must be 'box' or 'guided'")
        H, W = left_t.shape[-2:]
        if keys_t is None:
            keys_t = torch.empty((H, W), dtype=torch.int32, device=left_t.device)
        if right_keys_t is None:
            right_keys_t = torch.empty((H, W), dtype=torch.int32, device=left_t.device)
        _check_device_pair(left_t, right_t, keys_t)
        _check_device_pair(left_t, right_t, right_keys_t)
        _capi.check(self._lib.sm_slice_keys_lr_device(self._h, left_t.data_ptr(), right_t.data_ptr(), W, H, W, radius,
                                                      d_lo, d_hi, _flags(agg, False, pairs=pairs), keys_t.data_ptr(),
                                                      right_keys_t.data_ptr(), self._stream_ptr(stream)))
        return keys_t, right_keys_t

    def right_keys_to_disp_device(self, keys_t, out_t=None, stream=None):
        """Combined right-view keys (any shape, int32) -> dR, the d field of each key (no threshold)."""
        import torch
        if keys_t.dtype != torch.int32 or not keys_t.is_contiguous() or not keys_t.is_cuda:
            raise ValueError("keys_t must be a contiguous int32 device tensor")
        if out_t is None:
            out_t = torch.empty(keys_t.shape, dtype=torch.uint8, device=keys_t.device)
        _check_out(out_t, keys_t.shape, torch.uint8, keys_t.device)
        _capi.check(self._lib.sm_right_keys_to_disp_device(self._h, keys_t.data_ptr(), keys_t.numel(), out_t.data_ptr(),
                                                           self._stream_ptr(stream)))
        return out_t

    def lr_check_device(self, left_disp_t, right_disp_t, out_t=None, mask_t=None, stream=None):
        """StereoDisparity.cpp:136-147 on [H, W] uint8 device maps: occluded (x - d < 0, d == 0 or
        |d - dR(x - d)| > 1) -> 0.  out_t may be left_disp_t (in place)."""
        import torch
        H, W = left_disp_t.shape
        for t in (left_disp_t, right_disp_t):
            _check_out(t, (H, W), torch.uint8, left_disp_t.device, "maps")
        if out_t is None:
            out_t = torch.empty_like(left_disp_t)
        _check_out(out_t, (H, W), torch.uint8, left_disp_t.device)
        if mask_t is not None:
            _check_out(mask_t, (H, W), torch.uint8, left_disp_t.device, "mask_t")
        _capi.check(self._lib.sm_lr_check_device(self._h, left_disp_t.data_ptr(), right_disp_t.data_ptr(), W, H, W,
                                                 out_t.data_ptr(), mask_t.data_ptr() if mask_t is not None else None,
                                                 W, self._stream_ptr(stream)))
        return out_t

    def guided_keys_to_disp_device(self, keys_t, out_t=None, stream=None):
        """Combined guided keys -> uint8 disparity (d where q < 50, else 0)."""
        import torch
        H, W = keys_t.shape[-2:]
        if keys_t.dtype != torch.int32 or not keys_t.is_cuda or not keys_t.is_contiguous():
            raise ValueError("keys_t must be a contiguous int32 device tensor")
        if out_t is None:
            out_t = torch.empty((H, W), dtype=torch.uint8, device=keys_t.device)
        _check_out(out_t.view(-1) if out_t.is_contiguous() else out_t, (H * W,), torch.uint8, keys_t.device)
        _capi.check(self._lib.sm_guided_keys_to_disp_device(self._h, keys_t.data_ptr(), W, H, out_t.data_ptr(), W,
                                                            self._stream_ptr(stream)))
        return out_t


class BlockMatcherGroup:
    """Several GPUs driven from this process through the C ABI's group handle (``sm_create_group``):
    one frame in row bands (one band per device, bit-identical to a single-device pass), or a batch
    of frames spread over the devices.  ``devices`` may repeat an index (several handles on one GPU)."""

    def __init__(self, devices: Sequence[int], max_width: int = 1920, max_height: int = 1080, max_disp: int = 256):
        self._lib = _capi.load()
        devs = (ctypes.c_int * len(devices))(*devices)
        g = ctypes.c_void_p()
        _capi.check(self._lib.sm_create_group(len(devices), devs, max_width, max_height, max_disp, ctypes.byref(g)))
        self._g = g
        self.devices = list(devices)

    def close(self):
        if getattr(self, "_g", None) is not None and self._g.value:
            self._lib.sm_destroy_group(self._g)
            self._g = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __len__(self):
        n = ctypes.c_int()
        _capi.check(self._lib.sm_group_size(self._g, ctypes.byref(n)))
        return n.value

    def set_guided_eps(self, eps: float):
        _capi.check(self._lib.sm_group_set_param_f(self._g, _capi.SM_PARAM_GUIDED_EPS, float(eps)))

    def set_sgm_penalties(self, p1: int = 0, p2: int = 0):
        """BlockMatcher.set_sgm_penalties on every member (agg='sgm' runs in match_batch only: whole frames)."""
        _capi.check(self._lib.sm_group_set_param_f(self._g, _capi.SM_PARAM_SGM_P1, float(int(p1))))
        _capi.check(self._lib.sm_group_set_param_f(self._g, _capi.SM_PARAM_SGM_P2, float(int(p2))))

    def set_sgm_paths(self, paths: int = 4):
        """BlockMatcher.set_sgm_paths on every member (agg='sgm' runs in match_batch only: whole frames)."""
        _capi.check(self._lib.sm_group_set_param_f(self._g, _capi.SM_PARAM_SGM_PATHS, float(paths)))

    def set_min_disp(self, d0: int = 0):
        """BlockMatcher.set_min_disp on every member (match_batch with pairs='in-view' honours it)."""
        _capi.check(self._lib.sm_group_set_param_f(self._g, _capi.SM_PARAM_MIN_DISP, float(d0)))

    def set_speckle(self, size: int = 0, range: int = 1):  # noqa: A002
        """BlockMatcher.set_speckle on every member: match_batch runs whole frames and honours it; the row-band
        calls (match, match_lr) and match_dslice refuse a size > 0 and say why."""
        _capi.check(self._lib.sm_group_set_param_f(self._g, _capi.SM_PARAM_SPECKLE_SIZE, float(int(size))))
        _capi.check(self._lib.sm_group_set_param_f(self._g, _capi.SM_PARAM_SPECKLE_RANGE, float(int(range))))

    def set_fill(self, max_gap: int = 0):
        """BlockMatcher.set_fill on every member: match_batch and the row-band calls (match, match_lr) honour it,
        since the rule never crosses a row; match_dslice refuses a gap > 0 and says why."""
        _capi.check(self._lib.sm_group_set_param_f(self._g, _capi.SM_PARAM_FILL_GAP, float(int(max_gap))))

    def match(self, left, right, radius: int, num_disp: int, agg: str = "box", lr_check: bool = False,
              median: bool = False, cost: str = "ad", pairs: str = "reference") -> np.ndarray:
        """One frame, row-banded over the group (sm_group_block_match_u8).  cost='census' needs whole frames
        (match_batch): the library refuses it here and says why."""
        L = _as_u8_image(left, "left")
        R = _as_u8_image(right, "right")
        if L.shape != R.shape:
            raise ValueError("left/right sizes differ")
        H, W = L.shape
        out = np.empty((H, W), np.uint8)
        _capi.check(self._lib.sm_group_block_match_u8(self._g, L.ctypes.data, R.ctypes.data, W, H, W, radius,
                                                      num_disp, _flags(agg, lr_check, median, cost, pairs),
                                                      out.ctypes.data, W))
        return out

    def match_lr(self, left, right, radius: int, num_disp: int, agg: str = "box", median: bool = False,
                 pairs: str = "reference") -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
        """(checked disparity, right-view disparity, valid mask), row-banded over the group."""
        L = _as_u8_image(left, "left")
        R = _as_u8_image(right, "right")
        H, W = L.shape
        out, rd, mask = (np.empty((H, W), np.uint8) for _ in range(3))
        _capi.check(self._lib.sm_group_block_match_lr_u8(self._g, L.ctypes.data, R.ctypes.data, W, H, W, radius,
                                                         num_disp, _flags(agg, True, median, pairs=pairs), out.ctypes.data,
                                                         rd.ctypes.data, mask.ctypes.data, W))
        return out, rd, mask

    def match_dslice(self, left, right, radius: int, num_disp: int, agg: str = "box",
                     lr_check: bool = False, pairs: str = "reference") -> np.ndarray:
        """One frame sharded over disparities (sm_group_dslice_block_match_u8): each member matches
        its slice of [0, num_disp), RCCL MIN reduce-scatter + all-gather over the members' devices.
        lr_check: the right view's slice keys take a second reduce-scatter + all-gather and the map is
        LR-checked.  Members must be distinct devices."""
        if agg not in ("box", "guided"):
            raise ValueError("agg must be 'box' or 'guided'")
        L = _as_u8_image(left, "left")
        R = _as_u8_image(right, "right")
        if L.shape != R.shape:
            raise ValueError("left/right sizes differ")
        H, W = L.shape
        out = np.empty((H, W), np.uint8)
        _capi.check(self._lib.sm_group_dslice_block_match_u8(self._g, L.ctypes.data, R.ctypes.data, W, H, W, radius,
                                                             num_disp, _flags(agg, lr_check, False, pairs=pairs),
                                                             out.ctypes.data, W))
        return out

    def match_batch(self, lefts, rights, radius: int, num_disp: int, agg: str = "box", lr_check: bool = False,
                    median: bool = False, cost: str = "ad", pairs: str = "reference"):
        """A list of equal-size pairs; frame f runs on member f mod len(group)."""
        Ls = [_as_u8_image(a, "left") for a in lefts]
        Rs = [_as_u8_image(a, "right") for a in rights]
        if len(Ls) != len(Rs) or any(a.shape != Ls[0].shape for a in Ls + Rs):
            raise ValueError("expected equal-size left/right lists")
        if not Ls:
            return []
        H, W = Ls[0].shape
        outs = [np.empty((H, W), np.uint8) for _ in Ls]
        n = len(Ls)
        ptrs = lambda arrs: (ctypes.c_void_p * n)(*[a.ctypes.data for a in arrs])  # noqa: E731
        _capi.check(self._lib.sm_group_block_match_batch_u8(self._g, ptrs(Ls), ptrs(Rs), n, W, H, W, radius,
                                                            num_disp, _flags(agg, lr_check, median, cost, pairs),
                                                            ptrs(outs), W))
        return outs


_default: Optional[BlockMatcher] = None


def _default_matcher(W: int, H: int, D: int) -> BlockMatcher:
    global _default
    if _default is None or W > _default.max_width or H > _default.max_height or D > _default.max_disp:
        if _default is not None:
            _default.close()
        _default = BlockMatcher(0, max(W, 1920), max(H, 1080), 256)
    return _default


def blockMatching_gpu(h_left, h_right, SADWindowSize: int, searchRange: int) -> np.ndarray:
    """Drop-in for ``blockMatching_gpu`` (Device.cu:173): returns the uint8 disparity map.

    Prints the reference's four stage lines in ms, as Device.cu:218,238,257,292 always does:
    "upload data", "pre calculation" (0: the AD cost is fused into the match), "find corr" and
    "download data".  ``SM_QUIET`` in the environment silences them.
    """
    import os
    L = _as_u8_image(h_left, "h_left")
    m = _default_matcher(L.shape[1], L.shape[0], searchRange)
    quiet = bool(os.environ.get("SM_QUIET"))
    if not quiet:
        m.set_stage_timing(True)
    out = m.match(L, h_right, SADWindowSize, searchRange)
    if not quiet:
        u, c, d = m.stage_ms()
        print(f"upload data : {u:g}\npre calculation : 0\nfind corr : {c:g}\ndownload data : {d:g}")
    return out


block_matching_gpu = blockMatching_gpu
