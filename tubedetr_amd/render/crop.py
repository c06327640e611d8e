"""Grounded tubes cropped out of decoded frames (td_tube_crop, csrc/tube_crop.hip): ``crop_tubes``."""
from __future__ import annotations

from typing import NamedTuple, Optional, Sequence, Tuple, Union

import torch

from .. import _hip
from ..frame_jobs import _MATRICES, _check_geometry, _check_margin, _describe, _launch_pooled, _planes, _put_planes
from .clips import _as_list, _check_clip, _clips_of, _device_of, _tube_tensors
from .frames import DeviceFrames

MAX_CROP_SRC_COLS = 8192
MAX_CROP_SIDE = 4096


class TubeCrops(NamedTuple):
    """What ``crop_tubes`` returns for one clip: the crops in the uint8 video + mask layout of a staged batch."""
    pixels: torch.Tensor   # uint8 (T, 3, oh, ow): the resized window in the top-left rh x rw, zeros elsewhere
    mask: torch.Tensor     # bool (T, oh, ow): True on the padding
    valid: torch.Tensor    # bool (T,): False for a frame without a crop (outside the span, no tube row, a degenerate box)
    windows: torch.Tensor  # int32 (T, 6): (wy0, wx0, ch, cw, rh, rw) - source window and resized size; zeros when not valid


def _check_src_width(sw: int):
    if sw > MAX_CROP_SRC_COLS:
        raise ValueError(f"frame width {sw}: at most {MAX_CROP_SRC_COLS} for a crop (the window can be the whole row)")


def _crop_geometry(size, margin, keep_aspect):
    try:
        oh, ow = size
        num, den = margin
    except (TypeError, ValueError):
        raise ValueError(f"size {size!r} and margin {margin!r}: two integers each") from None
    if any(isinstance(v, bool) or int(v) != v for v in (oh, ow, num, den)):
        raise ValueError(f"size {size!r} and margin {margin!r}: two integers each")
    oh, ow, num, den = int(oh), int(ow), int(num), int(den)
    if not (1 <= oh <= MAX_CROP_SIDE and 1 <= ow <= MAX_CROP_SIDE):
        raise ValueError(f"size {oh} x {ow}: sides in 1..{MAX_CROP_SIDE}")
    _check_margin(num, den)
    if keep_aspect not in (0, 1, False, True):
        raise ValueError(f"keep_aspect {keep_aspect!r}: a bool")
    return oh, ow, num, den, int(bool(keep_aspect))


def crop_job(src: int, T: int, sh: int, sw: int, boxes: int, n_tube: int, dst: int, size: Tuple[int, int] = (224, 224), pix_fmt: str = "rgb24", matrix: str = "bt601",
             full_range: bool = False, span: Optional[int] = None, frame_map: Optional[int] = None, margin: Tuple[int, int] = (0, 1), keep_aspect: bool = True,
             mask: Optional[int] = None, valid: Optional[int] = None, windows: Optional[int] = None,
             planes: Optional[Sequence[int]] = None, pitches: Optional[Sequence[int]] = None, frame_stride: Optional[int] = None):
    """One ``td_crop_job``: T frames of sh x sw in ``pix_fmt`` at device address ``src``, the tube ``boxes`` (fp32 [n_tube][4];
    ``span`` int64 [2] and ``frame_map`` int32 [T] or None) cropped into ``dst`` (uint8 [T][3][oh][ow]); ``mask`` ([T][oh][ow]),
    ``valid`` ([T]) and ``windows`` (int32 [T][6]) are device addresses or None.  Without ``planes`` / ``pitches`` /
    ``frame_stride`` the frames are tightly packed (``DeviceFrames``); else the planes are the device addresses of frame 0's
    planes and the pitches their row pitches."""
    T, sh, sw, n_tube = int(T), int(sh), int(sw), int(n_tube)
    _check_geometry(pix_fmt, T, sh, sw)
    _check_src_width(sw)
    if matrix not in _MATRICES:
        raise ValueError(f"matrix {matrix!r}: one of {_MATRICES}")
    if n_tube < 1:
        raise ValueError(f"n_tube = {n_tube}: at least one tube row")
    if not boxes or not dst:
        raise ValueError("boxes and dst are device addresses, not None")
    oh, ow, num, den, keep = _crop_geometry(size, margin, keep_aspect)
    fmt, tight, sizes = _planes(pix_fmt, sh, sw)
    j = _hip.CropJob()
    _put_planes(j, "", _describe(src, sizes, tight, planes, pitches, frame_stride))
    j.fmt, j.matrix, j.full_range = fmt, _MATRICES.index(matrix), int(bool(full_range))
    j.T, j.sh, j.sw = T, sh, sw
    j.boxes, j.span, j.frame_map, j.n_tube = boxes, span, frame_map, n_tube
    j.oh, j.ow, j.margin_num, j.margin_den, j.keep_aspect = oh, ow, num, den, keep
    j.dst, j.mask, j.valid, j.windows = dst, mask, valid, windows
    return j


def crop_tubes(frames: Union[DeviceFrames, Sequence[DeviceFrames]], boxes, span=None, frame_map=None, size: Tuple[int, int] = (224, 224),
               margin: Tuple[int, int] = (0, 1), keep_aspect: bool = True):
    """Crop grounded tubes out of decoded frames: ONE launch for one clip or for a list of clips (then ``boxes``, ``span`` and
    ``frame_map`` are lists too, or None; the same clip may appear several times, once per tube).  Per clip:
      boxes      fp32 (n_tube, 4) xyxy in the frames' pixels on the device: what ``PostProcess`` returned for the clip, stacked;
      span       int64 (2,): the clip's row of ``sted_decode``'s output; frames outside it get no crop; None: all rows;
      frame_map  int32 (T,): the tube row of each frame; None: frame t is row t (``densify`` interpolates the boxes to every frame instead).
    ``size`` = (oh, ow) of every crop; ``margin`` = (num, den): context of num / den of the box side added on every side before
    the window is clamped to the frame; ``keep_aspect``: the window keeps its shape inside oh x ow (padded at the bottom /
    right, ``mask`` True there) instead of being stretched.  The rule is exact and stated in include/tubedetr_hip.h.
    Returns ``TubeCrops`` (a list for a list).  Nothing here synchronises or copies to the host."""
    single, clips = _clips_of(frames)
    if not clips:
        return []
    n, device = len(clips), _device_of(clips)
    oh, ow, num, den, keep = _crop_geometry(size, margin, keep_aspect)
    boxes_l, span_l, map_l = (_as_list(v, n, k) for v, k in ((boxes, "boxes"), (span, "span"), (frame_map, "frame_map")))
    prepared = []
    for c, b, s, m in zip(clips, boxes_l, span_l, map_l):  # every refusal comes before the first allocation and the launch
        _check_clip(c, device)
        if b is None:
            raise ValueError("boxes: a torch.float32 tensor (n_tube, 4) per clip")
        b, s, _, m = _tube_tensors(b, s, None, m, c.T, device)
        if b.dim() != 2 or b.shape[0] < 1 or s is not None and s.dim() != 1 or m is not None and m.dim() != 1:
            raise ValueError("boxes (n_tube, 4) with n_tube >= 1, span (2,), frame_map (T,)")
        _check_src_width(c.w)
        prepared.append((c, b, s, m))
    jobs, keep_alive, results = [], [], []
    for c, b, s, m in prepared:
        pixels = torch.empty((c.T, 3, oh, ow), dtype=torch.uint8, device=device)
        mask = torch.empty((c.T, oh, ow), dtype=torch.bool, device=device)
        valid = torch.empty((c.T,), dtype=torch.bool, device=device)
        windows = torch.empty((c.T, 6), dtype=torch.int32, device=device)
        jobs.append(crop_job(c.data.data_ptr(), c.T, c.h, c.w, b.data_ptr(), b.shape[0], pixels.data_ptr(), (oh, ow), c.pix_fmt, c.matrix, c.full_range,
                             _hip.ptr(s), _hip.ptr(m), (num, den), bool(keep), mask.data_ptr(), valid.data_ptr(), windows.data_ptr()))
        keep_alive.append((c.data, b, s, m))
        results.append(TubeCrops(pixels, mask, valid, windows))
    return _launch_pooled("td_tube_crop", jobs, keep_alive, results, single, device)
