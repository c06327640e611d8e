"""Grounded tubes redacted in decoded frames (td_tube_redact, csrc/redact.hip): ``redact``."""
from __future__ import annotations

from typing import Optional, Sequence, Tuple, Union

import torch

from .. import _hip
from ..frame_jobs import MAX_RECTS, _check_geometry, _check_margin, _launch_pooled, _planes, _put_src_dst, _rgb3
from .clips import _as_list, _boxes_K, _check_clip, _check_K, _check_out, _clips_of, _device_of, _tube_tensors
from .frames import DeviceFrames, color_in_space

REDACT_MODES = ("fill", "mosaic", "blur")


def _redact_what(mode, cell, radius, margin, invert):
    if mode not in REDACT_MODES:
        raise ValueError(f"mode {mode!r}: one of {REDACT_MODES}")
    try:
        num, den = margin
    except (TypeError, ValueError):
        raise ValueError(f"margin {margin!r}: two integers") from None
    if any(isinstance(v, bool) or int(v) != v for v in (cell, radius, num, den)):
        raise ValueError(f"cell {cell!r}, radius {radius!r} and margin {margin!r}: integers")
    cell, radius, num, den = int(cell), int(radius), int(num), int(den)
    if mode == "mosaic" and not (2 <= cell <= 256 and cell % 2 == 0):
        raise ValueError(f"cell {cell}: an even number in 2..256")
    if mode == "blur" and not 1 <= radius <= 64:
        raise ValueError(f"radius {radius}: 1..64")
    _check_margin(num, den)
    if invert not in (0, 1, False, True):
        raise ValueError(f"invert {invert!r}: a bool")
    return REDACT_MODES.index(mode), cell, radius, num, den, int(bool(invert))


def redact_job(src: int, T: int, sh: int, sw: int, boxes: int, n_tube: int, K: int = 1, dst: Optional[int] = None, pix_fmt: str = "rgb24", span: Optional[int] = None,
               frame_map: Optional[int] = None, mode: str = "mosaic", cell: int = 16, radius: int = 8, color=(0, 0, 0), margin: Tuple[int, int] = (0, 1), invert: bool = False,
               src_planes: Optional[Sequence[int]] = None, src_pitches: Optional[Sequence[int]] = None, src_frame_stride: Optional[int] = None,
               dst_planes: Optional[Sequence[int]] = None, dst_pitches: Optional[Sequence[int]] = None, dst_frame_stride: Optional[int] = None):
    """One ``td_redact_job``: T frames of sh x sw in ``pix_fmt`` at device address ``src``, redacted into ``dst`` (None: in
    place).  ``boxes`` (fp32 [n_tube][K][4], required), ``span`` (int64 [K][2]) and ``frame_map`` (int32 [T]) are device
    addresses or None; ``color`` is three bytes in the FRAMES' colour space (``color_in_space``).  Without ``*_planes`` /
    ``*_pitches`` / ``*_frame_stride`` the frames are tightly packed (``DeviceFrames``); else the planes are the device
    addresses of frame 0's planes and the pitches their row pitches."""
    T, sh, sw, n_tube, K = int(T), int(sh), int(sw), int(n_tube), int(K)
    _check_geometry(pix_fmt, T, sh, sw)
    if n_tube < 1:
        raise ValueError(f"n_tube = {n_tube}: at least one tube row")
    if not 1 <= K <= MAX_RECTS:
        raise ValueError(f"K = {K}: 1..{MAX_RECTS} rectangles per tube row")
    if not boxes:
        raise ValueError("boxes is a device address, not None")
    code, cell, radius, num, den, inv = _redact_what(mode, cell, radius, margin, invert)
    fmt, tight, sizes = _planes(pix_fmt, sh, sw)
    j = _hip.RedactJob()
    _put_src_dst(j, src, dst, sizes, tight, src_planes, src_pitches, src_frame_stride, dst_planes, dst_pitches, dst_frame_stride)
    j.fmt, j.T, j.sh, j.sw = fmt, T, sh, sw
    j.boxes, j.span, j.frame_map = boxes, span, frame_map
    j.n_tube, j.K, j.mode, j.invert = n_tube, K, code, inv
    j.margin_num, j.margin_den, j.cell, j.radius = num, den, cell, radius
    j.color[:] = _rgb3("color", color)
    return j


def redact(frames: Union[DeviceFrames, Sequence[DeviceFrames]], boxes, span=None, frame_map=None, mode: str = "mosaic", cell: int = 16, radius: int = 8,
           color=(0, 0, 0), margin: Tuple[int, int] = (0, 1), invert: bool = False, out: Union[None, DeviceFrames, Sequence[DeviceFrames]] = None):
    """Hide grounded tubes in decoded frames - or, with ``invert``, everything but them: ONE launch for one clip or for a list
    of clips (then ``boxes``, ``span``, ``frame_map`` and ``out`` are lists too, or None).  Per clip:
      boxes      fp32 (n_tube, 4) or (n_tube, K, 4) xyxy in the frames' pixels on the device: one tube, or the K <= 8 tubes of a
                 clip whose UNION is hidden in one pass;
      span       int64 (2,) or (K, 2): a row of ``sted_decode``'s output or a pick of ``moments_topk`` per tube; None: all rows;
      frame_map  int32 (T,): the tube row of each frame; None: frame t is row t (``densify(mode="hull")`` covers the frames between two rows instead);
      out        ``DeviceFrames`` of the same geometry to write into; the clip itself: in place (not for "blur"); None: a new buffer.
    ``mode``: "fill" (``color``, RGB, converted by ``color_in_space``), "mosaic" (``cell`` even, 2..256) or "blur" (a box mean of
    ``radius`` 1..64); ``margin`` = (num, den) grows every box by num / den of its side first.  The rule is exact and stated in
    include/tubedetr_hip.h.  Returns the redacted ``DeviceFrames`` (a list for a list).  Nothing here synchronises or copies to
    the host."""
    single, clips = _clips_of(frames)
    if not clips:
        return []
    n, device = len(clips), _device_of(clips)
    _redact_what(mode, cell, radius, margin, invert)
    color = _rgb3("color", color)
    boxes_l, span_l, map_l, out_l = (_as_list(v, n, k) for v, k in ((boxes, "boxes"), (span, "span"), (frame_map, "frame_map"), (out, "out")))
    prepared = []
    for c, b, s, m, o in zip(clips, boxes_l, span_l, map_l, out_l):  # every refusal comes before the first allocation and the launch
        _check_clip(c, device)
        if b is None:
            raise ValueError("boxes: a torch.float32 tensor (n_tube, 4) or (n_tube, K, 4) per clip")
        b, s, _, m = _tube_tensors(b, s, None, m, c.T, device)
        shape = "boxes (n_tube, 4) or (n_tube, K, 4) with n_tube >= 1, frame_map (T,)"
        if m is not None and m.dim() != 1:
            raise ValueError(shape)
        K = _check_K(_boxes_K(b, shape), s, "boxes carry K = {K} rectangles per tube row")
        _check_out(o, c, device)
        if o is not None and mode == "blur" and o.data.data_ptr() == c.data.data_ptr():
            raise ValueError('mode "blur" cannot run in place (out is the clip itself): it reads neighbours that are already rewritten')
        prepared.append((c, b, s, m, o, K))
    jobs, keep, results = [], [], []
    for c, b, s, m, o, K in prepared:
        if o is None:
            o = c.empty_like()
        jobs.append(redact_job(c.data.data_ptr(), c.T, c.h, c.w, b.data_ptr(), b.shape[0], K, o.data.data_ptr(), c.pix_fmt, _hip.ptr(s), _hip.ptr(m), mode, cell, radius,
                               color_in_space(color, c.pix_fmt, c.matrix, c.full_range), margin, invert))
        keep.append((c.data, b, s, m))
        results.append(o)
    return _launch_pooled("td_tube_redact", jobs, keep, results, single, device)
