"""Rendered frames exported: cut, downscaled, converted (td_frame_export, csrc/frame_export.hip): ``export``."""
from __future__ import annotations

from typing import Optional, Sequence, Tuple, Union

import torch

from .. import _hip
from ..frame_jobs import _MATRICES, _PIX_FMTS, _check_geometry, _describe, _frame_bytes, _int_in, _launch_pooled, _planes, _put_planes, _rgb3
from .clips import _as_list, _check_clip, _clips_of, _dev_tensor, _device_of
from .dense import MAX_DENSE_STEP, MAX_DENSE_T, MAX_FRAME_NO
from .frames import DeviceFrames, color_in_space

MAX_EXPORT_SRC_COLS = 8192
MAX_EXPORT_RESIZE_PIXELS = 1 << 24


def export_job(src: int, T: int, sh: int, sw: int, dst: int, src_fmt: str = "rgb24", dst_fmt: Optional[str] = None, size: Optional[Tuple[int, int]] = None,
               frame_size: Optional[Tuple[int, int]] = None, pad=(0, 0, 0), take: Optional[int] = None, To: Optional[int] = None, valid: Optional[int] = None,
               matrix: str = "bt601", full_range: bool = False,
               src_planes: Optional[Sequence[int]] = None, src_pitches: Optional[Sequence[int]] = None, src_frame_stride: Optional[int] = None,
               dst_planes: Optional[Sequence[int]] = None, dst_pitches: Optional[Sequence[int]] = None, dst_frame_stride: Optional[int] = None):
    """One ``td_export_job``: T frames of sh x sw in ``src_fmt`` at device address ``src`` become ``To`` frames of ``frame_size``
    = (dh, dw) in ``dst_fmt`` (None: the source's) at ``dst``, the picture resized to ``size`` = (oh, ow) (None: kept) at the top
    left and ``pad`` - three bytes in the DESTINATION's colour space (``color_in_space``) - everywhere else (``frame_size`` None:
    no padding).  ``take`` (int32 [To]) and ``valid`` (bytes [To]) are device addresses or None; without ``take``, To is T.
    ``matrix`` / ``full_range`` describe whichever side is yuv.  Without ``*_planes`` / ``*_pitches`` / ``*_frame_stride`` both
    sides are tightly packed (``DeviceFrames``); else the planes are the device addresses of frame 0's planes and the pitches
    their row pitches."""
    T, sh, sw = int(T), int(sh), int(sw)
    _check_geometry(src_fmt, T, sh, sw)
    dst_fmt = src_fmt if dst_fmt is None else dst_fmt
    if sw > MAX_EXPORT_SRC_COLS:
        raise ValueError(f"frame width {sw}: at most {MAX_EXPORT_SRC_COLS} for an export")
    if matrix not in _MATRICES:
        raise ValueError(f"matrix {matrix!r}: one of {_MATRICES}")
    oh, ow = (sh, sw) if size is None else (int(size[0]), int(size[1]))
    if not (1 <= oh <= sh and 1 <= ow <= sw):
        raise ValueError(f"size {oh} x {ow}: between 1 x 1 and the source's {sh} x {sw} (nothing is enlarged)")
    if (oh, ow) != (sh, sw) and sh * sw > MAX_EXPORT_RESIZE_PIXELS:
        raise ValueError(f"a resizing export takes frames of at most 2^24 pixels, not {sh} x {sw}")
    dh, dw = (oh, ow) if frame_size is None else (int(frame_size[0]), int(frame_size[1]))
    if dh < oh or dw < ow:
        raise ValueError(f"frame_size {dh} x {dw} is smaller than the picture of {oh} x {ow}")
    To = (T if take is None else None) if To is None else int(To)
    if To is None:
        raise ValueError("To: the number of entries of take")
    if take is None and To != T:
        raise ValueError(f"To = {To} without take: it is T = {T}")
    _check_geometry(dst_fmt, To, dh, dw)
    if not dst and dst_planes is None:
        raise ValueError("dst is a device address, not None")
    sfmt, stight, ssizes = _planes(src_fmt, sh, sw)
    dfmt, dtight, dsizes = _planes(dst_fmt, dh, dw)
    j = _hip.ExportJob()
    _put_planes(j, "src", _describe(src, ssizes, stight, src_planes, src_pitches, src_frame_stride))
    _put_planes(j, "dst", _describe(dst, dsizes, dtight, dst_planes, dst_pitches, dst_frame_stride))
    j.src_fmt, j.dst_fmt, j.matrix, j.full_range = sfmt, dfmt, _MATRICES.index(matrix), int(bool(full_range))
    j.T, j.sh, j.sw, j.take, j.To, j.oh, j.ow, j.dh, j.dw = T, sh, sw, take, To, oh, ow, dh, dw
    j.pad[:] = _rgb3("pad", pad)
    j.valid = valid
    return j


def _export_size(size, sh: int, sw: int) -> Tuple[int, int]:
    if size is None:
        return sh, sw
    if isinstance(size, (tuple, list)):
        if len(size) != 2:
            raise ValueError(f"size {size!r}: (oh, ow) or the short side")
        return _int_in("oh", size[0], 1, sh), _int_in("ow", size[1], 1, sw)
    short, other = min(sh, sw), max(sh, sw)
    size = _int_in("size", size, 1, short)
    scaled = max(1, (2 * other * size + short) // (2 * short))  # rounded to nearest
    return (size, scaled) if sh <= sw else (scaled, size)


def moment_take(span: torch.Tensor, n: int, first: int = 0, step: int = 1) -> torch.Tensor:
    """``take`` for ``export`` from a moment: ``span`` is int64 (2,), first and last SAMPLED row of the answer (a row of
    ``sted_decode``'s output, a pick of ``moments_topk``), row r sampled at decoded frame first + r step.  Returns int32 (n,) on
    span's device: entry i is f0 + i with f0 = first + step span[0] for as long as f0 + i <= first + step span[1], then -1 (a
    blank frame).  Torch ops, no host copy: ``export(frames, take=moment_take(span, n), want_valid=True)`` cuts the clip to the answer."""
    if not torch.is_tensor(span) or span.dtype != torch.int64 or tuple(span.shape) != (2,):
        raise ValueError("span: an int64 tensor (2,)")
    n, first, step = _int_in("n", n, 0, MAX_DENSE_T), _int_in("first", first, -MAX_FRAME_NO, MAX_FRAME_NO), _int_in("step", step, 1, MAX_DENSE_STEP)
    idx = first + step * span[0] + torch.arange(n, dtype=torch.int64, device=span.device)
    return torch.where(idx <= first + step * span[1], idx, torch.full_like(idx, -1)).to(torch.int32)


def export(frames: Union[DeviceFrames, Sequence[DeviceFrames]], size=None, pix_fmt: Optional[str] = None, take=None, To: Optional[int] = None, multiple: int = 2,
           pad_color=(0, 0, 0), want_valid: bool = False):
    """Export rendered frames: ONE launch for one clip or for a list of clips (then ``take`` and ``To`` are lists too, or None).
      size       None: the frames' size; (oh, ow); or an int: the short side, the other one scaled with it (rounded to nearest,
                 at least 1).  Only the same size or smaller: an area mean, so nothing aliases at any ratio;
      pix_fmt    "rgb24" / "yuv420p" / "nv12"; None: the frames' own.  The clip's matrix and range describe the yuv side;
      take       which frames, in which order: None (all), an int32 tensor on the device (``moment_take``), or a Python sequence /
                 range.  An entry outside [0, T) gives a blank frame of ``pad_color``;
      To         the number of output frames when fewer than ``take`` has entries; None: all of them;
      multiple   the frame's sides are the picture's rounded up to a multiple of this (2: what yuv420p encoders want, the
                 reference demo's pad=ceil(iw/2)*2; 1: no padding), filled with ``pad_color`` (RGB; ``color_in_space`` converts it).
    Returns the exported ``DeviceFrames`` - with ``want_valid``, (``DeviceFrames``, bool (To,): False for a blank frame) - or a
    list of them.  The rule is exact and stated in include/tubedetr_hip.h.  Nothing here synchronises or copies to the host."""
    single, clips = _clips_of(frames)
    if not clips:
        return []
    n, device = len(clips), _device_of(clips)
    multiple = _int_in("multiple", multiple, 1, 256)
    pad_color = _rgb3("pad_color", pad_color)
    if pix_fmt is not None and pix_fmt not in _PIX_FMTS:
        raise ValueError(f"pix_fmt {pix_fmt!r}: one of {_PIX_FMTS}")
    take_l = [take] if single else _as_list(take, n, "take")
    To_l = [To] if single else _as_list(To, n, "To")
    prepared = []
    for c, tk, to in zip(clips, take_l, To_l):  # every refusal comes before the first allocation and the launch
        _check_clip(c, device)
        oh, ow = _export_size(size, c.h, c.w)
        dh, dw = -(-oh // multiple) * multiple, -(-ow // multiple) * multiple
        if tk is not None and not torch.is_tensor(tk):
            tk = torch.tensor([_int_in("take", v, -(1 << 31), (1 << 31) - 1) for v in tk], dtype=torch.int32).pin_memory().to(device, non_blocking=True)
        tk = _dev_tensor(tk, torch.int32, (), "take", device)
        if tk is not None and tk.dim() != 1:
            raise ValueError("take: int32 (To,)")
        n_out = c.T if tk is None else int(tk.numel())
        if to is not None:
            if tk is None and int(to) != c.T:
                raise ValueError(f"To = {to} without take: it is T = {c.T}")
            n_out = _int_in("To", to, 0, n_out)
        fmt = c.pix_fmt if pix_fmt is None else pix_fmt
        _check_geometry(fmt, n_out, dh, dw)
        prepared.append((c, tk, n_out, fmt, oh, ow, dh, dw))
    jobs, keep, results = [], [], []
    for c, tk, n_out, fmt, oh, ow, dh, dw in prepared:
        out = DeviceFrames(torch.empty(n_out * _frame_bytes(fmt, dh, dw), dtype=torch.uint8, device=device), n_out, dh, dw, fmt, c.matrix, c.full_range)
        valid = torch.empty((n_out,), dtype=torch.bool, device=device) if want_valid else None
        results.append((out, valid) if want_valid else out)
        if n_out == 0:  # nothing to write, and an empty tensor has no address to describe
            continue
        jobs.append(export_job(c.data.data_ptr(), c.T, c.h, c.w, out.data.data_ptr(), c.pix_fmt, fmt, (oh, ow), (dh, dw),
                               color_in_space(pad_color, fmt, c.matrix, c.full_range), _hip.ptr(tk), n_out, _hip.ptr(valid), c.matrix, c.full_range))
        keep.append((c.data, tk))
    return _launch_pooled("td_frame_export", jobs, keep, results, single, device)
