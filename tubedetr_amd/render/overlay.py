"""Grounded tubes drawn into decoded frames (td_tube_overlay, csrc/overlay.hip): ``annotate``."""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional, Sequence, Tuple, Union

import torch

from .. import _hip
from ..frame_jobs import _alpha, _check_geometry, _heat_grid, _launch_pooled, _planes, _put_src_dst, _rgb3, _thickness
from .clips import _as_list, _check_clip, _check_out, _clips_of, _device_of, _tube_tensors
from .frames import DeviceFrames, color_in_space


@dataclass(frozen=True)
class TubeStyle:
    """How an answer is drawn; colours are RGB whatever the frames' pixel format (``annotate`` converts them).  The
    defaults are the reference demo's: a #FAFF00 outline, no attention overlay, frames outside the span left as they are."""
    box_color: Tuple[int, int, int] = (0xFA, 0xFF, 0x00)
    thickness: int = 2
    heat_color: Tuple[int, int, int] = (255, 0, 0)
    heat_alpha: int = 0       # of 256, at an attention level of 255
    dim_color: Tuple[int, int, int] = (0, 0, 0)
    dim_alpha: int = 0        # of 256, on the frames outside the span

    def __post_init__(self):
        for n in ("box_color", "heat_color", "dim_color"):
            object.__setattr__(self, n, _rgb3(n, getattr(self, n)))
        for n in ("heat_alpha", "dim_alpha"):
            object.__setattr__(self, n, _alpha(n, getattr(self, n)))
        _thickness(self.thickness)


def heat_from_attention(ca_weights: torch.Tensor, hw: Tuple[int, int], n_valid: Optional[int] = None) -> torch.Tensor:
    """The decoder's cross-attention ``ca_weights`` (frames, 1, S) -> uint8 [frames][h][w] maps for ``annotate``: the first
    h w entries of a frame (its visual tokens; S = h w + text tokens) divided by the frame's largest, times 255, rounded.
    The text tokens' share of the attention is dropped, so a map says WHERE the query looked, not how much of its attention
    went to the picture.  ``n_valid``: use only the first n_valid frames.  Torch ops on the device, no host copy."""
    h, w = _heat_grid(hw)
    if ca_weights.dim() != 3 or ca_weights.shape[1] != 1 or ca_weights.shape[2] < h * w:
        raise ValueError(f"ca_weights {tuple(ca_weights.shape)}: (frames, 1, S) with S >= {h * w}")
    a = ca_weights[: n_valid if n_valid is not None else ca_weights.shape[0], 0, : h * w].float()
    top = a.amax(dim=1, keepdim=True).clamp_min(torch.finfo(torch.float32).tiny)
    return (a / top * 255.0 + 0.5).floor().clamp_(0, 255).to(torch.uint8).view(-1, h, w)


def overlay_job(src: int, T: int, sh: int, sw: int, dst: Optional[int] = None, pix_fmt: str = "rgb24", boxes: Optional[int] = None, n_tube: int = 0,
                span: Optional[int] = None, frame_map: Optional[int] = None, heat: Optional[int] = None, heat_hw: Tuple[int, int] = (0, 0),
                box_color=(0xFA, 0xFF, 0x00), heat_color=(255, 0, 0), dim_color=(0, 0, 0), thickness: int = 2, heat_alpha: int = 0, dim_alpha: int = 0,
                src_planes: Optional[Sequence[int]] = None, src_pitches: Optional[Sequence[int]] = None, src_frame_stride: Optional[int] = None,
                dst_planes: Optional[Sequence[int]] = None, dst_pitches: Optional[Sequence[int]] = None, dst_frame_stride: Optional[int] = None):
    """One ``td_overlay_job``: T frames of sh x sw in ``pix_fmt`` at device address ``src``, annotated into ``dst`` (None:
    in place).  ``boxes`` / ``span`` / ``frame_map`` / ``heat`` are device addresses or None (fp32 [n_tube][4], int64 [2],
    int32 [T], uint8 [n_tube][heat_hw[0]][heat_hw[1]]); the colours are three bytes in the FRAMES' colour space
    (``color_in_space``).  Without ``*_planes`` / ``*_pitches`` / ``*_frame_stride`` the frames are tightly packed
    (``DeviceFrames``); else the planes are the device addresses of frame 0's planes and the pitches their row pitches."""
    T, sh, sw = int(T), int(sh), int(sw)
    _check_geometry(pix_fmt, T, sh, sw)
    _thickness(thickness)
    mh, mw = _heat_grid(heat_hw, heat is not None)
    if n_tube < 0:
        raise ValueError(f"n_tube = {n_tube} is negative")
    fmt, tight, sizes = _planes(pix_fmt, sh, sw)
    j = _hip.OverlayJob()
    _put_src_dst(j, src, dst, sizes, tight, src_planes, src_pitches, src_frame_stride, dst_planes, dst_pitches, dst_frame_stride)
    j.fmt, j.T, j.sh, j.sw = fmt, T, sh, sw
    j.boxes, j.span, j.frame_map, j.heat = boxes, span, frame_map, heat
    j.n_tube, j.mh, j.mw = int(n_tube), mh, mw
    j.thickness, j.heat_alpha, j.dim_alpha = int(thickness), _alpha("heat_alpha", heat_alpha), _alpha("dim_alpha", dim_alpha)
    j.box_color[:], j.heat_color[:], j.dim_color[:] = _rgb3("box_color", box_color), _rgb3("heat_color", heat_color), _rgb3("dim_color", dim_color)
    return j


def annotate(frames: Union[DeviceFrames, Sequence[DeviceFrames]], boxes, span=None, heat=None, frame_map=None, style: TubeStyle = TubeStyle(),
             out: Union[None, DeviceFrames, Sequence[DeviceFrames]] = None):
    """Draw grounded tubes into decoded frames: ONE launch for one clip or for a list of clips (then ``boxes``, ``span``,
    ``heat``, ``frame_map`` and ``out`` are lists too, or None).  Per clip:
      boxes      fp32 (n_tube, 4) xyxy in the frames' pixels on the device: what ``PostProcess`` returned for the clip, stacked; None: no box;
      span       int64 (2,): the clip's row of ``sted_decode``'s output (first and last tube row with the object); None: all rows;
      heat       uint8 (n_tube, mh, mw) from ``heat_from_attention``; None: no attention overlay;
      frame_map  int32 (T,): the tube row of each frame (a clip decoded at full rate, a tube predicted at 5 fps); None: frame t is row t;
                 (``densify`` gives such a clip one interpolated box, span and map per frame instead: pass them with frame_map = None;)
      out        ``DeviceFrames`` of the same geometry to write into; the clip itself: in place; None: a new buffer.
    Returns the annotated ``DeviceFrames`` (a list for a list).  Nothing here synchronises or copies to the host; ``style``'s
    RGB colours are converted to the frames' colour space by ``color_in_space``."""
    single, clips = _clips_of(frames)
    if not clips:
        return []
    n, device = len(clips), _device_of(clips)
    boxes_l, span_l, heat_l, map_l, out_l = (_as_list(v, n, k) for v, k in ((boxes, "boxes"), (span, "span"), (heat, "heat"), (frame_map, "frame_map"), (out, "out")))
    prepared = []
    for c, b, s, h, m, o in zip(clips, boxes_l, span_l, heat_l, map_l, out_l):  # every refusal comes before the first allocation and the launch
        _check_clip(c, device)
        b, s, h, m = _tube_tensors(b, s, h, m, c.T, device)
        if b is not None and b.dim() != 2 or s is not None and s.dim() != 1 or m is not None and m.dim() != 1 or h is not None and h.dim() != 3:
            raise ValueError("boxes (n_tube, 4), span (2,), heat (n_tube, mh, mw), frame_map (T,)")
        if b is not None and h is not None and b.shape[0] != h.shape[0]:
            raise ValueError(f"boxes have {b.shape[0]} tube rows, heat has {h.shape[0]}")
        _check_out(o, c, device)
        if h is not None:
            _heat_grid(h.shape[1:])
        prepared.append((c, b, s, h, m, o))
    jobs, keep, results = [], [], []
    for c, b, s, h, m, o in prepared:
        n_tube = b.shape[0] if b is not None else h.shape[0] if h is not None else 2 ** 31 - 1  # span only: no array that a row could index past
        if o is None:
            o = c.empty_like()
        space = (c.pix_fmt, c.matrix, c.full_range)
        jobs.append(overlay_job(c.data.data_ptr(), c.T, c.h, c.w, o.data.data_ptr(), c.pix_fmt, _hip.ptr(b), n_tube, _hip.ptr(s), _hip.ptr(m), _hip.ptr(h),
                                tuple(h.shape[1:]) if h is not None else (0, 0), color_in_space(style.box_color, *space), color_in_space(style.heat_color, *space),
                                color_in_space(style.dim_color, *space), style.thickness, style.heat_alpha, style.dim_alpha))
        keep.append((b, s, h, m))
        results.append(o)
    return _launch_pooled("td_tube_overlay", jobs, keep, results, single, device)
