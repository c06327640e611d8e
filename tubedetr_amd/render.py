"""Grounded tubes drawn into decoded frames on the device (td_tube_overlay, csrc/overlay.hip; K labelled tubes and a moment
timeline in one pass: td_tube_overlay_multi, csrc/overlay_multi.hip: ``annotate_tubes``), cropped out of them
(td_tube_crop, csrc/tube_crop.hip: ``crop_tubes``) and hidden in them (td_tube_redact, csrc/redact.hip: ``redact``); and, at
the end of this file, the stage in front of the three: ``densify`` (td_tube_densify, csrc/tube_dense.hip) interpolates the tube
rows, one per SAMPLED frame, to one box per DECODED frame, and ``frame_stats`` / ``shot_cuts`` (td_frame_stats, td_shot_cuts,
csrc/frame_stats.hip) find the hard cuts in the frames, at which ``densify(shots=...)`` (td_tube_densify_shots) stops.  The stage
behind them all is ``export`` (td_frame_export, csrc/frame_export.hip): the frames of the answer, downscaled, in the pixel
format the encoder wants, padded to even sides - what crosses to the host is the proxy, not the decoded clip.

The reference shows an answer on the host: demo_stvg.py:152-194 and server_stvg.py:218-257 re-decode the video to JPEGs,
open every frame in matplotlib, draw one rectangle and save the JPEG again.  Here the decoded frames stay on the device in
the decoder's own pixel format (``DeviceFrames``); ``annotate`` writes the boxes ``PostProcess`` returned, the span
``sted_decode`` returned and - optionally - the decoder's cross-attention (``heat_from_attention``) into them in ONE launch
for any number of clips, and the result goes to an encoder pipe as it is.  The pixel rule is exact integer arithmetic and is
stated in include/tubedetr_hip.h; so is the colour conversion of ``color_in_space``.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import List, NamedTuple, Optional, Sequence, Tuple, Union

import torch

from .augment import _MATRICES, _PIX_FMTS, DecodedClip

MAX_SIDE = 16384
MAX_MAP = 256
_ONE = 1 << 20  # fixed-point one of color_in_space


def _rgb3(name: str, c) -> Tuple[int, int, int]:
    c = tuple(c)
    if len(c) != 3 or any(int(v) != v or not 0 <= v <= 255 for v in c):
        raise ValueError(f"{name} {c!r}: three integers in 0..255")
    return tuple(int(v) for v in c)


def _alpha(name: str, a) -> int:
    if int(a) != a or not 0 <= a <= 256:
        raise ValueError(f"{name} {a!r}: an integer in [0, 256]")
    return int(a)


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
        if int(self.thickness) != self.thickness or self.thickness < 1:
            raise ValueError(f"thickness {self.thickness!r}: an integer >= 1")


def _forward_coefficients(matrix: str, full_range: bool):
    kr, kb = (0.299, 0.114) if matrix == "bt601" else (0.2126, 0.0722)
    kg = 1.0 - kr - kb
    sy, sc = (1.0, 1.0) if full_range else (219.0 / 255.0, 224.0 / 255.0)
    rows = ((kr * sy, kg * sy, kb * sy),
            (-kr / (2 * (1 - kb)) * sc, -kg / (2 * (1 - kb)) * sc, 0.5 * sc),
            (0.5 * sc, -kg / (2 * (1 - kr)) * sc, -kb / (2 * (1 - kr)) * sc))
    return rows, (0 if full_range else 16, 128, 128)


def color_in_space(rgb, pix_fmt: str = "rgb24", matrix: str = "bt601", full_range: bool = False) -> Tuple[int, int, int]:
    """The three bytes a job needs for the RGB colour ``rgb``: itself for rgb24; (Y, U, V) for yuv420p / nv12, by the exact
    integer forward of the header's conversion: component = clamp((c_r R + c_g G + c_b B + 2^20 offset + 2^19) >> 20) with
    round(2^20 x) coefficients of the textbook matrix (include/tubedetr_hip.h lists them by Kr, Kb and the range).  Within
    0.5004 of a level of the float64 formula for every (R, G, B).  20 fraction bits, not the 16 of the device's yuv -> rgb
    rule: the three limited-range U coefficients all round the same way at 16 bits, which puts bright colours 0.5036 off."""
    r, g, b = _rgb3("rgb", rgb)
    if pix_fmt not in _PIX_FMTS:
        raise ValueError(f"pix_fmt {pix_fmt!r}: one of {_PIX_FMTS}")
    if pix_fmt == "rgb24":
        return r, g, b
    if matrix not in _MATRICES:
        raise ValueError(f"matrix {matrix!r}: one of {_MATRICES}")
    rows, offs = _forward_coefficients(matrix, bool(full_range))
    out = []
    for (cr, cg, cb), off in zip(rows, offs):
        acc = round(_ONE * cr) * r + round(_ONE * cg) * g + round(_ONE * cb) * b + _ONE * off + _ONE // 2
        out.append(min(max(acc >> 20, 0), 255))
    return tuple(out)


def heat_from_attention(ca_weights: torch.Tensor, hw: Tuple[int, int], n_valid: Optional[int] = None) -> torch.Tensor:
    """The decoder's cross-attention ``ca_weights`` (frames, 1, S) -> uint8 [frames][h][w] maps for ``annotate``: the first
    h w entries of a frame (its visual tokens; S = h w + text tokens) divided by the frame's largest, times 255, rounded.
    The text tokens' share of the attention is dropped, so a map says WHERE the query looked, not how much of its attention
    went to the picture.  ``n_valid``: use only the first n_valid frames.  Torch ops on the device, no host copy."""
    h, w = int(hw[0]), int(hw[1])
    if not (1 <= h <= MAX_MAP and 1 <= w <= MAX_MAP):
        raise ValueError(f"token grid {h} x {w}: sides in 1..{MAX_MAP}")
    if ca_weights.dim() != 3 or ca_weights.shape[1] != 1 or ca_weights.shape[2] < h * w:
        raise ValueError(f"ca_weights {tuple(ca_weights.shape)}: (frames, 1, S) with S >= {h * w}")
    a = ca_weights[: n_valid if n_valid is not None else ca_weights.shape[0], 0, : h * w].float()
    top = a.amax(dim=1, keepdim=True).clamp_min(torch.finfo(torch.float32).tiny)
    return (a / top * 255.0 + 0.5).floor().clamp_(0, 255).to(torch.uint8).view(-1, h, w)


def _frame_bytes(pix_fmt: str, h: int, w: int) -> int:
    if pix_fmt == "rgb24":
        return 3 * w * h
    return w * h + 2 * ((w + 1) // 2) * ((h + 1) // 2)


def _check_geometry(pix_fmt: str, T: int, h: int, w: int):
    if pix_fmt not in _PIX_FMTS:
        raise ValueError(f"pix_fmt {pix_fmt!r}: one of {_PIX_FMTS}")
    if T < 0:
        raise ValueError(f"T = {T} is negative")
    if not (1 <= h <= MAX_SIDE and 1 <= w <= MAX_SIDE):
        raise ValueError(f"frame size {h} x {w}: sides in 1..{MAX_SIDE}")


@dataclass
class DeviceFrames:
    """T decoded frames of h x w ON THE DEVICE, laid out as ``DecodedClip`` lays them out on the host: ``data`` is the flat
    uint8 tensor, tightly packed, frame after frame (yuv420p: Y, U, V; nv12: Y, UV; rgb24: (h, w, 3))."""
    data: torch.Tensor
    T: int
    h: int
    w: int
    pix_fmt: str = "yuv420p"
    matrix: str = "bt601"
    full_range: bool = False

    def __post_init__(self):
        self.T, self.h, self.w = int(self.T), int(self.h), int(self.w)
        _check_geometry(self.pix_fmt, self.T, self.h, self.w)
        if self.matrix not in _MATRICES:
            raise ValueError(f"matrix {self.matrix!r}: one of {_MATRICES}")
        d = self.data
        if not torch.is_tensor(d) or d.dtype != torch.uint8 or not d.is_cuda or not d.is_contiguous():
            raise ValueError("data is a contiguous uint8 tensor on the device")
        if d.numel() != self.T * self.nbytes_per_frame:
            raise ValueError(f"{d.numel()} bytes for {self.T} {self.pix_fmt} frames of {self.h} x {self.w} ({self.nbytes_per_frame} bytes each)")
        self.data = d.view(-1)

    @property
    def nbytes_per_frame(self) -> int:
        return _frame_bytes(self.pix_fmt, self.h, self.w)

    @classmethod
    def from_decoded(cls, clip: DecodedClip, device) -> "DeviceFrames":
        """One upload of a ``DecodedClip`` through page-locked memory (asynchronous on the current stream)."""
        host = clip.data if clip.data.is_pinned() else clip.data.pin_memory()
        return cls(host.to(device, non_blocking=True), clip.T, clip.h, clip.w, clip.pix_fmt, clip.matrix, clip.full_range)

    def to_decoded(self) -> DecodedClip:
        """The inverse of ``from_decoded``: one download into page-locked memory, asynchronous on the current stream - the
        ``DecodedClip``'s bytes are there once the stream has passed the copy (``torch.cuda.current_stream().synchronize()``)."""
        host = torch.empty(self.data.numel(), dtype=torch.uint8, pin_memory=True)
        host.copy_(self.data, non_blocking=True)
        return DecodedClip(host, self.T, self.h, self.w, self.pix_fmt, self.matrix, self.full_range)

    def empty_like(self) -> "DeviceFrames":
        return DeviceFrames(torch.empty_like(self.data), self.T, self.h, self.w, self.pix_fmt, self.matrix, self.full_range)


def _planes(pix_fmt: str, sh: int, sw: int):
    """(fmt code, tight pitches, plane sizes) of one frame."""
    from . import _hip

    ch, cw = (sh + 1) // 2, (sw + 1) // 2
    if pix_fmt == "rgb24":
        return _hip.TD_SRC_RGB24, [3 * sw], [3 * sw * sh]
    if pix_fmt == "yuv420p":
        return _hip.TD_SRC_I420, [sw, cw, cw], [sw * sh, cw * ch, cw * ch]
    return _hip.TD_SRC_NV12, [sw, 2 * cw], [sw * sh, 2 * cw * ch]


def _describe(base, sizes, tight, planes, pitches, frame_stride):
    pitches = list(tight if pitches is None else pitches)
    if planes is None:
        planes = [base + sum(sizes[:i]) for i in range(len(sizes))]
        if frame_stride is None:
            frame_stride = sum(sizes)
    if len(planes) != len(sizes) or len(pitches) != len(sizes) or frame_stride is None:
        raise ValueError("one address and one pitch per plane, and the frame stride")
    return list(planes) + [None] * (3 - len(sizes)), pitches + [0] * (3 - len(sizes)), int(frame_stride)


def _describe_src_dst(j, src, dst, sizes, tight, src_planes, src_pitches, src_frame_stride, dst_planes, dst_pitches, dst_frame_stride):
    """The src* and dst* fields of an overlay or redact job; neither ``dst`` nor ``dst_planes``: in place."""
    s = _describe(src, sizes, tight, src_planes, src_pitches, src_frame_stride)
    d = s if dst is None and dst_planes is None else _describe(dst, sizes, tight, dst_planes, dst_pitches, dst_frame_stride)
    (j.src0, j.src1, j.src2), (j.src_pitch0, j.src_pitch1, j.src_pitch2), j.src_frame_stride = s
    (j.dst0, j.dst1, j.dst2), (j.dst_pitch0, j.dst_pitch1, j.dst_pitch2), j.dst_frame_stride = d


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
    from . import _hip

    T, sh, sw = int(T), int(sh), int(sw)
    _check_geometry(pix_fmt, T, sh, sw)
    if int(thickness) != thickness or thickness < 1:
        raise ValueError(f"thickness {thickness!r}: an integer >= 1")
    mh, mw = int(heat_hw[0]), int(heat_hw[1])
    if heat is not None and not (1 <= mh <= MAX_MAP and 1 <= mw <= MAX_MAP):
        raise ValueError(f"token grid {mh} x {mw}: sides in 1..{MAX_MAP}")
    if n_tube < 0:
        raise ValueError(f"n_tube = {n_tube} is negative")
    fmt, tight, sizes = _planes(pix_fmt, sh, sw)
    j = _hip.OverlayJob()
    _describe_src_dst(j, src, dst, sizes, tight, src_planes, src_pitches, src_frame_stride, dst_planes, dst_pitches, dst_frame_stride)
    j.fmt, j.T, j.sh, j.sw = fmt, T, sh, sw
    j.boxes, j.span, j.frame_map, j.heat = boxes, span, frame_map, heat
    j.n_tube, j.mh, j.mw = int(n_tube), mh, mw
    j.thickness, j.heat_alpha, j.dim_alpha = int(thickness), _alpha("heat_alpha", heat_alpha), _alpha("dim_alpha", dim_alpha)
    j.box_color[:], j.heat_color[:], j.dim_color[:] = _rgb3("box_color", box_color), _rgb3("heat_color", heat_color), _rgb3("dim_color", dim_color)
    return j


_JOB_TYPES = {"td_tube_overlay": "OverlayJob", "td_tube_overlay_multi": "OverlayMultiJob", "td_tube_crop": "CropJob", "td_tube_redact": "RedactJob",
              "td_tube_densify": "DenseJob", "td_frame_stats": "StatsJob", "td_shot_cuts": "CutsJob", "td_tube_follow": "FollowJob", "td_frame_export": "ExportJob"}  # entry point -> its record in _hip


def _enqueue(entry: str, jobs: Sequence, host: torch.Tensor, dev: torch.Tensor, nbytes: int):
    from . import _hip

    arr = (getattr(_hip, _JOB_TYPES[entry]) * len(jobs))(*jobs)
    _hip.check(getattr(_hip.lib(), entry)(arr, len(jobs), host.data_ptr(), dev.data_ptr(), nbytes, _hip.stream_ptr()), entry)


def _launch_fresh(entry: str, jobs: Sequence, device) -> tuple:
    """tube_overlay / tube_crop / tube_redact: one launch on the current stream with freshly allocated job tables."""
    from . import _hip

    nb = int(getattr(_hip.lib(), entry + "_table_bytes")(len(jobs)))
    host = torch.empty(max(nb, 256), dtype=torch.uint8, pin_memory=True)
    dev = torch.empty(max(nb, 256), dtype=torch.uint8, device=device)
    _enqueue(entry, jobs, host, dev, nb)
    return host, dev


def tube_overlay(jobs: Sequence, device) -> tuple:
    """One td_tube_overlay launch on the current stream with freshly allocated job tables; returns them: the caller keeps
    them alive until the stream has passed the launch (``annotate`` recycles its own instead)."""
    return _launch_fresh("td_tube_overlay", jobs, device)


# job tables of annotate(): (pinned, device, event recorded behind the launch).  A table is taken again only once its event has
# completed (a query, never a wait); otherwise a new one is made, so the pool grows to the number of launches in flight.
_tables: List[tuple] = []


def _take_table(nb: int, device):
    for i, (host, dev, ev) in enumerate(_tables):
        if host.numel() >= nb and dev.device == device and ev.query():
            return _tables.pop(i)
    n = max(nb, 4096)
    return torch.empty(n, dtype=torch.uint8, pin_memory=True), torch.empty(n, dtype=torch.uint8, device=device), torch.cuda.Event()


def _launch_pooled(entry: str, jobs: Sequence, keep: Sequence, results: list, single: bool, device, tail_bytes: int = 0, fill_tail=None, enqueue=None):
    """annotate / crop_tubes / redact / densify: one launch on the current stream with a pooled job table; ``keep`` holds, per
    clip, the tensors that the launch reads; returns ``results`` (its only entry for a single clip).  ``tail_bytes`` more bytes
    of the pooled pair are handed to ``fill_tail(host_tail, dev_tail)`` before the launch: small host inputs of the jobs travel
    in the table's memory and are guarded by its event.  ``enqueue(host, dev, nbytes)`` replaces the plain call of ``entry``,
    whose ``_table_bytes`` still sizes the table."""
    from . import _hip

    nb = int(getattr(_hip.lib(), entry + "_table_bytes")(len(jobs)))
    host, dev, ev = _take_table(nb + tail_bytes, device)
    if tail_bytes:
        fill_tail(host[nb:nb + tail_bytes], dev[nb:nb + tail_bytes])
    if enqueue is not None:
        enqueue(host, dev, host.numel())
    else:
        _enqueue(entry, jobs, host, dev, host.numel())
    ev.record()
    _tables.append((host, dev, ev))
    stream = torch.cuda.current_stream(device)
    for group in keep:  # contiguous() may have made copies: the allocator must not hand them out before the launch has run
        for t in group:
            if t is not None:
                t.record_stream(stream)
    return results[0] if single else results


def _as_list(v, n: int, name: str):
    if v is None:
        return [None] * n
    if isinstance(v, (list, tuple)):
        if len(v) != n:
            raise ValueError(f"{name}: {len(v)} entries for {n} clips")
        return list(v)
    if n != 1:
        raise ValueError(f"{name}: a list with one entry per clip")
    return [v]


def _dev_tensor(t, dtype, shape_tail, name, device):
    if t is None:
        return None
    ok = torch.is_tensor(t) and t.device == device and t.dtype == dtype
    if ok and shape_tail:
        ok = t.dim() >= len(shape_tail) and tuple(t.shape[t.dim() - len(shape_tail):]) == tuple(shape_tail)
    if not ok:
        raise ValueError(f"{name}: a {dtype} tensor [..., {', '.join(map(str, shape_tail))}] on {device}")
    return t.contiguous()


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
    from . import _hip

    single = isinstance(frames, DeviceFrames)
    clips = [frames] if single else list(frames)
    n = len(clips)
    if n == 0:
        return []
    device = clips[0].data.device
    boxes_l, span_l, heat_l, map_l, out_l = (_as_list(v, n, k) for v, k in ((boxes, "boxes"), (span, "span"), (heat, "heat"), (frame_map, "frame_map"), (out, "out")))
    jobs, keep, results = [], [], []
    for c, b, s, h, m, o in zip(clips, boxes_l, span_l, heat_l, map_l, out_l):
        if not isinstance(c, DeviceFrames) or c.data.device != device:
            raise ValueError("frames: DeviceFrames on one device")
        b = _dev_tensor(b, torch.float32, (4,), "boxes", device)
        s = _dev_tensor(s, torch.int64, (2,), "span", device)
        h = _dev_tensor(h, torch.uint8, (), "heat", device)
        m = _dev_tensor(m, torch.int32, (c.T,), "frame_map", device)
        if b is not None and b.dim() != 2 or s is not None and s.dim() != 1 or m is not None and m.dim() != 1 or h is not None and h.dim() != 3:
            raise ValueError("boxes (n_tube, 4), span (2,), heat (n_tube, mh, mw), frame_map (T,)")
        if b is not None and h is not None and b.shape[0] != h.shape[0]:
            raise ValueError(f"boxes have {b.shape[0]} tube rows, heat has {h.shape[0]}")
        n_tube = b.shape[0] if b is not None else h.shape[0] if h is not None else 2 ** 31 - 1  # span only: no array that a row could index past
        if o is None:
            o = c.empty_like()
        elif not isinstance(o, DeviceFrames) or (o.T, o.h, o.w, o.pix_fmt) != (c.T, c.h, c.w, c.pix_fmt) or o.data.device != device:
            raise ValueError("out: DeviceFrames of the clip's geometry and pixel format on its device")
        space = (c.pix_fmt, c.matrix, c.full_range)
        jobs.append(overlay_job(c.data.data_ptr(), c.T, c.h, c.w, o.data.data_ptr(), c.pix_fmt, _hip.ptr(b), n_tube, _hip.ptr(s), _hip.ptr(m), _hip.ptr(h),
                                tuple(h.shape[1:]) if h is not None else (0, 0), color_in_space(style.box_color, *space), color_in_space(style.heat_color, *space),
                                color_in_space(style.dim_color, *space), style.thickness, style.heat_alpha, style.dim_alpha))
        keep.append((b, s, h, m))
        results.append(o)
    return _launch_pooled("td_tube_overlay", jobs, keep, results, single, device)


# ---- grounded tubes cropped out of decoded frames (td_tube_crop, csrc/tube_crop.hip) ----------------------------------------
MAX_CROP_SRC_COLS = 8192
MAX_CROP_SIDE = 4096
MAX_MARGIN_DEN = 1024


class TubeCrops(NamedTuple):
    """What ``crop_tubes`` returns for one clip: the crops in the uint8 video + mask layout of a staged batch."""
    pixels: torch.Tensor   # uint8 (T, 3, oh, ow): the resized window in the top-left rh x rw, zeros elsewhere
    mask: torch.Tensor     # bool (T, oh, ow): True on the padding
    valid: torch.Tensor    # bool (T,): False for a frame without a crop (outside the span, no tube row, a degenerate box)
    windows: torch.Tensor  # int32 (T, 6): (wy0, wx0, ch, cw, rh, rw) - source window and resized size; zeros when not valid


def _check_margin(num: int, den: int):
    if not 1 <= den <= MAX_MARGIN_DEN:
        raise ValueError(f"margin denominator {den}: 1..{MAX_MARGIN_DEN}")
    if not 0 <= num <= 4 * den:
        raise ValueError(f"margin {num}/{den}: between 0 and 4")


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
    from . import _hip

    T, sh, sw, n_tube = int(T), int(sh), int(sw), int(n_tube)
    _check_geometry(pix_fmt, T, sh, sw)
    if sw > MAX_CROP_SRC_COLS:
        raise ValueError(f"frame width {sw}: at most {MAX_CROP_SRC_COLS} for a crop (the window can be the whole row)")
    if matrix not in _MATRICES:
        raise ValueError(f"matrix {matrix!r}: one of {_MATRICES}")
    if n_tube < 1:
        raise ValueError(f"n_tube = {n_tube}: at least one tube row")
    if not boxes or not dst:
        raise ValueError("boxes and dst are device addresses, not None")
    oh, ow, num, den, keep = _crop_geometry(size, margin, keep_aspect)
    fmt, tight, sizes = _planes(pix_fmt, sh, sw)
    j = _hip.CropJob()
    (j.plane0, j.plane1, j.plane2), (j.pitch0, j.pitch1, j.pitch2), j.frame_stride = _describe(src, sizes, tight, planes, pitches, frame_stride)
    j.fmt, j.matrix, j.full_range = fmt, _MATRICES.index(matrix), int(bool(full_range))
    j.T, j.sh, j.sw = T, sh, sw
    j.boxes, j.span, j.frame_map, j.n_tube = boxes, span, frame_map, n_tube
    j.oh, j.ow, j.margin_num, j.margin_den, j.keep_aspect = oh, ow, num, den, keep
    j.dst, j.mask, j.valid, j.windows = dst, mask, valid, windows
    return j


def tube_crop(jobs: Sequence, device) -> tuple:
    """One td_tube_crop launch on the current stream with freshly allocated job tables; returns them: the caller keeps them
    alive until the stream has passed the launch (``crop_tubes`` recycles its own instead)."""
    return _launch_fresh("td_tube_crop", jobs, device)


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
    from . import _hip

    single = isinstance(frames, DeviceFrames)
    clips = [frames] if single else list(frames)
    n = len(clips)
    if n == 0:
        return []
    if not isinstance(clips[0], DeviceFrames):
        raise ValueError("frames: DeviceFrames on one device")
    device = clips[0].data.device
    oh, ow, num, den, keep = _crop_geometry(size, margin, keep_aspect)
    boxes_l, span_l, map_l = (_as_list(v, n, k) for v, k in ((boxes, "boxes"), (span, "span"), (frame_map, "frame_map")))
    jobs, keep_alive, results = [], [], []
    for c, b, s, m in zip(clips, boxes_l, span_l, map_l):
        if not isinstance(c, DeviceFrames) or c.data.device != device:
            raise ValueError("frames: DeviceFrames on one device")
        if b is None:
            raise ValueError("boxes: a torch.float32 tensor (n_tube, 4) per clip")
        b = _dev_tensor(b, torch.float32, (4,), "boxes", device)
        s = _dev_tensor(s, torch.int64, (2,), "span", device)
        m = _dev_tensor(m, torch.int32, (c.T,), "frame_map", device)
        if b.dim() != 2 or b.shape[0] < 1 or s is not None and s.dim() != 1 or m is not None and m.dim() != 1:
            raise ValueError("boxes (n_tube, 4) with n_tube >= 1, span (2,), frame_map (T,)")
        pixels = torch.empty((c.T, 3, oh, ow), dtype=torch.uint8, device=device)
        mask = torch.empty((c.T, oh, ow), dtype=torch.bool, device=device)
        valid = torch.empty((c.T,), dtype=torch.bool, device=device)
        windows = torch.empty((c.T, 6), dtype=torch.int32, device=device)
        jobs.append(crop_job(c.data.data_ptr(), c.T, c.h, c.w, b.data_ptr(), b.shape[0], pixels.data_ptr(), (oh, ow), c.pix_fmt, c.matrix, c.full_range,
                             _hip.ptr(s), _hip.ptr(m), (num, den), bool(keep), mask.data_ptr(), valid.data_ptr(), windows.data_ptr()))
        keep_alive.append((c.data, b, s, m))
        results.append(TubeCrops(pixels, mask, valid, windows))
    return _launch_pooled("td_tube_crop", jobs, keep_alive, results, single, device)


# ---- grounded tubes redacted in decoded frames (td_tube_redact, csrc/redact.hip) ---------------------------------------------
MAX_RECTS = 8
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
    from . import _hip

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
    _describe_src_dst(j, src, dst, sizes, tight, src_planes, src_pitches, src_frame_stride, dst_planes, dst_pitches, dst_frame_stride)
    j.fmt, j.T, j.sh, j.sw = fmt, T, sh, sw
    j.boxes, j.span, j.frame_map = boxes, span, frame_map
    j.n_tube, j.K, j.mode, j.invert = n_tube, K, code, inv
    j.margin_num, j.margin_den, j.cell, j.radius = num, den, cell, radius
    j.color[:] = _rgb3("color", color)
    return j


def tube_redact(jobs: Sequence, device) -> tuple:
    """One td_tube_redact launch on the current stream with freshly allocated job tables; returns them: the caller keeps
    them alive until the stream has passed the launch (``redact`` recycles its own instead)."""
    return _launch_fresh("td_tube_redact", jobs, device)


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
    from . import _hip

    single = isinstance(frames, DeviceFrames)
    clips = [frames] if single else list(frames)
    n = len(clips)
    if n == 0:
        return []
    if not isinstance(clips[0], DeviceFrames):
        raise ValueError("frames: DeviceFrames on one device")
    device = clips[0].data.device
    _redact_what(mode, cell, radius, margin, invert)
    color = _rgb3("color", color)
    boxes_l, span_l, map_l, out_l = (_as_list(v, n, k) for v, k in ((boxes, "boxes"), (span, "span"), (frame_map, "frame_map"), (out, "out")))
    prepared = []
    for c, b, s, m, o in zip(clips, boxes_l, span_l, map_l, out_l):  # every refusal comes before the first allocation and the launch
        if not isinstance(c, DeviceFrames) or c.data.device != device:
            raise ValueError("frames: DeviceFrames on one device")
        if b is None:
            raise ValueError("boxes: a torch.float32 tensor (n_tube, 4) or (n_tube, K, 4) per clip")
        b = _dev_tensor(b, torch.float32, (4,), "boxes", device)
        s = _dev_tensor(s, torch.int64, (2,), "span", device)
        m = _dev_tensor(m, torch.int32, (c.T,), "frame_map", device)
        if b.dim() not in (2, 3) or b.shape[0] < 1 or m is not None and m.dim() != 1:
            raise ValueError("boxes (n_tube, 4) or (n_tube, K, 4) with n_tube >= 1, frame_map (T,)")
        K = 1 if b.dim() == 2 else int(b.shape[1])
        if not 1 <= K <= MAX_RECTS:
            raise ValueError(f"boxes carry K = {K} rectangles per tube row: 1..{MAX_RECTS}")
        if s is not None and not (s.dim() == 1 and K == 1 or s.dim() == 2 and s.shape[0] == K):
            raise ValueError(f"span: (2,) for one tube, ({K}, 2) for {K}")
        if o is not None and (not isinstance(o, DeviceFrames) or (o.T, o.h, o.w, o.pix_fmt) != (c.T, c.h, c.w, c.pix_fmt) or o.data.device != device):
            raise ValueError("out: DeviceFrames of the clip's geometry and pixel format on its device")
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


# ---- grounded tubes interpolated to every decoded frame (td_tube_densify, csrc/tube_dense.hip) -------------------------------
DENSE_MODES = ("hold", "lerp", "hull")
MAX_SMOOTH = 16
MAX_DENSE_T = 1 << 20
MAX_FRAME_NO = 1 << 23
MAX_DENSE_STEP = 1 << 16


class DenseTubes(NamedTuple):
    """What ``densify`` returns for one clip: the tube at the decoded rate.  An absent box is four NaNs, which ``annotate``,
    ``crop_tubes`` and ``redact`` take as "no box": pass ``boxes`` (and ``heat``) with frame_map = None."""
    boxes: torch.Tensor           # fp32 (T, 4) or (T, K, 4)
    span: torch.Tensor            # int64 (2,) or (K, 2): first and last dense frame of the span (``annotate``'s dim layer)
    valid: torch.Tensor           # bool (T,) or (T, K): False where the box is absent or not finite
    heat: Optional[torch.Tensor]  # uint8 (T, mh, mw), or None


def _int_in(name: str, v, lo: int, hi: int) -> int:
    try:
        ok = not isinstance(v, bool) and int(v) == v and lo <= int(v) <= hi
    except (TypeError, ValueError):
        ok = False
    if not ok:
        raise ValueError(f"{name} = {v!r}: an integer in {lo}..{hi}")
    return int(v)


def _dense_what(T, t0, first, step, mode, smooth, has_table: bool):
    if mode not in DENSE_MODES:
        raise ValueError(f"mode {mode!r}: one of {DENSE_MODES}")
    T, t0 = _int_in("T", T, 0, MAX_DENSE_T), _int_in("t0", t0, -MAX_FRAME_NO, MAX_FRAME_NO)
    if has_table:
        first, step = 0, 1
    else:
        first, step = _int_in("first", first, -MAX_FRAME_NO, MAX_FRAME_NO), _int_in("step", step, 1, MAX_DENSE_STEP)
    return T, t0, first, step, DENSE_MODES.index(mode), _int_in("smooth", smooth, 0, MAX_SMOOTH)


def dense_job(boxes: int, n_tube: int, T: int, dense: int, K: int = 1, span: Optional[int] = None, row_frame: Optional[int] = None, first: int = 0, step: int = 1,
              t0: int = 0, heat: Optional[int] = None, heat_hw: Tuple[int, int] = (0, 0), mode: str = "lerp", smooth: int = 0, valid: Optional[int] = None,
              dense_span: Optional[int] = None, dense_heat: Optional[int] = None):
    """One ``td_dense_job``: the tube ``boxes`` (fp32 [n_tube][K][4]) sampled at the frame numbers ``row_frame`` (int32 [n_tube];
    None: row r at first + r step) interpolated to the T frames t0 .. t0 + T - 1 into ``dense`` (fp32 [T][K][4]).  ``span`` (int64
    [K][2]), ``heat`` (uint8 [n_tube][heat_hw[0]][heat_hw[1]]), ``valid`` (bytes [T][K]), ``dense_span`` (int64 [K][2]) and
    ``dense_heat`` (uint8 [T][mh][mw], with ``heat``) are device addresses or None."""
    from . import _hip

    n_tube, K = int(n_tube), int(K)
    T, t0, first, step, code, smooth = _dense_what(T, t0, first, step, mode, smooth, row_frame is not None)
    if n_tube < 1:
        raise ValueError(f"n_tube = {n_tube}: at least one tube row")
    if not 1 <= K <= MAX_RECTS:
        raise ValueError(f"K = {K}: 1..{MAX_RECTS} rectangles per tube row")
    if not boxes or not dense:
        raise ValueError("boxes and dense are device addresses, not None")
    if (heat is None) != (dense_heat is None):
        raise ValueError("heat and dense_heat come together")
    mh, mw = int(heat_hw[0]), int(heat_hw[1])
    if heat is not None and not (1 <= mh <= MAX_MAP and 1 <= mw <= MAX_MAP):
        raise ValueError(f"token grid {mh} x {mw}: sides in 1..{MAX_MAP}")
    j = _hip.DenseJob()
    j.boxes, j.span, j.row_frame, j.heat = boxes, span, row_frame, heat
    j.n_tube, j.K, j.T, j.t0, j.first, j.step, j.mode, j.smooth, j.mh, j.mw = n_tube, K, T, t0, first, step, code, smooth, mh, mw
    j.dense, j.valid, j.dense_span, j.dense_heat = dense, valid, dense_span, dense_heat
    return j


def tube_densify(jobs: Sequence, device) -> tuple:
    """One td_tube_densify launch on the current stream with freshly allocated job tables; returns them: the caller keeps
    them alive until the stream has passed the launch (``densify`` recycles its own instead)."""
    return _launch_fresh("td_tube_densify", jobs, device)


def tube_densify_shots(jobs: Sequence, shots: Optional[Sequence], device) -> tuple:
    """One td_tube_densify_shots launch, as ``tube_densify``; ``shots`` holds one ``_hip.DenseShots`` per job, or is None."""
    from . import _hip

    nb = int(_hip.lib().td_tube_densify_shots_table_bytes(len(jobs)))
    host = torch.empty(max(nb, 256), dtype=torch.uint8, pin_memory=True)
    dev = torch.empty(max(nb, 256), dtype=torch.uint8, device=device)
    arr = (_hip.DenseJob * len(jobs))(*jobs)
    sarr = (_hip.DenseShots * len(jobs))(*shots) if shots is not None else None
    _hip.check(_hip.lib().td_tube_densify_shots(arr, sarr, len(jobs), host.data_ptr(), dev.data_ptr(), nb, _hip.stream_ptr()), "td_tube_densify_shots")
    return host, dev


def _per_clip(v, n: int, name: str, multi: bool):
    """A scalar serves every clip; with a list of clips, a list or tuple gives one value each."""
    if multi and isinstance(v, (list, tuple)):
        if len(v) != n:
            raise ValueError(f"{name}: {len(v)} entries for {n} clips")
        return list(v)
    return [v] * n


def densify(boxes, T, row_frame=None, first=0, step=1, t0=0, span=None, heat=None, mode: str = "lerp", smooth=0, shots=None, shots_t0=0):
    """Interpolate grounded tubes from the sampled frames to every decoded frame: ONE launch for one clip or for a list of
    clips (``boxes`` a list: ``row_frame``, ``span`` and ``heat`` are then lists too, or None, and ``T``, ``first``, ``step``,
    ``t0``, ``mode`` and ``smooth`` may be lists or one value for all).  Per clip:
      boxes      fp32 (n_tube, 4) or (n_tube, K, 4) xyxy on the device: what ``PostProcess`` returned, one row per sampled frame;
      T, t0      dense frame i of T has frame number t0 + i (a long video is done in chunks);
      row_frame  the frame number of every tube row, increasing: an int32 (n_tube,) tensor on the device, or a host sequence of
                 integers (uploaded with the job table, asynchronously); None: row r was sampled at first + r * step;
      span       int64 (2,) or (K, 2) tube rows, as ``redact`` takes them; None: all rows;
      heat       uint8 (n_tube, mh, mw) from ``heat_from_attention``; None: no maps;
      mode       "hold" (what a frame_map does), "lerp" (straight lines between two rows) or "hull" (the cover of both rows: for ``redact``);
      smooth     a radius in tube rows, 0..16: every row becomes the mean of the present rows around it first;
      shots      what ``shot_cuts`` returned for the clip (a ``Shots``), or its int32 (n,) shot id per frame on the device, entry i
                 for frame number ``shots_t0`` + i (a list of either, or of None, for a list of clips): the tube stops at the
                 cuts (``td_tube_densify_shots``) - no box is interpolated, smoothed or covered across one, the row on the frame's
                 own side of a cut stands alone.  Frames outside the array match every shot, so every chunk of a long video takes
                 the whole video's array.  None: the call is what it was.
    The rule is exact - numpy float32 reproduces every bit - and stated in include/tubedetr_hip.h.  Returns ``DenseTubes`` (a
    list for a list), whose boxes, span and heat go to ``annotate`` / ``crop_tubes`` / ``redact`` with frame_map = None.  Nothing
    here synchronises or copies to the host, and bad arguments are refused before the device is touched."""
    from . import _hip

    multi = isinstance(boxes, (list, tuple))
    clips = list(boxes) if multi else [boxes]
    n = len(clips)
    if n == 0:
        return []
    if multi:
        frames_l, span_l, heat_l = (_as_list(v, n, k) for v, k in ((row_frame, "row_frame"), (span, "span"), (heat, "heat")))
    else:
        frames_l, span_l, heat_l = [row_frame], [span], [heat]
    scalars = [_per_clip(v, n, k, multi) for v, k in ((T, "T"), (t0, "t0"), (first, "first"), (step, "step"), (mode, "mode"), (smooth, "smooth"))]
    if shots is None:
        shots_l = None
    else:
        shots_l = _as_list(shots, n, "shots") if multi else [shots]
        shots_l = [sh.shot if isinstance(sh, Shots) else sh for sh in shots_l]
        shots_t0_l = [_int_in("shots_t0", v, -MAX_FRAME_NO, MAX_FRAME_NO) for v in _per_clip(shots_t0, n, "shots_t0", multi)]
    if not torch.is_tensor(clips[0]) or not clips[0].is_cuda:
        # the scalars' refusals do not need a device: give them first, so that they are the same on a host without one
        for i in range(n):
            _dense_what(*(s[i] for s in scalars), has_table=frames_l[i] is not None)
        raise ValueError("boxes: a torch.float32 tensor (n_tube, 4) or (n_tube, K, 4) on the device per clip")
    device = clips[0].device
    prepared, tail = [], 0
    for i, (b, f, s, h) in enumerate(zip(clips, frames_l, span_l, heat_l)):  # every refusal comes before the first allocation and the launch
        Ti, t0i, firsti, stepi, _, smoothi = _dense_what(*(sc[i] for sc in scalars), has_table=f is not None)
        b = _dev_tensor(b, torch.float32, (4,), "boxes", device)
        s = _dev_tensor(s, torch.int64, (2,), "span", device)
        h = _dev_tensor(h, torch.uint8, (), "heat", device)
        if b is None or b.dim() not in (2, 3) or b.shape[0] < 1:
            raise ValueError("boxes (n_tube, 4) or (n_tube, K, 4) with n_tube >= 1")
        n_tube, K = int(b.shape[0]), 1 if b.dim() == 2 else int(b.shape[1])
        if not 1 <= K <= MAX_RECTS:
            raise ValueError(f"boxes carry K = {K} rectangles per tube row: 1..{MAX_RECTS}")
        if s is not None and not (s.dim() == 1 and K == 1 or s.dim() == 2 and s.shape[0] == K):
            raise ValueError(f"span: (2,) for one tube, ({K}, 2) for {K}")
        if h is not None and (h.dim() != 3 or h.shape[0] != n_tube or not (1 <= h.shape[1] <= MAX_MAP and 1 <= h.shape[2] <= MAX_MAP)):
            raise ValueError(f"heat: uint8 ({n_tube}, mh, mw) with mh and mw in 1..{MAX_MAP}")
        off = None
        if torch.is_tensor(f):
            f = _dev_tensor(f, torch.int32, (n_tube,), "row_frame", device)
            if f.dim() != 1:
                raise ValueError(f"row_frame: int32 ({n_tube},)")
        elif f is not None:
            f = [_int_in("row_frame entry", v, -MAX_FRAME_NO, MAX_FRAME_NO) for v in f]
            if len(f) != n_tube:
                raise ValueError(f"row_frame has {len(f)} entries for {n_tube} tube rows")
            off, tail = tail, tail + (4 * n_tube + 15) // 16 * 16
        if shots_l is not None and shots_l[i] is not None:
            sh = shots_l[i] = _dev_tensor(shots_l[i], torch.int32, (), "shots", device)
            if sh.dim() != 1 or sh.numel() > MAX_DENSE_T:
                raise ValueError(f"shots: a Shots, or an int32 (n,) tensor of shot ids with n <= {MAX_DENSE_T}")
        prepared.append((b, f, s, h, off, n_tube, K, Ti, i))
    jobs, keep, results, uploads = [], [], [], []
    for b, f, s, h, off, n_tube, K, Ti, i in prepared:
        dense = torch.empty(max(Ti, 1) * K * 4, dtype=torch.float32, device=device)[:Ti * K * 4]  # (T = 0 still has an address)
        valid = torch.empty(max(Ti, 1) * K, dtype=torch.bool, device=device)[:Ti * K]
        dspan = torch.empty((K, 2), dtype=torch.int64, device=device)
        dheat = None
        if h is not None:
            mb = int(h.shape[1] * h.shape[2])
            dheat = torch.empty(max(Ti, 1) * mb, dtype=torch.uint8, device=device)[:Ti * mb]
        table = f if torch.is_tensor(f) else None
        j = dense_job(b.data_ptr(), n_tube, Ti, dense.data_ptr(), K, _hip.ptr(s), _hip.ptr(table), scalars[2][i], scalars[3][i], scalars[1][i], _hip.ptr(h),
                      tuple(h.shape[1:]) if h is not None else (0, 0), scalars[4][i], scalars[5][i], valid.data_ptr(), dspan.data_ptr(), _hip.ptr(dheat))
        if off is not None:
            uploads.append((j, off, f))
        jobs.append(j)
        keep.append((b, s, h, table, shots_l[i] if shots_l is not None else None))
        one = b.dim() == 2
        results.append(DenseTubes(dense.view(Ti, 4) if one else dense.view(Ti, K, 4), dspan.view(2) if one else dspan, valid.view(Ti) if one else valid.view(Ti, K),
                                  dheat.view(Ti, h.shape[1], h.shape[2]) if h is not None else None))

    def fill_tail(host_tail, dev_tail):
        for j, off, values in uploads:
            host_tail[off:off + 4 * len(values)].view(torch.int32).copy_(torch.tensor(values, dtype=torch.int32))
            j.row_frame = dev_tail.data_ptr() + off
        dev_tail.copy_(host_tail, non_blocking=True)

    if shots_l is None:
        return _launch_pooled("td_tube_densify", jobs, keep, results, not multi, device, tail, fill_tail)

    def enqueue(host, dev, nbytes):
        arr = (_hip.DenseJob * n)(*jobs)
        sarr = (_hip.DenseShots * n)(*[_hip.DenseShots(_hip.ptr(sh), t, sh.numel() if sh is not None else 0) for sh, t in zip(shots_l, shots_t0_l)])
        _hip.check(_hip.lib().td_tube_densify_shots(arr, sarr, n, host.data_ptr(), dev.data_ptr(), nbytes, _hip.stream_ptr()), "td_tube_densify_shots")

    return _launch_pooled("td_tube_densify", jobs, keep, results, not multi, device, tail, fill_tail, enqueue)


# ---- shot cuts in decoded frames (td_frame_stats, td_shot_cuts, csrc/frame_stats.hip) -----------------------------------------
STAT_BINS = 64
MAX_STAT_STEP = 8
MAX_STAT_PIXELS = 1 << 24
MAX_CUT_T = 1 << 20
MAX_CUT_WINDOW = 16
MAX_CUT_FRACTION = 1 << 20


class FrameStats(NamedTuple):
    """What ``frame_stats`` returns for one clip."""
    hist: torch.Tensor  # int32 (T, 64) holding the uint32 counts: sampled pixels of frame t with luma >> 2 == b
    sad: torch.Tensor   # int32 (T,) holding the uint32 sums: |luma_t - luma_(t-1)| over the sampled pixels; 0 for frame 0, and for a repeated frame
    n: int              # sampled pixels per frame


class Shots(NamedTuple):
    """What ``shot_cuts`` returns for one clip; ``densify(..., shots=...)`` takes it."""
    cut: torch.Tensor    # bool (T,): frame t is the first of a new shot
    shot: torch.Tensor   # int32 (T,): the shot of frame t, counted from 0
    count: torch.Tensor  # int32 (1,) on the device: the number of shots
    d: torch.Tensor      # int32 (T,) holding uint32: the histogram distance to the frame before


def sampled_pixels(sh: int, sw: int, step: int = 1) -> int:
    """N of td_frame_stats: the pixels (y, x) with y % step == 0 and x % step == 0."""
    return ((sh + step - 1) // step) * ((sw + step - 1) // step)


def _stats_what(sh, sw, step):
    step = _int_in("step", step, 1, MAX_STAT_STEP)
    if sh * sw > MAX_STAT_PIXELS:
        raise ValueError(f"frame size {sh} x {sw}: at most {MAX_STAT_PIXELS} pixels (the sum of differences is 32 bits wide)")
    return step


def stats_job(src: int, T: int, sh: int, sw: int, pix_fmt: str = "rgb24", step: int = 1, hist: Optional[int] = None, sad: Optional[int] = None,
              src_planes: Optional[Sequence[int]] = None, src_pitches: Optional[Sequence[int]] = None, src_frame_stride: Optional[int] = None):
    """One ``td_stats_job``: T frames of sh x sw in ``pix_fmt`` at device address ``src`` (planes, pitches and frame stride as in
    ``overlay_job``), every ``step``-th pixel of every ``step``-th row; ``hist`` (uint32 [T][64]) and ``sad`` (uint32 [T]) are
    device addresses, one of them may be None."""
    from . import _hip

    T, sh, sw = int(T), int(sh), int(sw)
    _check_geometry(pix_fmt, T, sh, sw)
    step = _stats_what(sh, sw, step)
    if not hist and not sad:
        raise ValueError("hist and sad are device addresses: at least one of them")
    fmt, tight, sizes = _planes(pix_fmt, sh, sw)
    j = _hip.StatsJob()
    (j.src0, j.src1, j.src2), (j.src_pitch0, j.src_pitch1, j.src_pitch2), j.src_frame_stride = _describe(src, sizes, tight, src_planes, src_pitches, src_frame_stride)
    j.fmt, j.T, j.sh, j.sw, j.step = fmt, T, sh, sw, step
    j.hist, j.sad = hist, sad
    return j


def _fraction(name: str, v) -> Tuple[int, int]:
    try:
        num, den = v
    except (TypeError, ValueError):
        raise ValueError(f"{name} {v!r}: two integers (numerator, denominator)") from None
    return _int_in(name + " numerator", num, 0, MAX_CUT_FRACTION), _int_in(name + " denominator", den, 1, MAX_CUT_FRACTION)


def _cuts_what(hist, sad, peak, window):
    return _fraction("hist", hist) + _fraction("sad", sad) + _fraction("peak", peak) + (_int_in("window", window, 0, MAX_CUT_WINDOW),)


def cuts_job(hist: int, sad: int, T: int, n: int, cut: int, shot: int, n_shots: int, d: Optional[int] = None, hist_thr=(1, 4), sad_thr=(8, 1), peak=(3, 1),
             window: int = 4):
    """One ``td_cuts_job``: the statistics ``hist`` (uint32 [T][64]) and ``sad`` (uint32 [T]) of T frames of ``n`` sampled pixels
    decided into ``cut`` (bytes [T]), ``shot`` (int32 [T]), ``n_shots`` (int32 [1]) and, optionally, ``d`` (uint32 [T]): device
    addresses.  The thresholds are (numerator, denominator) pairs, ``window`` the peak test's radius in frames."""
    from . import _hip

    T, n = _int_in("T", T, 0, MAX_CUT_T), _int_in("n", n, 1, MAX_STAT_PIXELS)
    what = _cuts_what(hist_thr, sad_thr, peak, window)
    if not (hist and sad and cut and shot and n_shots):
        raise ValueError("hist, sad, cut, shot and n_shots are device addresses, not None")
    j = _hip.CutsJob()
    j.hist, j.sad, j.T, j.N = hist, sad, T, n
    j.hist_num, j.hist_den, j.sad_num, j.sad_den, j.peak_num, j.peak_den, j.w = what
    j.d, j.cut, j.shot, j.n_shots = d, cut, shot, n_shots
    return j


def launch_frame_stats(jobs: Sequence, device) -> tuple:
    """One td_frame_stats launch on the current stream with freshly allocated job tables; returns them: the caller keeps them
    alive until the stream has passed the launch (``frame_stats`` recycles its own instead)."""
    return _launch_fresh("td_frame_stats", jobs, device)


def launch_shot_cuts(jobs: Sequence, device) -> tuple:
    """One td_shot_cuts launch, as ``launch_frame_stats``."""
    return _launch_fresh("td_shot_cuts", jobs, device)


def frame_stats(frames: Union[DeviceFrames, Sequence[DeviceFrames]], step: int = 1):
    """A luma histogram per frame and the sum of absolute luma differences to the frame before, read from the decoded planes in
    ONE launch for one clip or for a list of clips (mixed sizes and formats).  ``step`` in 1..8 takes every ``step``-th pixel of
    every ``step``-th row, and the bytes read fall with it.  The rule is integers and stated in include/tubedetr_hip.h; a long
    video done in chunks overlaps them by one frame.  Returns ``FrameStats`` (a list for a list).  Nothing here synchronises or
    copies to the host, and bad arguments are refused before the device is touched."""
    single = isinstance(frames, DeviceFrames)
    clips = [frames] if single else list(frames)
    if len(clips) == 0:
        return []
    if not isinstance(clips[0], DeviceFrames):
        raise ValueError("frames: DeviceFrames on one device")
    device = clips[0].data.device
    for c in clips:  # every refusal comes before the first allocation and the launch
        if not isinstance(c, DeviceFrames) or c.data.device != device:
            raise ValueError("frames: DeviceFrames on one device")
        _stats_what(c.h, c.w, step)
    jobs, keep, results = [], [], []
    for c in clips:
        out = torch.empty(max(c.T, 1) * (STAT_BINS + 1), dtype=torch.int32, device=device)  # (T = 0 still has an address)
        hist, sad = out[:c.T * STAT_BINS], out[c.T * STAT_BINS:c.T * (STAT_BINS + 1)]
        if c.T > 0:  # (a clip without frames has no bytes, and its tensor no address: it is no job)
            jobs.append(stats_job(c.data.data_ptr(), c.T, c.h, c.w, c.pix_fmt, step, out.data_ptr(), out.data_ptr() + 4 * c.T * STAT_BINS))
            keep.append((c.data,))
        results.append(FrameStats(hist.view(c.T, STAT_BINS), sad, sampled_pixels(c.h, c.w, step)))
    if not jobs:
        return results[0] if single else results
    return _launch_pooled("td_frame_stats", jobs, keep, results, single, device)


def shot_cuts(frames_or_stats, step: int = 1, hist=(1, 4), sad=(8, 1), peak=(3, 1), window: int = 4):
    """Where the hard cuts of decoded clips are: ``frames_or_stats`` is a ``DeviceFrames`` (``frame_stats`` with ``step`` runs
    first), a ``FrameStats``, or a list of either kind.  Frame t starts a new shot when its histogram distance d[t] to the frame
    before exceeds ``hist`` = (num, den) of its maximum 2 n, its sum of differences exceeds ``sad`` = (num, den) grey levels per
    sampled pixel, and d[t] is the first largest value within ``window`` frames and more than ``peak`` = (num, den) times the
    mean of the others there - the rule, in integers, is stated in include/tubedetr_hip.h.  A one-frame flash gives one cut, at
    its first frame; fades and wipes give none.  The defaults are starting values tried on synthetic clips only: no footage has
    validated them.  Returns ``Shots`` (a list for a list); nothing synchronises, ``Shots.count`` stays on the device."""
    single = isinstance(frames_or_stats, (DeviceFrames, FrameStats))
    items = [frames_or_stats] if single else list(frames_or_stats)
    if len(items) == 0:
        return []
    _cuts_what(hist, sad, peak, window)
    if all(isinstance(v, DeviceFrames) for v in items):
        _int_in("step", step, 1, MAX_STAT_STEP)
        items = frame_stats(items, step)
    prepared = []
    for v in items:  # every refusal comes before the first allocation and the launch
        if not isinstance(v, FrameStats):
            raise ValueError("frames_or_stats: DeviceFrames or FrameStats, one kind per call")
        h, s = v.hist, v.sad
        if not (torch.is_tensor(h) and torch.is_tensor(s) and h.is_cuda and s.device == h.device and h.dtype == torch.int32 and s.dtype == torch.int32
                and h.dim() == 2 and h.shape[1] == STAT_BINS and s.dim() == 1 and s.shape[0] == h.shape[0]):
            raise ValueError(f"FrameStats: hist int32 (T, {STAT_BINS}) and sad int32 (T,) on the device")
        if h.device != items[0].hist.device:
            raise ValueError("frames_or_stats: statistics on one device")
        prepared.append((h.contiguous(), s.contiguous(), _int_in("T", h.shape[0], 0, MAX_CUT_T), _int_in("FrameStats.n", v.n, 1, MAX_STAT_PIXELS)))
    device = prepared[0][0].device
    jobs, keep, results = [], [], []
    for h, s, T, n in prepared:
        words = torch.empty(2 * max(T, 1) + 1, dtype=torch.int32, device=device)
        flags = torch.empty(max(T, 1), dtype=torch.bool, device=device)
        d, shot, count = words[:T], words[max(T, 1):max(T, 1) + T], words[2 * max(T, 1):]
        # (a tensor without elements has no address: T = 0 still hands addresses over, and none of them is read or written but n_shots)
        jobs.append(cuts_job(h.data_ptr() or words.data_ptr(), s.data_ptr() or words.data_ptr(), T, n, flags.data_ptr(), words.data_ptr() + 4 * max(T, 1),
                             words.data_ptr() + 8 * max(T, 1), words.data_ptr(), hist, sad, peak, window))
        keep.append((h, s))
        results.append(Shots(flags[:T], shot, count, d))
    return _launch_pooled("td_shot_cuts", jobs, keep, results, single, device)


# ---- boxes that follow the object's pixels between sampled frames (td_tube_follow, csrc/tube_follow.hip) ---------------------
MAX_FOLLOW_RADIUS = 16
MAX_FOLLOW_REACH = 64
MAX_FOLLOW_ACCEPT = 1 << 20


class FollowedTubes(NamedTuple):
    """What ``follow`` returns for one clip; ``boxes`` go to ``annotate`` / ``annotate_tubes`` / ``crop_tubes`` / ``redact`` with
    frame_map = None."""
    boxes: torch.Tensor   # fp32 (T, 4) or (T, K, 4): the input's boxes, the accepted ones moved by their offset
    offset: torch.Tensor  # int32 (T, 2) or (T, K, 2): (dy, dx); (0, 0) where the box was copied or the match rejected
    cost: torch.Tensor    # int32 (T,) or (T, K) holding uint32: the best candidate's sum of 256 absolute luma differences
    status: torch.Tensor  # uint8 (T,) or (T, K): 0 copied, 1 accepted, 2 rejected


def _accept(v) -> Tuple[int, int]:
    """``accept`` of ``follow``: grey levels per sample, an integer or a (numerator, denominator) pair."""
    if isinstance(v, (tuple, list)):
        try:
            num, den = v
        except (TypeError, ValueError):
            raise ValueError(f"accept {v!r}: an integer, or two integers (numerator, denominator)") from None
    else:
        num, den = v, 1
    return _int_in("accept numerator", num, 0, MAX_FOLLOW_ACCEPT), _int_in("accept denominator", den, 1, MAX_FOLLOW_ACCEPT)


def _follow_what(radius, reach, accept):
    return (_int_in("radius", radius, 0, MAX_FOLLOW_RADIUS), _int_in("reach", reach, 1, MAX_FOLLOW_REACH)) + _accept(accept)


def follow_job(src: int, T: int, sh: int, sw: int, boxes: int, anchor: int, out: int, K: int = 1, pix_fmt: str = "rgb24", shot: Optional[int] = None, radius: int = 8,
               reach: int = 3, accept=24, offset: Optional[int] = None, cost: Optional[int] = None, status: Optional[int] = None,
               src_planes: Optional[Sequence[int]] = None, src_pitches: Optional[Sequence[int]] = None, src_frame_stride: Optional[int] = None):
    """One ``td_follow_job``: T frames of sh x sw in ``pix_fmt`` at device address ``src`` (planes, pitches and frame stride as in
    ``overlay_job``); ``boxes`` (fp32 [T][K][4]), ``anchor`` (bytes [T]) and ``out`` (fp32 [T][K][4]; may be ``boxes``) are device
    addresses, ``shot`` (int32 [T]), ``offset`` (int32 [T][K][2]), ``cost`` (uint32 [T][K]) and ``status`` (bytes [T][K]) device
    addresses or None.  ``accept`` is an integer or a (numerator, denominator) pair."""
    from . import _hip

    T, sh, sw, K = int(T), int(sh), int(sw), int(K)
    _check_geometry(pix_fmt, T, sh, sw)
    radius, reach, num, den = _follow_what(radius, reach, accept)
    if not 1 <= K <= MAX_RECTS:
        raise ValueError(f"K = {K}: 1..{MAX_RECTS} rectangles per frame")
    if not boxes or not anchor or not out:
        raise ValueError("boxes, anchor and out are device addresses, not None")
    fmt, tight, sizes = _planes(pix_fmt, sh, sw)
    j = _hip.FollowJob()
    (j.src0, j.src1, j.src2), (j.src_pitch0, j.src_pitch1, j.src_pitch2), j.src_frame_stride = _describe(src, sizes, tight, src_planes, src_pitches, src_frame_stride)
    j.fmt, j.T, j.sh, j.sw, j.K = fmt, T, sh, sw, K
    j.boxes, j.anchor, j.shot = boxes, anchor, shot
    j.radius, j.reach, j.accept_num, j.accept_den = radius, reach, num, den
    j.out, j.offset, j.cost, j.status = out, offset, cost, status
    return j


def tube_follow(jobs: Sequence, device) -> tuple:
    """One td_tube_follow launch on the current stream with freshly allocated job tables; returns them: the caller keeps them
    alive until the stream has passed the launch (``follow`` recycles its own instead)."""
    return _launch_fresh("td_tube_follow", jobs, device)


def anchors(row_frame=None, first: int = 0, step: int = 1, T: Optional[int] = None, t0: int = 0, n_tube: Optional[int] = None, device=None) -> torch.Tensor:
    """The ``anchor`` vector of ``follow`` for the T dense frames t0 .. t0 + T - 1, uint8 (T,) on the device: 1 where the frame is
    a sampled one, whose boxes are the model's own.  The arguments are ``densify``'s: ``row_frame`` holds the frame number of every
    tube row (an int32 tensor on the device, or a host sequence of integers); None: row r was sampled at first + r * step, for
    r >= 0 (and r < ``n_tube``, when given).  A few torch operators, no synchronisation with a device table: this is not on the
    hot path - a caller with a fixed sampling pattern builds the vector once and keeps it."""
    T, t0 = _int_in("T", T, 0, MAX_DENSE_T), _int_in("t0", t0, -MAX_FRAME_NO, MAX_FRAME_NO)
    if row_frame is None:
        first, step = _int_in("first", first, -MAX_FRAME_NO, MAX_FRAME_NO), _int_in("step", step, 1, MAX_DENSE_STEP)
        if n_tube is not None:
            n_tube = _int_in("n_tube", n_tube, 1, MAX_DENSE_T)
    elif not torch.is_tensor(row_frame):
        row_frame = [_int_in("row_frame entry", v, -MAX_FRAME_NO, MAX_FRAME_NO) for v in row_frame]
    elif row_frame.dtype != torch.int32 or row_frame.dim() != 1 or not row_frame.is_cuda:
        raise ValueError("row_frame: an int32 (n_tube,) tensor on the device, or a host sequence of integers")
    if torch.is_tensor(row_frame):
        device = row_frame.device
    elif device is None:
        device = torch.device("cuda", torch.cuda.current_device())
    if row_frame is None:
        r = torch.arange(t0 - first, t0 - first + T, device=device)
        a = (r >= 0) & (r % step == 0)
        if n_tube is not None:
            a &= r < n_tube * step
        return a.to(torch.uint8)
    if not torch.is_tensor(row_frame):
        row_frame = torch.tensor(row_frame, dtype=torch.int32, device=device)
    i = row_frame.long() - t0
    a = torch.zeros(T + 1, dtype=torch.uint8, device=device)  # entry T takes the rows outside the T frames
    a[torch.where((i >= 0) & (i < T), i, torch.full_like(i, T))] = 1
    return a[:T]


def follow(frames: Union[DeviceFrames, Sequence[DeviceFrames]], boxes, anchor, shots=None, radius=8, reach=3, accept=24, in_place: bool = False):
    """Move the boxes of the frames between two sampled ones onto the object they belong to, by block matching in the decoded
    frames' luma: ONE launch for one clip or for a list of clips (``boxes``, ``anchor`` and ``shots`` are then lists too;
    ``radius``, ``reach`` and ``accept`` may be lists or one value for all).  Per clip:
      boxes    fp32 (T, 4) or (T, K, 4) xyxy on the device, one row per decoded frame, or the ``DenseTubes`` that ``densify``
               returned (four NaNs: no box);
      anchor   uint8 or bool (T,) on the device: non-zero where the frame's boxes are the model's own (``anchors`` makes it);
      shots    what ``shot_cuts`` returned for the clip (a ``Shots``) or its int32 (T,) tensor: no frame is matched against an
               anchor in another shot; None: one shot;
      radius   0..16 pixels searched around the interpolated position; reach 1..64 frames searched for an anchor;
      accept   the largest mean absolute luma difference per sample, in grey levels, at which a match moves the box: an integer
               or a (numerator, denominator) pair.  24 is a starting value that nobody has tried on real footage;
      in_place write into ``boxes`` (a contiguous tensor) instead of a new one: anchor boxes are never changed.
    A frame is matched against the nearest anchor frame (never against its neighbour: nothing drifts), translation only, on a
    16 x 16 grid of samples inside the anchor box; a rejected match leaves the interpolated box.  The rule is integers and stated in
    include/tubedetr_hip.h.  Returns ``FollowedTubes`` (a list for a list), whose boxes go to ``annotate`` / ``annotate_tubes`` /
    ``crop_tubes`` / ``redact`` with frame_map = None.  Nothing here synchronises or copies to the host, and bad arguments are
    refused before the device is touched."""
    from . import _hip

    single = isinstance(frames, DeviceFrames) or not isinstance(frames, (list, tuple))
    clips = [frames] if single else list(frames)
    n = len(clips)
    if n == 0:
        return []
    # (a tuple is ONE accept value, the pair: only a list, for a list of clips, gives one value each)
    accept_l = _per_clip(accept, n, "accept", not single and isinstance(accept, list))
    what = [_follow_what(*v) for v in zip(_per_clip(radius, n, "radius", not single), _per_clip(reach, n, "reach", not single), accept_l)]
    if not isinstance(clips[0], DeviceFrames):  # (the scalars' refusals came first: they are the same on a host without a device)
        raise ValueError("frames: DeviceFrames on one device")
    device = clips[0].data.device
    # (a DenseTubes and a Shots are tuples themselves: one clip takes them as they are)
    boxes_l, anchor_l, shots_l = ([boxes], [anchor], [shots]) if single else (_as_list(v, n, k) for v, k in ((boxes, "boxes"), (anchor, "anchor"), (shots, "shots")))
    prepared = []
    for c, b, a, s in zip(clips, boxes_l, anchor_l, shots_l):  # every refusal comes before the first allocation and the launch
        if not isinstance(c, DeviceFrames) or c.data.device != device:
            raise ValueError("frames: DeviceFrames on one device")
        given = b.boxes if isinstance(b, DenseTubes) else b
        b = _dev_tensor(given, torch.float32, (4,), "boxes", device)
        if b is None or b.dim() not in (2, 3) or b.shape[0] != c.T:
            raise ValueError(f"boxes: ({c.T}, 4) or ({c.T}, K, 4), one row per frame of the clip")
        K = 1 if b.dim() == 2 else int(b.shape[1])
        if not 1 <= K <= MAX_RECTS:
            raise ValueError(f"boxes carry K = {K} rectangles per frame: 1..{MAX_RECTS}")
        if in_place and b is not given:
            raise ValueError("in_place: boxes must be a contiguous tensor")
        if torch.is_tensor(a) and a.dtype == torch.bool:
            a = a.view(torch.uint8)
        a = _dev_tensor(a, torch.uint8, (c.T,), "anchor", device)
        if a is None or a.dim() != 1:
            raise ValueError(f"anchor: a uint8 or bool ({c.T},) tensor on the device")
        s = _dev_tensor(s.shot if isinstance(s, Shots) else s, torch.int32, (c.T,), "shots", device)
        if s is not None and s.dim() != 1:
            raise ValueError(f"shots: a Shots, or an int32 ({c.T},) tensor of shot ids")
        prepared.append((c, b, a, s, K))
    jobs, keep, results = [], [], []
    for (c, b, a, s, K), (radius_i, reach_i, num, den) in zip(prepared, what):
        T = c.T
        out = b if in_place else torch.empty_like(b)
        words = torch.empty(max(T, 1) * K * 3, dtype=torch.int32, device=device)  # (T = 0 still has an address)
        status = torch.empty(max(T, 1) * K, dtype=torch.uint8, device=device)
        if T > 0:  # (a clip without frames has no bytes, and its tensors no address: it is no job)
            jobs.append(follow_job(c.data.data_ptr(), T, c.h, c.w, b.data_ptr(), a.data_ptr(), out.data_ptr(), K, c.pix_fmt, _hip.ptr(s), radius_i, reach_i, (num, den),
                                   words.data_ptr(), words.data_ptr() + 8 * T * K, status.data_ptr()))
            keep.append((c.data, b, a, s))
        one = b.dim() == 2
        results.append(FollowedTubes(out, words[:2 * T * K].view((T, 2) if one else (T, K, 2)), words[2 * T * K:3 * T * K].view((T,) if one else (T, K)),
                                     status[:T * K].view((T,) if one else (T, K))))
    if not jobs:
        return results[0] if single else results
    return _launch_pooled("td_tube_follow", jobs, keep, results, single, device)


# ---- K labelled tubes and a moment timeline in one pass (td_tube_overlay_multi, csrc/overlay_multi.hip) -----------------------
MAX_TAG_H, MAX_TAG_W, MAX_TAG_SCALE, MAX_LANE_H, MAX_TIMELINE_ROWS = 32, 256, 8, 64, 1 << 20
PALETTE = ((0xFA, 0xFF, 0x00), (0x00, 0xC8, 0xFF), (0xFF, 0x5A, 0x5A), (0x5A, 0xFF, 0x7D), (0xFF, 0x8C, 0x00), (0xC8, 0x78, 0xFF), (0xFF, 0x78, 0xC8), (0x00, 0xA0, 0x8C))


@dataclass(frozen=True)
class TubeSetStyle:
    """How the K <= 8 tubes of a clip are drawn by ``annotate_tubes``; colours are RGB whatever the frames' pixel format.
    ``colors[k]`` is tube k's outline, tag plate and timeline segment.  The defaults draw outlines and (when ``annotate_tubes``
    is given tags) labels; ``lane_h`` > 0 adds the timeline: K lanes of lane_h rows at the bottom of the frame."""
    colors: Tuple[Tuple[int, int, int], ...] = PALETTE
    thickness: int = 2
    heat_color: Tuple[int, int, int] = (255, 0, 0)
    heat_alpha: int = 0       # of 256, at an attention level of 255
    dim_color: Tuple[int, int, int] = (0, 0, 0)
    dim_alpha: int = 0        # of 256, on the frames outside every span
    tag_text_color: Tuple[int, int, int] = (0, 0, 0)
    tag_alpha: int = 224      # of 256: the plate under a label, in the tube's colour
    tag_scale: int = 2        # frame pixels per bitmap sample
    lane_h: int = 0           # rows per tube of the timeline; 0: none
    bar_color: Tuple[int, int, int] = (32, 32, 32)
    bar_alpha: int = 160
    seg_alpha: int = 256
    cursor_color: Tuple[int, int, int] = (255, 255, 255)

    def __post_init__(self):
        colors = tuple(self.colors)
        if len(colors) != MAX_RECTS:
            raise ValueError(f"colors: {MAX_RECTS} RGB colours, not {len(colors)}")
        object.__setattr__(self, "colors", tuple(_rgb3(f"colors[{k}]", c) for k, c in enumerate(colors)))
        for n in ("heat_color", "dim_color", "tag_text_color", "bar_color", "cursor_color"):
            object.__setattr__(self, n, _rgb3(n, getattr(self, n)))
        for n in ("heat_alpha", "dim_alpha", "tag_alpha", "bar_alpha", "seg_alpha"):
            object.__setattr__(self, n, _alpha(n, getattr(self, n)))
        if int(self.thickness) != self.thickness or self.thickness < 1:
            raise ValueError(f"thickness {self.thickness!r}: an integer >= 1")
        _int_in("tag_scale", self.tag_scale, 1, MAX_TAG_SCALE)
        _int_in("lane_h", self.lane_h, 0, MAX_LANE_H)


# The label font: 5 x 7 dots per glyph, drawn by hand for this file ('#' = ink); rows top to bottom, separated by '/'.
_FONT = {
    " ": "...../...../...../...../...../...../.....",
    "0": ".###./#...#/#..##/#.#.#/##..#/#...#/.###.",
    "1": "..#../.##../..#../..#../..#../..#../.###.",
    "2": ".###./#...#/....#/...#./..#../.#.../#####",
    "3": "#####/...#./..#../...#./....#/#...#/.###.",
    "4": "...#./..##./.#.#./#..#./#####/...#./...#.",
    "5": "#####/#..../####./....#/....#/#...#/.###.",
    "6": "..##./.#.../#..../####./#...#/#...#/.###.",
    "7": "#####/....#/...#./..#../.#.../.#.../.#...",
    "8": ".###./#...#/#...#/.###./#...#/#...#/.###.",
    "9": ".###./#...#/#...#/.####/....#/...#./.##..",
    "A": ".###./#...#/#...#/#####/#...#/#...#/#...#",
    "B": "####./#...#/#...#/####./#...#/#...#/####.",
    "C": ".###./#...#/#..../#..../#..../#...#/.###.",
    "D": "###../#..#./#...#/#...#/#...#/#..#./###..",
    "E": "#####/#..../#..../####./#..../#..../#####",
    "F": "#####/#..../#..../####./#..../#..../#....",
    "G": ".###./#...#/#..../#.###/#...#/#...#/.####",
    "H": "#...#/#...#/#...#/#####/#...#/#...#/#...#",
    "I": ".###./..#../..#../..#../..#../..#../.###.",
    "J": "..###/...#./...#./...#./...#./#..#./.##..",
    "K": "#...#/#..#./#.#../##.../#.#../#..#./#...#",
    "L": "#..../#..../#..../#..../#..../#..../#####",
    "M": "#...#/##.##/#.#.#/#.#.#/#...#/#...#/#...#",
    "N": "#...#/#...#/##..#/#.#.#/#..##/#...#/#...#",
    "O": ".###./#...#/#...#/#...#/#...#/#...#/.###.",
    "P": "####./#...#/#...#/####./#..../#..../#....",
    "Q": ".###./#...#/#...#/#...#/#.#.#/#..#./.##.#",
    "R": "####./#...#/#...#/####./#.#../#..#./#...#",
    "S": ".####/#..../#..../.###./....#/....#/####.",
    "T": "#####/..#../..#../..#../..#../..#../..#..",
    "U": "#...#/#...#/#...#/#...#/#...#/#...#/.###.",
    "V": "#...#/#...#/#...#/#...#/#...#/.#.#./..#..",
    "W": "#...#/#...#/#...#/#.#.#/#.#.#/#.#.#/.#.#.",
    "X": "#...#/#...#/.#.#./..#../.#.#./#...#/#...#",
    "Y": "#...#/#...#/#...#/.#.#./..#../..#../..#..",
    "Z": "#####/....#/...#./..#../.#.../#..../#####",
    ".": "...../...../...../...../...../.##../.##..",
    ":": "...../.##../.##../...../.##../.##../.....",
    "%": "##.../##..#/...#./..#../.#.../#..##/...##",
    "-": "...../...../...../#####/...../...../.....",
    "#": ".#.#./.#.#./#####/.#.#./#####/.#.#./.#.#.",
}
FONT_H, FONT_W = 7, 5
MAX_LABEL_CHARS = (MAX_TAG_W - 1) // (FONT_W + 1)


def _label_rows(texts) -> List[List[int]]:
    """The (K, 9, w) bytes of ``label_tags`` as nested lists (no device, no tensor: this is also ``annotate_tubes``'s check)."""
    if isinstance(texts, str) or not isinstance(texts, (list, tuple)) or not 1 <= len(texts) <= MAX_RECTS or not all(isinstance(s, str) for s in texts):
        raise ValueError(f"texts: a list of 1..{MAX_RECTS} strings")
    texts = [s.upper() for s in texts]
    for s in texts:
        for ch in s:
            if ch not in _FONT:
                raise ValueError(f"label {s!r}: no glyph for {ch!r} (digits, A-Z, space and . : % - #)")
        if len(s) > MAX_LABEL_CHARS:
            raise ValueError(f"label {s!r}: more than {MAX_LABEL_CHARS} characters")
    w = 1 + (FONT_W + 1) * max(len(s) for s in texts)
    out = []
    for s in texts:
        rows = [[0] * w for _ in range(FONT_H + 2)]
        for i, ch in enumerate(s):
            for y, line in enumerate(_FONT[ch].split("/")):
                for x, dot in enumerate(line):
                    if dot == "#":
                        rows[1 + y][1 + (FONT_W + 1) * i + x] = 255
        out.append(rows)
    return out


def label_tags(texts: Sequence[str], device=None) -> torch.Tensor:
    """uint8 (K, 9, w) alpha bitmaps of K labels for ``annotate_tubes`` / ``overlay_multi_job``: the built-in 5 x 7 font (digits,
    A-Z - lowercase maps to uppercase -, space and . : % - #) with a margin of one sample, a column between glyphs, ink = 255,
    rows padded to the longest text (w = 6 n + 1).  Any other character raises ValueError.  ``device``: where the tensor goes."""
    t = torch.tensor(_label_rows(texts), dtype=torch.uint8)
    return t if device is None else t.to(device)


def overlay_multi_job(src: int, T: int, sh: int, sw: int, dst: Optional[int] = None, pix_fmt: str = "rgb24", boxes: Optional[int] = None, n_tube: int = 0, K: int = 1,
                      span: Optional[int] = None, frame_map: Optional[int] = None, heat: Optional[int] = None, heat_hw: Tuple[int, int] = (0, 0),
                      tags: Optional[int] = None, tag_hw: Tuple[int, int] = (0, 0), tag_scale: int = 1, tag_alpha: int = 0, tag_text_color=(0, 0, 0),
                      tube_colors=PALETTE, heat_color=(255, 0, 0), dim_color=(0, 0, 0), thickness: int = 2, heat_alpha: int = 0, dim_alpha: int = 0,
                      lane_h: int = 0, bar_color=(32, 32, 32), bar_alpha: int = 0, seg_alpha: int = 0, cursor_color=(255, 255, 255),
                      src_planes: Optional[Sequence[int]] = None, src_pitches: Optional[Sequence[int]] = None, src_frame_stride: Optional[int] = None,
                      dst_planes: Optional[Sequence[int]] = None, dst_pitches: Optional[Sequence[int]] = None, dst_frame_stride: Optional[int] = None):
    """One ``td_overlay_multi_job``: the frames side is ``overlay_job``'s; ``boxes`` (fp32 [n_tube][K][4]), ``span`` (int64 [K][2]),
    ``frame_map``, ``heat`` and ``tags`` (uint8 [K][tag_hw[0]][tag_hw[1]], needs ``boxes``) are device addresses or None; the
    colours - ``tube_colors`` are eight - are three bytes in the FRAMES' colour space (``color_in_space``); ``lane_h`` > 0 draws
    the timeline (then 1 <= n_tube <= 2^20 and K lane_h <= sh)."""
    from . import _hip

    T, sh, sw, n_tube = int(T), int(sh), int(sw), int(n_tube)
    _check_geometry(pix_fmt, T, sh, sw)
    K = _int_in("K", K, 1, MAX_RECTS)
    if int(thickness) != thickness or thickness < 1:
        raise ValueError(f"thickness {thickness!r}: an integer >= 1")
    mh, mw = int(heat_hw[0]), int(heat_hw[1])
    if heat is not None and not (1 <= mh <= MAX_MAP and 1 <= mw <= MAX_MAP):
        raise ValueError(f"token grid {mh} x {mw}: sides in 1..{MAX_MAP}")
    if n_tube < 0:
        raise ValueError(f"n_tube = {n_tube} is negative")
    tag_h, tag_w = int(tag_hw[0]), int(tag_hw[1])
    if tags is not None:
        if boxes is None:
            raise ValueError("tags need boxes")
        if not (1 <= tag_h <= MAX_TAG_H and 1 <= tag_w <= MAX_TAG_W):
            raise ValueError(f"tags of {tag_h} x {tag_w}: 1..{MAX_TAG_H} rows of 1..{MAX_TAG_W} samples")
        tag_scale = _int_in("tag_scale", tag_scale, 1, MAX_TAG_SCALE)
    lane_h = _int_in("lane_h", lane_h, 0, MAX_LANE_H)
    if lane_h and not 1 <= n_tube <= MAX_TIMELINE_ROWS:
        raise ValueError(f"a timeline (lane_h > 0) needs n_tube in 1..{MAX_TIMELINE_ROWS}, not {n_tube}")
    if K * lane_h > sh:
        raise ValueError(f"K lane_h = {K} x {lane_h} rows do not fit a frame of {sh} rows")
    tube_colors = tuple(tube_colors)
    if len(tube_colors) != MAX_RECTS:
        raise ValueError(f"tube_colors: {MAX_RECTS} colours, not {len(tube_colors)}")
    fmt, tight, sizes = _planes(pix_fmt, sh, sw)
    j = _hip.OverlayMultiJob()
    _describe_src_dst(j, src, dst, sizes, tight, src_planes, src_pitches, src_frame_stride, dst_planes, dst_pitches, dst_frame_stride)
    j.fmt, j.T, j.sh, j.sw = fmt, T, sh, sw
    j.boxes, j.span, j.frame_map, j.heat, j.tags = boxes, span, frame_map, heat, tags
    j.n_tube, j.K, j.mh, j.mw = n_tube, K, mh, mw
    j.thickness, j.heat_alpha, j.dim_alpha = int(thickness), _alpha("heat_alpha", heat_alpha), _alpha("dim_alpha", dim_alpha)
    j.tag_h, j.tag_w, j.tag_scale, j.tag_alpha = tag_h, tag_w, int(tag_scale), _alpha("tag_alpha", tag_alpha)
    j.lane_h, j.bar_alpha, j.seg_alpha = lane_h, _alpha("bar_alpha", bar_alpha), _alpha("seg_alpha", seg_alpha)
    for k, c in enumerate(tube_colors):
        j.tube_color[k][:] = _rgb3(f"tube_colors[{k}]", c)
    for name, c in (("heat_color", heat_color), ("dim_color", dim_color), ("tag_text_color", tag_text_color), ("bar_color", bar_color), ("cursor_color", cursor_color)):
        getattr(j, name)[:] = _rgb3(name, c)
    return j


def tube_overlay_multi(jobs: Sequence, device) -> tuple:
    """One td_tube_overlay_multi launch on the current stream with freshly allocated job tables; returns them: the caller keeps
    them alive until the stream has passed the launch (``annotate_tubes`` recycles its own instead)."""
    return _launch_fresh("td_tube_overlay_multi", jobs, device)


def annotate_tubes(frames: Union[DeviceFrames, Sequence[DeviceFrames]], boxes, span=None, heat=None, frame_map=None, tags=None, style: TubeSetStyle = TubeSetStyle(),
                   out: Union[None, DeviceFrames, Sequence[DeviceFrames]] = None):
    """Draw the K <= 8 tubes of a clip - the answers to K sentences, or the K best moments of one - into its decoded frames, each
    in its own colour with a label, and a timeline of the K spans: ONE launch and one pass over the frames for one clip or for a
    list of clips (then ``boxes``, ``span``, ``heat``, ``frame_map``, ``tags`` and ``out`` are lists too, or None).  Per clip:
      boxes      fp32 (n_tube, 4) or (n_tube, K, 4) xyxy in the frames' pixels on the device; (n_tube, 4) with a (K, 2) span: the one
                 tube is drawn in the colour of every moment whose span holds the frame; None: no box;
      span       int64 (2,) or (K, 2) tube rows, both ends included: rows of ``sted_decode``, ``DenseTubes.span`` or ``Moments.pairs[v]``
                 (a (-1, -1) row never draws); None: all rows;
      heat       uint8 (n_tube, mh, mw); None: no attention overlay;
      frame_map  int32 (T,): the tube row of each frame; None: frame t is row t (as for ``DenseTubes``);
      tags       the labels: a uint8 (K, h, w) tensor on the device (``label_tags``), or a list of K strings, which are rasterised
                 on the host and travel with the job table; None: no labels;
      out        ``DeviceFrames`` of the same geometry to write into; the clip itself: in place; None: a new buffer.
    ``style.lane_h`` > 0 draws the timeline and needs boxes or heat (they say how many tube rows there are).  The rule is exact and
    stated in include/tubedetr_hip.h.  Returns the annotated ``DeviceFrames`` (a list for a list).  Nothing here synchronises or
    copies to the host, and every refusal comes before the first allocation."""
    from . import _hip

    single = isinstance(frames, DeviceFrames)
    clips = [frames] if single else list(frames)
    n = len(clips)
    if n == 0:
        return []
    if not isinstance(clips[0], DeviceFrames):
        raise ValueError("frames: DeviceFrames on one device")
    if not isinstance(style, TubeSetStyle):
        raise ValueError("style: a TubeSetStyle")
    device = clips[0].data.device
    boxes_l, span_l, heat_l, map_l, out_l = (_as_list(v, n, k) for v, k in ((boxes, "boxes"), (span, "span"), (heat, "heat"), (frame_map, "frame_map"), (out, "out")))
    tags_l = [tags] if single else _as_list(tags, n, "tags")
    prepared, tail = [], 0
    for c, b, s, h, m, g, o in zip(clips, boxes_l, span_l, heat_l, map_l, tags_l, out_l):  # every refusal comes before the first allocation and the launch
        if not isinstance(c, DeviceFrames) or c.data.device != device:
            raise ValueError("frames: DeviceFrames on one device")
        b = _dev_tensor(b, torch.float32, (4,), "boxes", device)
        s = _dev_tensor(s, torch.int64, (2,), "span", device)
        h = _dev_tensor(h, torch.uint8, (), "heat", device)
        m = _dev_tensor(m, torch.int32, (c.T,), "frame_map", device)
        if b is not None and b.dim() not in (2, 3) or s is not None and s.dim() not in (1, 2) or m is not None and m.dim() != 1 or h is not None and h.dim() != 3:
            raise ValueError("boxes (n_tube, 4) or (n_tube, K, 4), span (2,) or (K, 2), heat (n_tube, mh, mw), frame_map (T,)")
        K = int(b.shape[1]) if b is not None and b.dim() == 3 else int(s.shape[0]) if s is not None and s.dim() == 2 else 1
        if not 1 <= K <= MAX_RECTS:
            raise ValueError(f"K = {K} tubes per clip: 1..{MAX_RECTS}")
        if s is not None and not (s.dim() == 1 and K == 1 or s.dim() == 2 and s.shape[0] == K):
            raise ValueError(f"span: (2,) for one tube, ({K}, 2) for {K}")
        if h is not None and not (1 <= h.shape[1] <= MAX_MAP and 1 <= h.shape[2] <= MAX_MAP):
            raise ValueError(f"heat: uint8 (n_tube, mh, mw) with mh and mw in 1..{MAX_MAP}")
        if b is not None and h is not None and b.shape[0] != h.shape[0]:
            raise ValueError(f"boxes have {b.shape[0]} tube rows, heat has {h.shape[0]}")
        n_tube = b.shape[0] if b is not None else h.shape[0] if h is not None else 2 ** 31 - 1  # span only: no array that a row could index past
        if style.lane_h and not 1 <= n_tube <= MAX_TIMELINE_ROWS:
            raise ValueError(f"a timeline (style.lane_h > 0) needs boxes or heat with 1..{MAX_TIMELINE_ROWS} tube rows")
        if K * style.lane_h > c.h:
            raise ValueError(f"K lane_h = {K} x {style.lane_h} rows do not fit a frame of {c.h} rows")
        rows, off = None, None
        if g is not None:
            if b is None:
                raise ValueError("tags need boxes")
            if torch.is_tensor(g):
                g = _dev_tensor(g, torch.uint8, (), "tags", device)
                if g.dim() != 3 or g.shape[0] != K or not (1 <= g.shape[1] <= MAX_TAG_H and 1 <= g.shape[2] <= MAX_TAG_W):
                    raise ValueError(f"tags: uint8 ({K}, h, w) with h in 1..{MAX_TAG_H} and w in 1..{MAX_TAG_W}, or {K} strings")
                tag_hw = (int(g.shape[1]), int(g.shape[2]))
            else:
                rows = _label_rows(g)
                if len(rows) != K:
                    raise ValueError(f"tags: {len(rows)} labels for {K} tubes")
                tag_hw = (len(rows[0]), len(rows[0][0]))
                off, tail = tail, tail + (K * tag_hw[0] * tag_hw[1] + 15) // 16 * 16
                g = None
        else:
            tag_hw = (0, 0)
        if o is not None and (not isinstance(o, DeviceFrames) or (o.T, o.h, o.w, o.pix_fmt) != (c.T, c.h, c.w, c.pix_fmt) or o.data.device != device):
            raise ValueError("out: DeviceFrames of the clip's geometry and pixel format on its device")
        prepared.append((c, b, s, h, m, g, o, K, n_tube, tag_hw, rows, off))
    jobs, keep, results, uploads = [], [], [], []
    for c, b, s, h, m, g, o, K, n_tube, tag_hw, rows, off in prepared:
        if o is None:
            o = c.empty_like()
        if b is not None and b.dim() == 2 and K > 1:  # one tube, K moments
            b = b[:, None, :].expand(-1, K, -1).contiguous()
        space = (c.pix_fmt, c.matrix, c.full_range)
        has_tags = g is not None or rows is not None
        # (labels given as strings have no device address yet: fill_tail puts it into the job; 1 stands for "there are tags" until then)
        j = overlay_multi_job(c.data.data_ptr(), c.T, c.h, c.w, o.data.data_ptr(), c.pix_fmt, _hip.ptr(b), n_tube, K, _hip.ptr(s), _hip.ptr(m), _hip.ptr(h),
                              tuple(h.shape[1:]) if h is not None else (0, 0), _hip.ptr(g) if g is not None else (1 if rows is not None else None), tag_hw,
                              style.tag_scale if has_tags else 1, style.tag_alpha, color_in_space(style.tag_text_color, *space),
                              tuple(color_in_space(col, *space) for col in style.colors), color_in_space(style.heat_color, *space), color_in_space(style.dim_color, *space),
                              style.thickness, style.heat_alpha, style.dim_alpha, style.lane_h, color_in_space(style.bar_color, *space), style.bar_alpha, style.seg_alpha,
                              color_in_space(style.cursor_color, *space))
        if rows is not None:
            uploads.append((j, off, rows))
        jobs.append(j)
        keep.append((b, s, h, m, g))
        results.append(o)

    def fill_tail(host_tail, dev_tail):
        for j, off, rows in uploads:  # the labels travel in the table's memory; the job gets their device address
            flat = torch.tensor(rows, dtype=torch.uint8).view(-1)
            host_tail[off:off + flat.numel()].copy_(flat)
            j.tags = dev_tail.data_ptr() + off
        dev_tail.copy_(host_tail, non_blocking=True)

    return _launch_pooled("td_tube_overlay_multi", jobs, keep, results, single, device, tail, fill_tail)


# ---- rendered frames exported: cut, downscaled, converted (td_frame_export, csrc/frame_export.hip) ----------------------------
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
    from . import _hip

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
    (j.src0, j.src1, j.src2), (j.src_pitch0, j.src_pitch1, j.src_pitch2), j.src_frame_stride = _describe(src, ssizes, stight, src_planes, src_pitches, src_frame_stride)
    (j.dst0, j.dst1, j.dst2), (j.dst_pitch0, j.dst_pitch1, j.dst_pitch2), j.dst_frame_stride = _describe(dst, dsizes, dtight, dst_planes, dst_pitches, dst_frame_stride)
    j.src_fmt, j.dst_fmt, j.matrix, j.full_range = sfmt, dfmt, _MATRICES.index(matrix), int(bool(full_range))
    j.T, j.sh, j.sw, j.take, j.To, j.oh, j.ow, j.dh, j.dw = T, sh, sw, take, To, oh, ow, dh, dw
    j.pad[:] = _rgb3("pad", pad)
    j.valid = valid
    return j


def frame_export(jobs: Sequence, device) -> tuple:
    """One td_frame_export launch on the current stream with freshly allocated job tables; returns them: the caller keeps
    them alive until the stream has passed the launch (``export`` recycles its own instead)."""
    return _launch_fresh("td_frame_export", jobs, device)


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
    from . import _hip

    single = isinstance(frames, DeviceFrames)
    clips = [frames] if single else list(frames)
    n = len(clips)
    if n == 0:
        return []
    if not isinstance(clips[0], DeviceFrames):
        raise ValueError("frames: DeviceFrames on one device")
    device = clips[0].data.device
    multiple = _int_in("multiple", multiple, 1, 256)
    pad_color = _rgb3("pad_color", pad_color)
    if pix_fmt is not None and pix_fmt not in _PIX_FMTS:
        raise ValueError(f"pix_fmt {pix_fmt!r}: one of {_PIX_FMTS}")
    take_l = [take] if single else _as_list(take, n, "take")
    To_l = [To] if single else _as_list(To, n, "To")
    prepared = []
    for c, tk, to in zip(clips, take_l, To_l):  # every refusal comes before the first allocation and the launch
        if not isinstance(c, DeviceFrames) or c.data.device != device:
            raise ValueError("frames: DeviceFrames on one device")
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
    if not jobs:
        return results[0] if single else results
    return _launch_pooled("td_frame_export", jobs, keep, results, single, device)
