"""K labelled tubes and a moment timeline in one pass (td_tube_overlay_multi, csrc/overlay_multi.hip): ``annotate_tubes``."""
from __future__ import annotations

from dataclasses import dataclass
from typing import List, Optional, Sequence, Tuple, Union

import torch

from .. import _hip
from ..frame_jobs import MAX_MAP, MAX_RECTS, _alpha, _check_geometry, _grid_ok, _heat_grid, _int_in, _launch_pooled, _planes, _put_src_dst, _rgb3, _thickness
from .clips import _as_list, _check_clip, _check_K, _check_out, _clips_of, _dev_tensor, _device_of, _tube_tensors
from .frames import DeviceFrames, color_in_space

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
        _thickness(self.thickness)
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
    T, sh, sw, n_tube = int(T), int(sh), int(sw), int(n_tube)
    _check_geometry(pix_fmt, T, sh, sw)
    K = _int_in("K", K, 1, MAX_RECTS)
    _thickness(thickness)
    mh, mw = _heat_grid(heat_hw, heat is not None)
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
    _put_src_dst(j, src, dst, sizes, tight, src_planes, src_pitches, src_frame_stride, dst_planes, dst_pitches, dst_frame_stride)
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
    single, clips = _clips_of(frames)
    if not clips:
        return []
    n, device = len(clips), _device_of(clips)
    if not isinstance(style, TubeSetStyle):
        raise ValueError("style: a TubeSetStyle")
    boxes_l, span_l, heat_l, map_l, out_l = (_as_list(v, n, k) for v, k in ((boxes, "boxes"), (span, "span"), (heat, "heat"), (frame_map, "frame_map"), (out, "out")))
    tags_l = [tags] if single else _as_list(tags, n, "tags")
    prepared = []
    for c, b, s, h, m, g, o in zip(clips, boxes_l, span_l, heat_l, map_l, tags_l, out_l):  # every refusal comes before the first allocation and the launch
        _check_clip(c, device)
        b, s, h, m = _tube_tensors(b, s, h, m, c.T, device)
        if b is not None and b.dim() not in (2, 3) or s is not None and s.dim() not in (1, 2) or m is not None and m.dim() != 1 or h is not None and h.dim() != 3:
            raise ValueError("boxes (n_tube, 4) or (n_tube, K, 4), span (2,) or (K, 2), heat (n_tube, mh, mw), frame_map (T,)")
        K = int(b.shape[1]) if b is not None and b.dim() == 3 else int(s.shape[0]) if s is not None and s.dim() == 2 else 1
        _check_K(K, s, "K = {K} tubes per clip")
        if h is not None and not _grid_ok(h.shape[1], h.shape[2]):
            raise ValueError(f"heat: uint8 (n_tube, mh, mw) with mh and mw in 1..{MAX_MAP}")
        if b is not None and h is not None and b.shape[0] != h.shape[0]:
            raise ValueError(f"boxes have {b.shape[0]} tube rows, heat has {h.shape[0]}")
        n_tube = b.shape[0] if b is not None else h.shape[0] if h is not None else 2 ** 31 - 1  # span only: no array that a row could index past
        if style.lane_h and not 1 <= n_tube <= MAX_TIMELINE_ROWS:
            raise ValueError(f"a timeline (style.lane_h > 0) needs boxes or heat with 1..{MAX_TIMELINE_ROWS} tube rows")
        if K * style.lane_h > c.h:
            raise ValueError(f"K lane_h = {K} x {style.lane_h} rows do not fit a frame of {c.h} rows")
        rows = None
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
                g = None
        else:
            tag_hw = (0, 0)
        _check_out(o, c, device)
        prepared.append((c, b, s, h, m, g, o, K, n_tube, tag_hw, rows))
    jobs, keep, results, uploads = [], [], [], []
    for c, b, s, h, m, g, o, K, n_tube, tag_hw, rows in prepared:
        if o is None:
            o = c.empty_like()
        if b is not None and b.dim() == 2 and K > 1:  # one tube, K moments
            b = b[:, None, :].expand(-1, K, -1).contiguous()
        space = (c.pix_fmt, c.matrix, c.full_range)
        has_tags = g is not None or rows is not None
        # (labels given as strings have no device address yet: they travel with the table, and the launch puts their address into the job;
        # 1 stands for "there are tags" until then)
        j = overlay_multi_job(c.data.data_ptr(), c.T, c.h, c.w, o.data.data_ptr(), c.pix_fmt, _hip.ptr(b), n_tube, K, _hip.ptr(s), _hip.ptr(m), _hip.ptr(h),
                              tuple(h.shape[1:]) if h is not None else (0, 0), _hip.ptr(g) if g is not None else (1 if rows is not None else None), tag_hw,
                              style.tag_scale if has_tags else 1, style.tag_alpha, color_in_space(style.tag_text_color, *space),
                              tuple(color_in_space(col, *space) for col in style.colors), color_in_space(style.heat_color, *space), color_in_space(style.dim_color, *space),
                              style.thickness, style.heat_alpha, style.dim_alpha, style.lane_h, color_in_space(style.bar_color, *space), style.bar_alpha, style.seg_alpha,
                              color_in_space(style.cursor_color, *space))
        if rows is not None:
            uploads.append((j, "tags", torch.tensor(rows, dtype=torch.uint8)))
        jobs.append(j)
        keep.append((b, s, h, m, g))
        results.append(o)
    return _launch_pooled("td_tube_overlay_multi", jobs, keep, results, single, device, uploads)
