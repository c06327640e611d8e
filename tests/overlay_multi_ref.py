"""numpy restatement of td_tube_overlay_multi's rule, written from the text in include/tubedetr_hip.h (not from the kernel): a
frame is a list of (alpha per luma pixel, colour) layers in the rule's order, applied by tests/overlay_ref.py's blend and chroma
mean.  Plain loops over frames, tubes and layers; Python integers for the timeline's 64-bit products.

Frames are "planes" as in tests/overlay_ref.py."""
import numpy as np

from overlay_ref import blend, box_alpha_map, box_corners, chroma_alpha, heat_alpha_map


def timeline_row(x, n_tube, sw):
    """i(x) = floor(x n_tube / sw)."""
    return (int(x) * int(n_tube)) // int(sw)


def cursor_columns(r, n_tube, sw):
    """[xc0, xc1) of tube row r."""
    xc0 = (int(r) * int(sw)) // int(n_tube)
    return xc0, max(((int(r) + 1) * int(sw)) // int(n_tube), xc0 + 1)


def tag_origin(x0, y0, tag_h, tag_scale):
    """(px0, py0) of the plate of a box whose rounded corner is (x0, y0)."""
    ph = tag_h * tag_scale
    return x0, (y0 - ph if y0 - ph >= 0 else y0)


def rect_alpha(sh, sw, x0, y0, x1, y1, a):
    """alpha a on the pixels of [x0, x1) x [y0, y1) that lie in the frame."""
    m = np.zeros((sh, sw), dtype=np.int64)
    xa, xb, ya, yb = max(x0, 0), min(x1, sw), max(y0, 0), min(y1, sh)
    if xa < xb and ya < yb:
        m[ya:yb, xa:xb] = a
    return m


def glyph_alpha(tag, sh, sw, px0, py0, scale):
    """The glyph layer of one tag (uint8 (tag_h, tag_w)): a = (256 m + 127) / 255 inside the plate."""
    a = np.zeros((sh, sw), dtype=np.int64)
    th, tw = tag.shape
    for y in range(max(py0, 0), min(py0 + th * scale, sh)):
        for x in range(max(px0, 0), min(px0 + tw * scale, sw)):
            a[y, x] = (256 * int(tag[(y - py0) // scale, (x - px0) // scale]) + 127) // 255
    return a


def frame_layers(r, sh, sw, K, n_tube, boxes, span, heat, tags, tube_color, heat_color, dim_color, thickness, heat_alpha, dim_alpha, tag_scale, tag_alpha, tag_text_color,
                 lane_h, bar_color, bar_alpha, seg_alpha, cursor_color):
    """The (alpha, colour) layers of a frame whose tube row r lies in [0, n_tube), in the rule's order."""

    def in_span(k):
        return span is None or int(span[k][0]) <= r <= int(span[k][1])

    stack = []
    if span is not None and not any(in_span(k) for k in range(K)):
        stack.append((np.full((sh, sw), dim_alpha, dtype=np.int64), dim_color))
    if heat is not None:
        stack.append((heat_alpha_map(heat[r], sh, sw, heat_alpha), heat_color))
    drawn = []
    if boxes is not None:
        for k in range(K):
            c = box_corners(boxes[r][k]) if in_span(k) else None
            drawn.append(c)
            if c is not None:
                stack.append((box_alpha_map(boxes[r][k], sh, sw, thickness), tube_color[k]))
        if tags is not None:
            for k in range(K):
                if drawn[k] is None:
                    continue
                th, tw = tags[k].shape
                px0, py0 = tag_origin(drawn[k][0], drawn[k][1], th, tag_scale)
                stack.append((rect_alpha(sh, sw, px0, py0, px0 + tw * tag_scale, py0 + th * tag_scale, tag_alpha), tube_color[k]))
                stack.append((glyph_alpha(tags[k], sh, sw, px0, py0, tag_scale), tag_text_color))
    if lane_h > 0:
        top = sh - K * lane_h
        stack.append((rect_alpha(sh, sw, 0, top, sw, sh, bar_alpha), bar_color))
        rows = np.array([timeline_row(x, n_tube, sw) for x in range(sw)])
        for k in range(K):
            a = np.zeros((sh, sw), dtype=np.int64)
            cols = np.ones(sw, dtype=bool) if span is None else (rows >= int(span[k][0])) & (rows <= int(span[k][1]))
            a[sh - (K - k) * lane_h : sh - (K - k - 1) * lane_h, cols] = seg_alpha
            stack.append((a, tube_color[k]))
        xc0, xc1 = cursor_columns(r, n_tube, sw)
        stack.append((rect_alpha(sh, sw, xc0, top, xc1, sh, 256), cursor_color))
    return stack


PALETTE = ((250, 255, 0), (0, 200, 255), (255, 90, 90), (90, 255, 125), (255, 140, 0), (200, 120, 255), (255, 120, 200), (0, 160, 140))


def overlay_multi_ref(planes, fmt, boxes=None, span=None, frame_map=None, heat=None, tags=None, K=None, n_tube=None, tube_color=PALETTE, heat_color=(255, 0, 0),
                      dim_color=(0, 0, 0), thickness=2, heat_alpha=0, dim_alpha=0, tag_scale=1, tag_alpha=0, tag_text_color=(0, 0, 0), lane_h=0, bar_color=(32, 32, 32),
                      bar_alpha=0, seg_alpha=0, cursor_color=(255, 255, 255)):
    """The annotated frames, same structure and dtype as ``planes``.  boxes (n_tube, K, 4) float32 | None; span (K, 2) | None;
    frame_map (T,) ints | None; heat uint8 (n_tube, mh, mw) | None; tags uint8 (K, tag_h, tag_w) | None; colours in the frames'
    own colour space."""
    rgb = fmt == "rgb24"
    planes = (planes,) if rgb else tuple(planes)
    out = [p.astype(np.int64) for p in planes]
    T, sh, sw = planes[0].shape[:3]
    if K is None:
        K = boxes.shape[1] if boxes is not None else len(span) if span is not None else 1
    if n_tube is None:
        n_tube = len(boxes) if boxes is not None else len(heat) if heat is not None else 2 ** 31 - 1
    for t in range(T):
        r = int(frame_map[t]) if frame_map is not None else t
        if not 0 <= r < n_tube:
            continue  # a plain copy
        for a, c in frame_layers(r, sh, sw, K, n_tube, boxes, span, heat, tags, tube_color, heat_color, dim_color, thickness, heat_alpha, dim_alpha, tag_scale, tag_alpha,
                                 tag_text_color, lane_h, bar_color, bar_alpha, seg_alpha, cursor_color):
            if rgb:
                for k in range(3):
                    out[0][t, :, :, k] = blend(out[0][t, :, :, k], c[k], a)
                continue
            out[0][t] = blend(out[0][t], c[0], a)
            ac = chroma_alpha(a)
            if fmt == "yuv420p":
                out[1][t] = blend(out[1][t], c[1], ac)
                out[2][t] = blend(out[2][t], c[2], ac)
            else:
                out[1][t, :, :, 0] = blend(out[1][t, :, :, 0], c[1], ac)
                out[1][t, :, :, 1] = blend(out[1][t, :, :, 1], c[2], ac)
    out = [o.astype(np.uint8) for o in out]
    return out[0] if rgb else tuple(out)
