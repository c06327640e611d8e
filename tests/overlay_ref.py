"""numpy restatement of td_tube_overlay's rule, written from the text in include/tubedetr_hip.h (not from the kernel):
plain loops over frames and layers, one frame vectorised, int64 arithmetic, np.float32 for the box rounding.

Frames are "planes" as tests/test_yuv_input_gpu.py makes them: rgb24 one array (T, h, w, 3); yuv420p (Y (T, h, w),
U (T, ch, cw), V (T, ch, cw)); nv12 (Y, UV (T, ch, cw, 2)); ch = (h + 1) // 2, cw = (w + 1) // 2."""
import numpy as np

from tube_rule_ref import rounded_corners as box_corners  # fp32 xyxy -> (x0, y0, x1, y1) ints, or None for a box that draws nothing


def blend(v, c, a):
    """(v (256 - a) + c a + 128) >> 8 on int64 arrays."""
    return (v * (256 - a) + c * a + 128) >> 8


def map_coord(n_pix, m):
    """g of every pixel index 0..n_pix-1 for a map side of m samples."""
    v = np.arange(n_pix, dtype=np.int64)
    return np.clip(((2 * v + 1) * m * 128) // n_pix - 128, 0, 256 * (m - 1))


def heat_alpha_map(q, sh, sw, heat_alpha):
    """q: uint8 (mh, mw) -> the heat layer's alpha of every luma pixel, int64 (sh, sw)."""
    q = q.astype(np.int64)
    mh, mw = q.shape
    gy, gx = map_coord(sh, mh), map_coord(sw, mw)
    iy, fy, ix, fx = gy >> 8, (gy & 255)[:, None], gx >> 8, (gx & 255)[None, :]
    iy1, ix1 = np.minimum(iy + 1, mh - 1), np.minimum(ix + 1, mw - 1)
    q00, q01, q10, q11 = q[iy][:, ix], q[iy][:, ix1], q[iy1][:, ix], q[iy1][:, ix1]
    h = ((256 - fy) * ((256 - fx) * q00 + fx * q01) + fy * ((256 - fx) * q10 + fx * q11) + 32768) >> 16
    return (h * heat_alpha + 127) // 255


def box_alpha_map(box, sh, sw, th):
    c = box_corners(box)
    a = np.zeros((sh, sw), dtype=np.int64)
    if c is None:
        return a
    x0, y0, x1, y1 = c
    y, x = np.arange(sh)[:, None], np.arange(sw)[None, :]
    outer = (x >= x0) & (x < x1) & (y >= y0) & (y < y1)
    inner = (x >= x0 + th) & (x < x1 - th) & (y >= y0 + th) & (y < y1 - th)
    a[outer & ~inner] = 256
    return a


def chroma_alpha(a):
    """Mean alpha of the luma pixels of every 2 x 2 block that exist: (sum + n // 2) // n."""
    sh, sw = a.shape
    ch, cw = (sh + 1) // 2, (sw + 1) // 2
    s = np.zeros((2 * ch, 2 * cw), dtype=np.int64)
    n = np.zeros((2 * ch, 2 * cw), dtype=np.int64)
    s[:sh, :sw] = a
    n[:sh, :sw] = 1
    s = s.reshape(ch, 2, cw, 2).sum(axis=(1, 3))
    n = n.reshape(ch, 2, cw, 2).sum(axis=(1, 3))
    return (s + n // 2) // n


def overlay_ref(planes, fmt, boxes=None, span=None, frame_map=None, heat=None, box_color=(250, 255, 0), heat_color=(255, 0, 0), dim_color=(0, 0, 0),
                thickness=2, heat_alpha=0, dim_alpha=0, n_tube=None):
    """The annotated frames, same structure and dtype as ``planes``.  boxes (n_tube, 4) float32 | None; span (s0, s1) | None;
    frame_map (T,) ints | None; heat uint8 (n_tube, mh, mw) | None; colours in the frames' own colour space."""
    rgb = fmt == "rgb24"
    planes = (planes,) if rgb else tuple(planes)
    out = [p.astype(np.int64) for p in planes]
    T, sh, sw = planes[0].shape[:3]
    if n_tube is None:
        n_tube = len(boxes) if boxes is not None else len(heat) if heat is not None else 2 ** 31 - 1
    for t in range(T):
        r = int(frame_map[t]) if frame_map is not None else t
        if not 0 <= r < n_tube:
            continue  # a plain copy
        inside = span is None or int(span[0]) <= r <= int(span[1])
        stack = []  # (alpha per luma pixel, colour)
        if span is not None and not inside:
            stack.append((np.full((sh, sw), dim_alpha, dtype=np.int64), dim_color))
        if heat is not None:
            stack.append((heat_alpha_map(heat[r], sh, sw, heat_alpha), heat_color))
        if boxes is not None and inside:
            stack.append((box_alpha_map(boxes[r], sh, sw, thickness), box_color))
        for a, c in stack:
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
