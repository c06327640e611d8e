"""numpy restatement of td_tube_redact's rule, written from the text in include/tubedetr_hip.h (not from the kernel): the
numbers in the comments are the rule's steps.  Planes come and go in the layout of tests/test_overlay_gpu.py::make_planes:
rgb24 (T, sh, sw, 3); yuv420p (Y, U, V); nv12 (Y, UV) with UV (T, ch, cw, 2)."""
import numpy as np

from tube_rule_ref import box_in_frame, round_coord  # noqa: F401 (3: round_coord; 2 - 5: box_in_frame)

MODES = ("fill", "mosaic", "blur")


def snapped_rect(box, sh, sw, mode, cell, margin):
    """Steps 2 (finiteness) to 6 for one box: (X0, X1, Y0, Y1) in luma pixels, or None when the rectangle is absent."""
    w = box_in_frame(box, sh, sw, margin)
    if w is None:
        return None
    wx0, wx1, wy0, wy1 = w
    if mode == "mosaic":  # 6
        return ((wx0 // cell) * cell, min(((wx1 + cell - 1) // cell) * cell, sw), (wy0 // cell) * cell, min(((wy1 + cell - 1) // cell) * cell, sh))
    return (wx0 & ~1, min(wx1 + (wx1 & 1), sw), wy0 & ~1, min(wy1 + (wy1 & 1), sh))


def luma_selection(T, sh, sw, boxes, span=None, frame_map=None, mode="mosaic", cell=16, margin=(0, 1), invert=False):
    """7: bool (T, sh, sw), True where a luma pixel (rgb24: a pixel) is selected."""
    boxes = np.asarray(boxes, dtype=np.float32)
    if boxes.ndim == 2:
        boxes = boxes[:, None, :]
    n_tube, K = boxes.shape[:2]
    if span is not None:
        span = np.asarray(span, dtype=np.int64).reshape(K, 2)
    sel = np.zeros((T, sh, sw), dtype=bool)
    for t in range(T):
        r = int(frame_map[t]) if frame_map is not None else t  # 1
        if 0 <= r < n_tube:  # 2
            for k in range(K):
                if span is not None and not (span[k, 0] <= r <= span[k, 1]):
                    continue
                rect = snapped_rect(boxes[r, k], sh, sw, mode, cell, margin)
                if rect is not None:
                    sel[t, rect[2]:rect[3], rect[0]:rect[1]] = True
    return sel != bool(invert)


def mosaic_plane(a, cp):
    """8, MOSAIC: every sample of the (rows, cols) plane replaced by its cell's rounded mean."""
    rows, cols = a.shape
    ys, xs = np.arange(0, rows, cp), np.arange(0, cols, cp)
    sums = np.add.reduceat(np.add.reduceat(a.astype(np.int64), ys, axis=0), xs, axis=1)
    n = np.outer(np.minimum(ys + cp, rows) - ys, np.minimum(xs + cp, cols) - xs)
    v = (sums + n // 2) // n
    return np.repeat(np.repeat(v, cp, axis=0), cp, axis=1)[:rows, :cols]


def blur_plane(a, rp):
    """8, BLUR: every sample replaced by the rounded mean of the window's samples that lie in the plane."""
    rows, cols = a.shape
    S = np.zeros((rows + 1, cols + 1), dtype=np.int64)
    S[1:, 1:] = a.astype(np.int64).cumsum(0).cumsum(1)
    y0, y1 = np.maximum(np.arange(rows) - rp, 0), np.minimum(np.arange(rows) + rp, rows - 1) + 1
    x0, x1 = np.maximum(np.arange(cols) - rp, 0), np.minimum(np.arange(cols) + rp, cols - 1) + 1
    sums = S[y1][:, x1] - S[y0][:, x1] - S[y1][:, x0] + S[y0][:, x0]
    n = np.outer(y1 - y0, x1 - x0)
    return (sums + n // 2) // n


def redact_plane(a, sel, mode, par, value):
    """One channel of one plane of one frame: (rows, cols) uint8 and its selection."""
    if mode == "fill":
        new = np.full(a.shape, value, dtype=np.int64)
    elif mode == "mosaic":
        new = mosaic_plane(a, par)
    else:
        new = blur_plane(a, par)
    return np.where(sel, new, a).astype(np.uint8)


def redact_ref(planes, fmt, boxes, span=None, frame_map=None, mode="mosaic", cell=16, radius=8, color=(0, 0, 0), margin=(0, 1), invert=False):
    assert mode in MODES
    luma = planes if fmt == "rgb24" else planes[0]
    T, sh, sw = luma.shape[:3]
    sel = luma_selection(T, sh, sw, boxes, span, frame_map, mode, cell, margin, invert)
    csel = sel[:, 0::2, 0::2]  # 7: chroma sample (i, j) asks luma pixel (2 i, 2 j)
    par = cell if mode == "mosaic" else radius
    cpar = cell // 2 if mode == "mosaic" else (radius + 1) // 2

    def channels(p, s, pr, comps):  # p (T, rows, cols, len(comps))
        out = np.empty_like(p)
        for t in range(T):
            for c, comp in enumerate(comps):
                out[t, :, :, c] = redact_plane(p[t, :, :, c], s[t], mode, pr, color[comp])
        return out

    if fmt == "rgb24":
        return channels(planes, sel, par, (0, 1, 2))
    Y = channels(planes[0][..., None], sel, par, (0,))[..., 0]
    if fmt == "yuv420p":
        return (Y, channels(planes[1][..., None], csel, cpar, (1,))[..., 0], channels(planes[2][..., None], csel, cpar, (2,))[..., 0])
    return (Y, channels(planes[1], csel, cpar, (1, 2)))
