"""numpy restatement of td_tube_crop's rule (include/tubedetr_hip.h, steps 1 - 6, 8 and 9: tube row, empties, rounding,
margin, clamp, output size, valid and the window record) and the composer of the expected output: the pixels themselves
(step 7) are whatever a given resizer makes of the sub-image - td_clip_resample on the GPU, ``resample_f64`` in float64.
Written from the header's text, with Python integers (unbounded) and np.float32 for the rounding step."""
import numpy as np

from tube_rule_ref import box_in_frame, round_coord  # noqa: F401 (round_coord: tests import it from here)

EMPTY = (0, 0, 0, 0, 0, 0)


def out_size(ch: int, cw: int, oh: int, ow: int, keep_aspect) -> tuple:
    """rh x rw of a ch x cw window in oh x ow (step 6)."""
    if not keep_aspect:
        return oh, ow
    if cw * oh >= ch * ow:
        return min(oh, max(1, (2 * ch * ow + cw) // (2 * cw))), ow
    return oh, min(ow, max(1, (2 * cw * oh + ch) // (2 * ch)))


def box_window(box, sh: int, sw: int, oh: int, ow: int, margin=(0, 1), keep_aspect=True) -> tuple:
    """(wy0, wx0, ch, cw, rh, rw) of one box in an sh x sw frame, or EMPTY (steps 2 - 6 without the span and the tube row)."""
    w = box_in_frame(box, sh, sw, margin)  # steps 2 (finiteness) to 5
    if w is None:
        return EMPTY
    wx0, wx1, wy0, wy1 = w
    cw, ch = wx1 - wx0, wy1 - wy0
    rh, rw = out_size(ch, cw, oh, ow, keep_aspect)
    return wy0, wx0, ch, cw, rh, rw


def tube_windows(boxes, T: int, sh: int, sw: int, oh: int, ow: int, span=None, frame_map=None, margin=(0, 1), keep_aspect=True):
    """(valid bool [T], windows int32 [T][6]) of a tube (steps 1 - 6, 8, 9)."""
    boxes = np.asarray(boxes, dtype=np.float32).reshape(-1, 4)
    valid, windows = np.zeros(T, dtype=bool), np.zeros((T, 6), dtype=np.int32)
    for t in range(T):
        r = int(frame_map[t]) if frame_map is not None else t
        if not 0 <= r < boxes.shape[0]:
            continue
        if span is not None and not int(span[0]) <= r <= int(span[1]):
            continue
        w = box_window(boxes[r], sh, sw, oh, ow, margin, keep_aspect)
        if w != EMPTY:
            valid[t], windows[t] = True, w
    return valid, windows


def compose(frames_rgb: np.ndarray, windows: np.ndarray, oh: int, ow: int, resize):
    """Expected (pixels uint8 [T][3][oh][ow], mask uint8 [T][oh][ow]) from rgb frames (T, sh, sw, 3), the window records and
    ``resize(t, sub_image (ch, cw, 3), rh, rw) -> (rh, rw, 3) uint8``: the resized window top-left, zeros and mask 1 around."""
    T = frames_rgb.shape[0]
    pixels, mask = np.zeros((T, 3, oh, ow), dtype=np.uint8), np.ones((T, oh, ow), dtype=np.uint8)
    for t in range(T):
        wy0, wx0, ch, cw, rh, rw = (int(v) for v in windows[t])
        if rh == 0:
            continue
        out = np.asarray(resize(t, frames_rgb[t, wy0 : wy0 + ch, wx0 : wx0 + cw], rh, rw))
        assert out.shape == (rh, rw, 3) and out.dtype == np.uint8
        pixels[t, :, :rh, :rw] = out.transpose(2, 0, 1)
        mask[t, :rh, :rw] = 0
    return pixels, mask
