"""The steps that td_tube_overlay, td_tube_crop and td_tube_redact share (include/tubedetr_hip.h: a box's rounded corners, the
margin, the clamp to the frame), restated once for tests/overlay_ref.py, tests/tube_crop_ref.py and tests/redact_ref.py.
Written from the header's text: Python integers (unbounded), np.float32 for the rounding step."""
import numpy as np


def round_coord(v) -> int:
    """(int)floorf(clamp(v, +-2^20) + 0.5f) in fp32."""
    v = np.float32(v)
    v = np.minimum(np.maximum(v, np.float32(-1048576.0)), np.float32(1048576.0))
    return int(np.floor(np.float32(v + np.float32(0.5))))


def rounded_corners(box):
    """fp32 xyxy -> (x0, y0, x1, y1) ints, or None - the box is absent - when a corner is not finite or x1 <= x0 or y1 <= y0."""
    b = np.asarray(box, dtype=np.float32)
    if not np.isfinite(b).all():
        return None
    x0, y0, x1, y1 = (round_coord(v) for v in b)
    if x1 <= x0 or y1 <= y0:
        return None
    return x0, y0, x1, y1


def grow_and_clamp(corners, sh: int, sw: int, margin=(0, 1)):
    """margin = (num, den) of the box's side added on every side (the division's operands are not negative), then the clamp to
    the sh x sw frame: (wx0, wx1, wy0, wy1), or None when nothing of the box lies in the frame."""
    x0, y0, x1, y1 = corners
    num, den = int(margin[0]), int(margin[1])
    mx, my = ((x1 - x0) * num) // den, ((y1 - y0) * num) // den
    wx0, wx1, wy0, wy1 = max(x0 - mx, 0), min(x1 + mx, sw), max(y0 - my, 0), min(y1 + my, sh)
    if wx1 <= wx0 or wy1 <= wy0:
        return None
    return wx0, wx1, wy0, wy1


def box_in_frame(box, sh: int, sw: int, margin=(0, 1)):
    """Both steps for one box: (wx0, wx1, wy0, wy1) or None."""
    c = rounded_corners(box)
    return None if c is None else grow_and_clamp(c, sh, sw, margin)
