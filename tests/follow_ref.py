"""numpy restatement of td_tube_follow's rule, written from the text in include/tubedetr_hip.h (not from the kernel): the luma of
the three pixel formats, the anchor choice, the 16 x 16 template, the candidates' sums, the tie order and the accept test.  Every
integer is exact (Python integers / numpy int64); the one float step, box + offset, is one np.float32 addition per coordinate.
``scene`` is the synthetic clip the rule was tried on: a panning texture, an object that moves on eased (not straight) paths
between the sampled frames, a little noise."""
import numpy as np

from tube_rule_ref import round_coord

GRID = 16
F32 = np.float32


def luma_of_rgb(rgb):
    """(..., 3) uint8 -> uint8: (77 R + 150 G + 29 B + 128) >> 8."""
    c = np.asarray(rgb).astype(np.int64)
    return ((77 * c[..., 0] + 150 * c[..., 1] + 29 * c[..., 2] + 128) >> 8).astype(np.uint8)


def luma_of_planes(planes, fmt):
    """rgb24: the (T, sh, sw, 3) array; yuv420p: (Y, U, V); nv12: (Y, UV).  Returns uint8 (T, sh, sw); chroma is never read."""
    return luma_of_rgb(planes) if fmt == "rgb24" else np.asarray(planes[0], dtype=np.uint8)


def find_anchor(boxes, anchor, t, k, reach, shot=None):
    """Step 2: the anchor frame of (t, k), or None."""
    T = boxes.shape[0]
    for d in range(1, reach + 1):
        for q in (t - d, t + d):
            if 0 <= q < T and anchor[q] != 0 and np.isfinite(boxes[q, k]).all() and (shot is None or shot[q] == shot[t]):
                return q
    return None


def sample_points(a, sh, sw):
    """Step 4 for the rounded anchor box a: (py, px) int64 (16,) each, or None when nothing of the box lies in the frame."""
    x0, y0, x1, y1 = max(a[0], 0), max(a[1], 0), min(a[2], sw), min(a[3], sh)
    w, h = x1 - x0, y1 - y0
    if w <= 0 or h <= 0:
        return None
    j = np.arange(GRID, dtype=np.int64)
    return y0 + ((2 * j + 1) * h) // 32, x0 + ((2 * j + 1) * w) // 32


def candidate_costs(Lt, tem, py, px, ddy, ddx, R):
    """Step 6: c(dy, dx) for every candidate, int64 (2 R + 1, 2 R + 1) indexed [dy + R][dx + R]."""
    sh, sw = Lt.shape
    Lt = Lt.astype(np.int64)
    c = np.zeros((2 * R + 1, 2 * R + 1), dtype=np.int64)
    for dy in range(-R, R + 1):
        rows = Lt[np.clip(py + ddy + dy, 0, sh - 1)]
        for dx in range(-R, R + 1):
            c[dy + R, dx + R] = np.abs(rows[:, np.clip(px + ddx + dx, 0, sw - 1)] - tem).sum()
    return c


def best_candidate(c, R):
    """Step 7: (cost, dy, dx): the smallest c, then the smallest dy^2 + dx^2, then dy, then dx."""
    best = min((int(c[dy + R, dx + R]), dy * dy + dx * dx, dy, dx) for dy in range(-R, R + 1) for dx in range(-R, R + 1))
    return best[0], best[2], best[3]


def follow_ref(luma, boxes, anchor, shot=None, radius=8, reach=3, accept=(24, 1)):
    """luma uint8 (T, sh, sw); boxes fp32 (T, K, 4) or (T, 4); anchor (T,); shot int (T,) or None; accept (num, den) or an integer.
    Returns a dict: out fp32 like boxes (compare its bits), offset int32 (.., 2) as (dy, dx), cost uint32, status uint8."""
    luma = np.asarray(luma, dtype=np.uint8)
    given = np.asarray(boxes, dtype=F32)
    b3 = given[:, None] if given.ndim == 2 else given
    T, K = b3.shape[:2]
    sh, sw = luma.shape[1:] if T else (1, 1)
    num, den = accept if isinstance(accept, (tuple, list)) else (accept, 1)
    out = b3.copy()
    offset = np.zeros((T, K, 2), dtype=np.int32)
    cost = np.zeros((T, K), dtype=np.uint32)
    status = np.zeros((T, K), dtype=np.uint8)
    for t in range(T):
        for k in range(K):
            B = b3[t, k]
            if anchor[t] != 0 or not np.isfinite(B).all():
                continue  # 1: copied
            g = find_anchor(b3, anchor, t, k, reach, shot)
            if g is None:
                continue
            a = [round_coord(v) for v in b3[g, k]]
            b = [round_coord(v) for v in B]
            pts = sample_points(a, sh, sw)
            if pts is None:
                continue
            py, px = pts
            tem = luma[g][py[:, None], px[None, :]].astype(np.int64)
            ddx, ddy = ((b[0] + b[2]) - (a[0] + a[2])) >> 1, ((b[1] + b[3]) - (a[1] + a[3])) >> 1
            c, dy, dx = best_candidate(candidate_costs(luma[t], tem, py, px, ddy, ddx, radius), radius)
            cost[t, k] = c
            if c * den <= num * 256:
                status[t, k] = 1
                offset[t, k] = (dy, dx)
                if dy != 0 or dx != 0:
                    out[t, k] = (B[0] + F32(dx), B[1] + F32(dy), B[2] + F32(dx), B[3] + F32(dy))
            else:
                status[t, k] = 2
    tail = given.shape[1:-1]
    return {"out": out.reshape(given.shape), "offset": offset.reshape((T,) + tail + (2,)), "cost": cost.reshape((T,) + tail), "status": status.reshape((T,) + tail)}


# ---- the synthetic scene -----------------------------------------------------------------------------------------------------------
OBJ_W, OBJ_H, INTERVAL = 40, 30, 6


def _smooth(a):
    for _ in range(2):
        a = (a + np.roll(a, 1, 0) + np.roll(a, 1, 1) + np.roll(a, -1, 0) + np.roll(a, -1, 1)) / 5
    return (a - a.min()) / (a.max() - a.min()) * 255


def scene(T=25, sh=96, sw=128, seed=0, noise=2):
    """A smoothed random texture that pans 1 px per frame with a 40 x 30 smoothed-texture object pasted over it; the object moves
    12 px in x and 6 px in y per 6-frame interval, eased inside each: x by round(12 p^2), y by round(6 sqrt(p)), p = (t mod 6) / 6;
    +-``noise`` levels per frame.  Returns (luma uint8 (T, sh, sw), true boxes fp32 (T, 4), anchor uint8 (T,) - 1 at t % 6 == 0 -,
    lerp fp32 (T, 4): the true boxes at the anchors and straight lines between them, the last anchor held behind it)."""
    rng = np.random.default_rng(seed)
    assert T <= 80  # the texture is 80 columns wider than the frame
    bg = _smooth(rng.integers(0, 256, (sh + 40, sw + 80)).astype(np.float64))
    ob = _smooth(rng.integers(0, 256, (OBJ_H, OBJ_W)).astype(np.float64))
    luma = np.zeros((T, sh, sw), dtype=np.uint8)
    true = np.zeros((T, 4), dtype=F32)
    for t in range(T):
        f = bg[10:10 + sh, t:t + sw].copy()
        p, k = (t % INTERVAL) / INTERVAL, t // INTERVAL
        ox, oy = 20 + 12 * k + int(round(12 * p * p)), 15 + 6 * k + int(round(6 * np.sqrt(p)))
        f[oy:oy + OBJ_H, ox:ox + OBJ_W] = ob[:max(min(OBJ_H, sh - oy), 0), :max(min(OBJ_W, sw - ox), 0)]
        f = f + rng.integers(-noise, noise + 1, f.shape)
        luma[t] = np.clip(f, 0, 255).astype(np.uint8)
        true[t] = (ox, oy, ox + OBJ_W, oy + OBJ_H)
    anchor = (np.arange(T) % INTERVAL == 0).astype(np.uint8)
    lerp = true.copy()
    for t in range(T):
        a = t // INTERVAL * INTERVAL
        if t != a:
            lerp[t] = true[a] + (true[a + INTERVAL] - true[a]) * F32((t - a) / INTERVAL) if a + INTERVAL < T else true[a]
    return luma, true, anchor, lerp


def corner_error(boxes, true):
    """The largest corner error per frame, in pixels."""
    return np.abs(np.asarray(boxes, dtype=np.float64) - np.asarray(true, dtype=np.float64)).max(axis=-1)
