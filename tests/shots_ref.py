"""numpy restatement of the shot-cut rules, written from the text in include/tubedetr_hip.h (not from the kernels): td_frame_stats
(sampled pixels, luma, histogram, sum of absolute differences), td_shot_cuts (the four conditions, the tie rule, the prefix sum)
and td_tube_densify_shots (the densify rule of tests/tube_dense_ref.py, imported and not edited, stopped at cuts).  Every
integer is exact: Python integers or numpy int64 / uint32.  ``synthetic_clip`` is the clip the defaults were tried on."""
import numpy as np

from tube_dense_ref import F32, QNAN_BITS, densify_ref, place, presence, row_frames, working_box

BINS = 64


# ---- td_frame_stats -------------------------------------------------------------------------------------------------------------
def luma_of_rgb(rgb):
    """(..., 3) uint8 -> uint8: (77 R + 150 G + 29 B + 128) >> 8."""
    c = np.asarray(rgb).astype(np.int64)
    return ((77 * c[..., 0] + 150 * c[..., 1] + 29 * c[..., 2] + 128) >> 8).astype(np.uint8)


def sampled_pixels(sh, sw, step=1):
    return ((sh + step - 1) // step) * ((sw + step - 1) // step)


def frame_stats_ref(luma, step=1):
    """luma uint8 (T, sh, sw): the Y plane as stored, or luma_of_rgb.  Returns (hist uint32 (T, 64), sad uint32 (T,), N)."""
    luma = np.asarray(luma, dtype=np.uint8)
    T, sh, sw = luma.shape
    s = luma[:, ::step, ::step].astype(np.int64).reshape(T, -1)
    n = sampled_pixels(sh, sw, step)
    assert s.shape[1] == n
    hist = np.zeros((T, BINS), dtype=np.uint32)
    sad = np.zeros(T, dtype=np.uint32)
    for t in range(T):
        hist[t] = np.bincount(s[t] >> 2, minlength=BINS)
        if t > 0:
            sad[t] = np.abs(s[t] - s[t - 1]).sum()
    return hist, sad, n


# ---- td_shot_cuts ---------------------------------------------------------------------------------------------------------------
def hist_distance(hist):
    """d uint32 (T,): d[0] = 0, d[t] = sum_b |hist[t][b] - hist[t-1][b]|."""
    h = np.asarray(hist).astype(np.int64)
    d = np.zeros(h.shape[0], dtype=np.uint32)
    if h.shape[0] > 1:
        d[1:] = np.abs(h[1:] - h[:-1]).sum(1)
    return d


def conditions(d, sad, n, t, hist_thr=(1, 4), sad_thr=(8, 1), peak=(3, 1), w=4):
    """The four conditions of frame t >= 1, as a tuple of bools, in Python integers."""
    d = [int(v) for v in d]
    T = len(d)
    q_set = [q for q in range(max(1, t - w), min(T - 1, t + w) + 1) if q != t]
    c1 = d[t] * hist_thr[1] > hist_thr[0] * 2 * n
    c2 = int(sad[t]) * sad_thr[1] > sad_thr[0] * n
    c3 = all(d[q] < d[t] if q < t else d[q] <= d[t] for q in q_set)
    c4 = len(q_set) == 0 or d[t] * peak[1] * len(q_set) > peak[0] * sum(d[q] for q in q_set)
    return c1, c2, c3, c4


def cuts_from_distance(d, sad, n, **thr):
    """dict(cut uint8 (T,), shot int32 (T,), n_shots int) from d and sad."""
    T = len(d)
    cut = np.zeros(T, dtype=np.uint8)
    for t in range(1, T):
        cut[t] = 1 if all(conditions(d, sad, n, t, **thr)) else 0
    shot = np.cumsum(cut, dtype=np.int64).astype(np.int32)
    return dict(cut=cut, shot=shot, n_shots=int(shot[-1]) + 1 if T else 0)


def shot_cuts_ref(hist, sad, n, **thr):
    """dict(d uint32 (T,), cut, shot, n_shots) from the statistics."""
    d = hist_distance(hist)
    return dict(d=d, **cuts_from_distance(d, sad, n, **thr))


# ---- the synthetic clip ---------------------------------------------------------------------------------------------------------
def _tri(v, period):
    """Integer triangle wave in 0 .. period // 2."""
    return np.abs(v % period - period // 2)


def _scene(h, w, base, a1, a2, k):
    """An h x w picture in integers: two triangle waves of amplitudes a1, a2 and a little hash noise around ``base``."""
    y, x = np.mgrid[0:h, 0:w].astype(np.int64)
    noise = ((y * 73856093 + x * 19349663 + k * 83492791) >> 3) % 7 - 3
    return base + _tri((3 + k) * x + 2 * y, 64) * a1 // 32 + _tri(5 * y - (1 + k) * x, 48) * a2 // 24 + noise


def synthetic_clip(sh=48, sw=64):
    """uint8 (67, sh, sw) luma: a slow pan (1 pixel per frame), a hard cut at frame 20, a 12-frame cross-fade starting at frame 35, a
    one-frame +60 flash at frame 51, a hard cut at frame 57 into a fast pan (8 pixels per frame).  Integers only."""
    wide = sw + 96
    a, b, c, d = _scene(sh, wide, 40, 50, 30, 0), _scene(sh, wide, 150, 40, 50, 1), _scene(sh, wide, 95, 30, 40, 2), _scene(sh, wide, 175, 60, 20, 3)
    frames = []
    for t in range(67):
        if t < 20:
            f = a[:, t:t + sw]
        elif t < 35:
            f = b[:, :sw]
        elif t < 47:
            m = t - 34  # 1 .. 12
            f = (b[:, :sw] * (12 - m) + c[:, :sw] * m + 6) // 12
        elif t < 57:
            f = c[:, :sw] + (60 if t == 51 else 0)
        else:
            f = d[:, 8 * (t - 57):8 * (t - 57) + sw]
        frames.append(np.clip(f, 0, 255))
    return np.stack(frames).astype(np.uint8)


SYNTHETIC_CUTS = [20, 51, 57]


# ---- td_tube_densify_shots ------------------------------------------------------------------------------------------------------
def shot_of(shot, shot_t0, f):
    """The shot of frame number f; None - unknown, which matches every shot - outside the array or without one."""
    if shot is None:
        return None
    i = f - shot_t0
    return int(shot[i]) if 0 <= i < len(shot) else None


def one_shot(x, y):
    return x is None or y is None or x == y


def densify_shots_ref(boxes, T, row_frame=None, first=0, step=1, t0=0, span=None, heat=None, mode="lerp", smooth=0, shot=None, shot_t0=0):
    """densify_ref's result under the extensions 1', 2', 3', 4' and 7' of td_tube_densify_shots; ``shot`` is the int array of shot
    ids, entry i for frame number shot_t0 + i, or None."""
    out = densify_ref(boxes, T, row_frame=row_frame, first=first, step=step, t0=t0, span=span, heat=heat, mode=mode, smooth=smooth)
    if shot is None:
        return out
    boxes = np.asarray(boxes, dtype=np.float32)
    if boxes.ndim == 2:
        boxes = boxes[:, None, :]
    n_tube, K = boxes.shape[:2]
    rf = row_frames(n_tube, row_frame, first, step)
    present = presence(boxes, None if span is None else np.asarray(span, dtype=np.int64).reshape(K, 2))
    row_shot = [shot_of(shot, shot_t0, f) for f in rf]

    def working(r, k):  # 2': the window takes the present rows in row r's own shot
        mine = present.copy()
        for q in range(n_tube):
            if not one_shot(row_shot[q], row_shot[r]):
                mine[q, k] = False
        return working_box(boxes, mine, r, k, smooth)

    dense = np.full((T, K, 4), QNAN_BITS, dtype=np.uint32)
    valid = np.zeros((T, K), dtype=np.uint8)
    out_heat = None if heat is None else np.zeros((T,) + np.asarray(heat).shape[1:], dtype=np.uint8)
    with np.errstate(all="ignore"):
        for i in range(T):
            where = place(rf, t0 + i)
            if where is None:
                continue
            a, num, den = where
            sf = shot_of(shot, shot_t0, t0 + i)
            ia = num == 0 or one_shot(row_shot[a], sf)
            ib = num == 0 or one_shot(row_shot[a + 1], sf)
            for k in range(K):
                v = None
                pa = bool(present[a, k])
                if not (ia and ib):  # a cut between the frame and a row: the other row alone, in every mode
                    r = a if ia else a + 1 if ib else None
                    if r is not None and present[r, k]:
                        v = working(r, k)
                elif num == 0 or mode == "hold":
                    if pa:
                        v = working(a, k)
                else:
                    pb = bool(present[a + 1, k])
                    if pa and pb:
                        A, B = working(a, k), working(a + 1, k)
                        if mode == "lerp":
                            wgt = F32(F32(num) / F32(den))
                            v = [F32(A[c] + F32(wgt * F32(B[c] - A[c]))) for c in range(4)]
                        else:
                            v = [B[c] if B[c] < A[c] else A[c] for c in (0, 1)] + [B[c] if B[c] > A[c] else A[c] for c in (2, 3)]
                    elif mode == "hull" and (pa or pb):
                        v = working(a if pa else a + 1, k)
                if v is not None:  # 5
                    v = np.array(v, dtype=np.float32)
                    bits = v.view(np.uint32).copy()
                    bits[np.isnan(v)] = QNAN_BITS
                    dense[i, k] = bits
                    valid[i, k] = 1 if np.isfinite(v).all() else 0
            if heat is not None:  # 7'
                h = np.asarray(heat, dtype=np.uint8)
                if not (ia and ib):
                    out_heat[i] = h[a] if ia else h[a + 1] if ib else 0
                else:
                    out_heat[i] = out["heat"][i]
    return dict(dense=dense, valid=valid, span=out["span"], heat=out_heat)
