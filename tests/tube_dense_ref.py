"""numpy restatement of td_tube_densify's rule, written from the text in include/tubedetr_hip.h (not from the kernel): the
numbers in the comments are the rule's steps.  Every fp32 value is an ``np.float32`` scalar, so every operation rounds once
to fp32; every integer is a Python integer."""
import numpy as np

MODES = ("hold", "lerp", "hull")
QNAN_BITS = 0x7FC00000
MAX_DEN = 1 << 24
F32 = np.float32


def row_frames(n_tube, row_frame=None, first=0, step=1):
    """The frame number of every tube row, as Python integers."""
    if row_frame is not None:
        rf = [int(v) for v in row_frame]
        assert len(rf) == n_tube
        return rf
    return [first + r * step for r in range(n_tube)]


def place(rf, f):
    """3: (a, num, den) of frame number f; None: absent; num = 0: the frame sits on row a."""
    n = len(rf)
    if f < rf[0] or f > rf[n - 1]:
        return None
    lo, hi = 0, n - 1
    while lo < hi:
        mid = (lo + hi + 1) >> 1
        if rf[mid] <= f:
            lo = mid
        else:
            hi = mid - 1
    a = lo
    if f == rf[a]:
        return a, 0, 1
    if a + 1 >= n:
        return None
    num, den = f - rf[a], rf[a + 1] - rf[a]
    if den <= 0 or den > MAX_DEN or not 0 < num < den:
        return None
    return a, num, den


def presence(boxes, span):
    """1: bool (n_tube, K)."""
    n_tube, K = boxes.shape[:2]
    ok = np.isfinite(boxes).all(-1)
    if span is not None:
        r = np.arange(n_tube)[:, None]
        ok &= (r >= span[None, :, 0]) & (r <= span[None, :, 1])
    return ok


def working_box(boxes, present, r, k, w):
    """2: the four np.float32 of the working box of the present row r."""
    if w == 0:
        return [boxes[r, k, c] for c in range(4)]
    n_tube = boxes.shape[0]
    s, count = [F32(0.0)] * 4, 0
    for q in range(max(r - w, 0), min(r + w, n_tube - 1) + 1):
        if present[q, k]:
            s = [F32(s[c] + boxes[q, k, c]) for c in range(4)]
            count += 1
    return [F32(s[c] / F32(count)) for c in range(4)]


def densify_ref(boxes, T, row_frame=None, first=0, step=1, t0=0, span=None, heat=None, mode="lerp", smooth=0):
    """boxes (n_tube, 4) or (n_tube, K, 4).  Returns dict(dense=uint32 bit patterns (T, K, 4), valid=uint8 (T, K),
    span=int64 (K, 2), heat=uint8 (T, mh, mw) or None)."""
    assert mode in MODES
    boxes = np.asarray(boxes, dtype=np.float32)
    if boxes.ndim == 2:
        boxes = boxes[:, None, :]
    n_tube, K = boxes.shape[:2]
    if span is not None:
        span = np.asarray(span, dtype=np.int64).reshape(K, 2)
    rf = row_frames(n_tube, row_frame, first, step)
    present = presence(boxes, span)
    dense = np.full((T, K, 4), QNAN_BITS, dtype=np.uint32)  # 5: absent
    valid = np.zeros((T, K), dtype=np.uint8)
    out_heat = None
    if heat is not None:
        heat = np.asarray(heat, dtype=np.uint8)
        assert heat.shape[0] == n_tube
        out_heat = np.zeros((T,) + heat.shape[1:], dtype=np.uint8)
    with np.errstate(all="ignore"):
        for i in range(T):
            where = place(rf, t0 + i)
            if where is None:
                continue
            a, num, den = where
            for k in range(K):
                v = None
                pa = bool(present[a, k])
                if num == 0 or mode == "hold":  # 3: an exact hit; 4: HOLD
                    if pa:
                        v = working_box(boxes, present, a, k, smooth)
                else:
                    pb = bool(present[a + 1, k])
                    if pa and pb:
                        A, B = working_box(boxes, present, a, k, smooth), working_box(boxes, present, a + 1, k, smooth)
                        if mode == "lerp":
                            wgt = F32(F32(num) / F32(den))
                            v = [F32(A[c] + F32(wgt * F32(B[c] - A[c]))) for c in range(4)]
                        else:
                            v = [B[c] if B[c] < A[c] else A[c] for c in (0, 1)] + [B[c] if B[c] > A[c] else A[c] for c in (2, 3)]
                    elif mode == "hull" and (pa or pb):
                        v = working_box(boxes, present, a if pa else a + 1, k, smooth)
                if v is not None:  # 5
                    v = np.array(v, dtype=np.float32)
                    bits = v.view(np.uint32).copy()
                    bits[np.isnan(v)] = QNAN_BITS
                    dense[i, k] = bits
                    valid[i, k] = 1 if np.isfinite(v).all() else 0
            if heat is not None:  # 7
                qa = heat[a].astype(np.int64)
                if num == 0 or mode == "hold":
                    out_heat[i] = qa
                else:
                    qb = heat[a + 1].astype(np.int64)
                    out_heat[i] = (qa * (den - num) + qb * num + den // 2) // den if mode == "lerp" else np.maximum(qa, qb)
    dspan = np.empty((K, 2), dtype=np.int64)  # 6
    for k in range(K):
        s0, s1 = (0, n_tube - 1) if span is None else (max(int(span[k, 0]), 0), min(int(span[k, 1]), n_tube - 1))
        if s0 > s1:
            dspan[k] = (0, -1)
            continue
        d0, d1 = rf[s0] - t0, rf[s1] - t0
        if mode == "hull":
            if s0 > 0:
                d0 = rf[s0 - 1] + 1 - t0
            if s1 < n_tube - 1:
                d1 = rf[s1 + 1] - 1 - t0
        dspan[k] = (d0, d1)
    return dict(dense=dense, valid=valid, span=dspan, heat=out_heat)


def dense_floats(ref):
    """The reference's boxes as float32 (T, K, 4)."""
    return ref["dense"].view(np.float32)
