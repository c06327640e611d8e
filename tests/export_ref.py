"""numpy restatement of td_frame_export's rule (include/tubedetr_hip.h): stages A (area resize), B (yuv -> rgb), C (rgb -> yuv),
their composition by format pair, ``take``, padding and ``valid``.  Written from the header's comment alone; frames are the
tightly packed layouts of ``DecodedClip`` / ``DeviceFrames``."""
import numpy as np

FMTS = ("rgb24", "yuv420p", "nv12")
_YUV_COEF = {("bt601", False): (16, 76309, 104597, 25675, 53279, 132201), ("bt601", True): (0, 65536, 91881, 22553, 46802, 116130),
             ("bt709", False): (16, 76309, 117489, 13975, 34925, 138438), ("bt709", True): (0, 65536, 103206, 12276, 30679, 121609)}  # yo, cy, crv, cgu, cgv, cbu
_ONE = 1 << 20


def forward_coefficients(matrix, full_range):
    """round(2^20 x) rows for Y, U, V and the three offsets, from Kr, Kb and the range as the header gives them."""
    kr, kb = (0.299, 0.114) if matrix == "bt601" else (0.2126, 0.0722)
    kg = 1.0 - kr - kb
    sy, sc = (1.0, 1.0) if full_range else (219.0 / 255.0, 224.0 / 255.0)
    rows = ((kr * sy, kg * sy, kb * sy), (-kr / (2 * (1 - kb)) * sc, -kg / (2 * (1 - kb)) * sc, 0.5 * sc), (0.5 * sc, -kg / (2 * (1 - kr)) * sc, -kb / (2 * (1 - kr)) * sc))
    return [[round(_ONE * c) for c in r] for r in rows], (0 if full_range else 16, 128, 128), rows


# ---- A -------------------------------------------------------------------------------------------------------------------------
def weights(n, m):
    """w[j][i] = max(0, min((j + 1) n, (i + 1) m) - max(j n, i m)): int64 [m][n]."""
    j = np.arange(m, dtype=np.int64)[:, None]
    i = np.arange(n, dtype=np.int64)[None, :]
    return np.maximum(0, np.minimum((j + 1) * n, (i + 1) * m) - np.maximum(j * n, i * m))


def area_resize(plane, m_y, m_x):
    """plane: uint8 [n_y][n_x] or [n_y][n_x][C] -> uint8 [m_y][m_x](...)."""
    n_y, n_x = plane.shape[:2]
    assert 1 <= m_y <= n_y and 1 <= m_x <= n_x
    if plane.ndim == 3:  # channel by channel: the int64 copy of a large frame is large
        return np.stack([area_resize(plane[..., c], m_y, m_x) for c in range(plane.shape[2])], axis=-1)
    v = plane.astype(np.int64)
    S = np.tensordot(weights(n_y, m_y), v, axes=(1, 0))      # [m_y][n_x](C)
    S = np.tensordot(weights(n_x, m_x), S, axes=(1, 1))      # [m_x][m_y](C)
    S = np.swapaxes(S, 0, 1)
    D = n_y * n_x
    out = (S + (D >> 1)) // D
    assert out.min() >= 0 and out.max() <= 255
    return out.astype(np.uint8)


# ---- B -------------------------------------------------------------------------------------------------------------------------
def yuv_to_rgb(Y, U, V, matrix, full_range):
    """Y [h][w], U and V [(h+1)/2][(w+1)/2] -> rgb [h][w][3]; chroma sample (y >> 1, x >> 1)."""
    yo, cy, crv, cgu, cgv, cbu = _YUV_COEF[(matrix, bool(full_range))]
    h, w = Y.shape
    ys, xs = np.arange(h) >> 1, np.arange(w) >> 1
    c = Y.astype(np.int64) - yo
    d = U.astype(np.int64)[ys][:, xs] - 128
    e = V.astype(np.int64)[ys][:, xs] - 128
    r = (cy * c + crv * e + 32768) >> 16
    g = (cy * c - cgu * d - cgv * e + 32768) >> 16
    b = (cy * c + cbu * d + 32768) >> 16
    return np.clip(np.stack([r, g, b], axis=-1), 0, 255).astype(np.uint8)


# ---- C -------------------------------------------------------------------------------------------------------------------------
def chroma_from_sums(Rs, Gs, Bs, n, row, return_acc=False):
    """One of U, V from the sums over the n = 1, 2, 4 pixels of a block; ``row`` = the three integer coefficients."""
    lg = {1: 0, 2: 1, 4: 2}[int(n)] if np.isscalar(n) else np.log2(n).astype(np.int64)
    acc = row[0] * Rs + row[1] * Gs + row[2] * Bs + n * (_ONE * 128 + _ONE // 2)
    val = np.clip(acc >> (20 + lg), 0, 255)
    return (val, acc) if return_acc else val


def rgb_to_yuv(rgb, matrix, full_range):
    """rgb [h][w][3] -> Y [h][w], U, V [(h+1)/2][(w+1)/2]."""
    (ry, ru, rv), offs, _ = forward_coefficients(matrix, bool(full_range))
    h, w = rgb.shape[:2]
    p = rgb.astype(np.int64)
    Y = np.clip((ry[0] * p[..., 0] + ry[1] * p[..., 1] + ry[2] * p[..., 2] + _ONE * offs[0] + _ONE // 2) >> 20, 0, 255).astype(np.uint8)
    ch, cw = (h + 1) // 2, (w + 1) // 2
    padded = np.zeros((2 * ch, 2 * cw, 3), np.int64)
    padded[:h, :w] = p
    count = np.zeros((2 * ch, 2 * cw), np.int64)
    count[:h, :w] = 1
    sums = padded.reshape(ch, 2, cw, 2, 3).sum(axis=(1, 3))
    n = count.reshape(ch, 2, cw, 2).sum(axis=(1, 3))
    U = chroma_from_sums(sums[..., 0], sums[..., 1], sums[..., 2], n, ru).astype(np.uint8)
    V = chroma_from_sums(sums[..., 0], sums[..., 1], sums[..., 2], n, rv).astype(np.uint8)
    return Y, U, V


# ---- frames ----------------------------------------------------------------------------------------------------------------------
def frame_bytes(fmt, h, w):
    return 3 * h * w if fmt == "rgb24" else h * w + 2 * ((h + 1) // 2) * ((w + 1) // 2)


def unpack(frame, fmt, h, w):
    """One tightly packed frame -> rgb [h][w][3], or (Y, U, V)."""
    if fmt == "rgb24":
        return frame.reshape(h, w, 3)
    ch, cw = (h + 1) // 2, (w + 1) // 2
    Y = frame[:h * w].reshape(h, w)
    if fmt == "yuv420p":
        return Y, frame[h * w:h * w + ch * cw].reshape(ch, cw), frame[h * w + ch * cw:].reshape(ch, cw)
    uv = frame[h * w:].reshape(ch, cw, 2)
    return Y, uv[..., 0], uv[..., 1]


def pack(planes, fmt):
    if fmt == "rgb24":
        return np.ascontiguousarray(planes).reshape(-1)
    Y, U, V = planes
    if fmt == "yuv420p":
        return np.concatenate([Y.reshape(-1), U.reshape(-1), V.reshape(-1)])
    return np.concatenate([Y.reshape(-1), np.stack([U, V], axis=-1).reshape(-1)])


def _padded(plane, h, w, value):
    out = np.empty((h, w) + plane.shape[2:], np.uint8)
    out[...] = np.asarray(value, np.uint8)
    out[:plane.shape[0], :plane.shape[1]] = plane
    return out


def export_frame(frame, src_fmt, sh, sw, dst_fmt, oh, ow, dh, dw, pad, matrix="bt601", full_range=False):
    """One source frame (None: a blank frame) -> one tightly packed destination frame of dh x dw."""
    cdh, cdw = (dh + 1) // 2, (dw + 1) // 2
    if frame is None:
        if dst_fmt == "rgb24":
            return pack(_padded(np.zeros((0, 0, 3), np.uint8), dh, dw, pad), dst_fmt)
        z = np.zeros((0, 0), np.uint8)
        return pack((_padded(z, dh, dw, pad[0]), _padded(z, cdh, cdw, pad[1]), _padded(z, cdh, cdw, pad[2])), dst_fmt)
    src = unpack(frame, src_fmt, sh, sw)
    if src_fmt == "rgb24" or dst_fmt == "rgb24":
        rgb = src if src_fmt == "rgb24" else yuv_to_rgb(*src, matrix, full_range)
        pic = area_resize(rgb, oh, ow)
        if dst_fmt == "rgb24":
            return pack(_padded(pic, dh, dw, pad), dst_fmt)
        Y, U, V = rgb_to_yuv(pic, matrix, full_range)
    else:
        coh, cow = (oh + 1) // 2, (ow + 1) // 2
        Y, U, V = area_resize(src[0], oh, ow), area_resize(src[1], coh, cow), area_resize(src[2], coh, cow)
    return pack((_padded(Y, dh, dw, pad[0]), _padded(U, cdh, cdw, pad[1]), _padded(V, cdh, cdw, pad[2])), dst_fmt)


def export(data, src_fmt, T, sh, sw, dst_fmt, oh, ow, dh, dw, pad=(0, 0, 0), take=None, matrix="bt601", full_range=False):
    """data: uint8 [T * frame_bytes] -> (uint8 [To * frame_bytes(dst)], valid uint8 [To])."""
    fb = frame_bytes(src_fmt, sh, sw)
    take = list(range(T)) if take is None else [int(t) for t in take]
    out, valid, cache = [], [], {}
    for t in take:
        ok = 0 <= t < T
        key = t if ok else None
        if key not in cache:
            cache[key] = export_frame(data[t * fb:(t + 1) * fb] if ok else None, src_fmt, sh, sw, dst_fmt, oh, ow, dh, dw, pad, matrix, full_range)
        out.append(cache[key])
        valid.append(1 if ok else 0)
    flat = np.concatenate(out) if out else np.zeros(0, np.uint8)
    return flat, np.asarray(valid, np.uint8)
