"""How every wrapper of this package reads its arguments: one clip or a list of clips, per-clip lists, tensors on the clips'
device, the shape rules of tubes (boxes, K, span) and of ``out``.  Checks only: nothing here allocates on the device."""
from __future__ import annotations

import torch

from ..frame_jobs import MAX_RECTS
from .frames import DeviceFrames

_FRAMES = "frames: DeviceFrames on one device"


def _clips_of(frames, kinds=(DeviceFrames,), lists_only: bool = False):
    """(single, clips): one clip is a list of one.  ``lists_only``: whatever is no list or tuple is one clip."""
    single = isinstance(frames, kinds) or lists_only and not isinstance(frames, (list, tuple))
    return single, [frames] if single else list(frames)


def _device_of(clips):
    """The device of the first clip, which all of them share (``_check_clip``)."""
    if not isinstance(clips[0], DeviceFrames):
        raise ValueError(_FRAMES)
    return clips[0].data.device


def _check_clip(c, device):
    if not isinstance(c, DeviceFrames) or c.data.device != device:
        raise ValueError(_FRAMES)


def _as_list(v, n: int, name: str):
    if v is None:
        return [None] * n
    if isinstance(v, (list, tuple)):
        if len(v) != n:
            raise ValueError(f"{name}: {len(v)} entries for {n} clips")
        return list(v)
    if n != 1:
        raise ValueError(f"{name}: a list with one entry per clip")
    return [v]


def _per_clip(v, n: int, name: str, multi: bool):
    """A scalar serves every clip; with a list of clips, a list or tuple gives one value each."""
    return _as_list(v, n, name) if multi and isinstance(v, (list, tuple)) else [v] * n


def _dev_tensor(t, dtype, shape_tail, name, device):
    if t is None:
        return None
    ok = torch.is_tensor(t) and t.device == device and t.dtype == dtype
    if ok and shape_tail:
        ok = t.dim() >= len(shape_tail) and tuple(t.shape[t.dim() - len(shape_tail):]) == tuple(shape_tail)
    if not ok:
        raise ValueError(f"{name}: a {dtype} tensor [..., {', '.join(map(str, shape_tail))}] on {device}")
    return t.contiguous()


def _tube_tensors(b, s, h, m, T: int, device):
    """A clip's boxes fp32 [..., 4], span int64 [..., 2], heat uint8 and frame_map int32 [..., T] on ``device``, contiguous; None stays None."""
    return (_dev_tensor(b, torch.float32, (4,), "boxes", device), _dev_tensor(s, torch.int64, (2,), "span", device),
            _dev_tensor(h, torch.uint8, (), "heat", device), _dev_tensor(m, torch.int32, (T,), "frame_map", device))


def _boxes_K(b, text: str, rows: int = None) -> int:
    """K of a clip's boxes: (n, 4) hold one tube, (n, K, 4) hold K.  ``text`` refuses anything else (None too), boxes without a
    row and - with ``rows`` - boxes of another number of rows."""
    if b is None or b.dim() not in (2, 3) or (b.shape[0] < 1 if rows is None else b.shape[0] != rows):
        raise ValueError(text)
    return 1 if b.dim() == 2 else int(b.shape[1])


def _check_K(K: int, s, k_text: str) -> int:
    """K is in 1..MAX_RECTS (``k_text``, with ``{K}`` in it, refuses it), and the span is (2,) for one tube, (K, 2) for K."""
    if not 1 <= K <= MAX_RECTS:
        raise ValueError(k_text.format(K=K) + f": 1..{MAX_RECTS}")
    if s is not None and not (s.dim() == 1 and K == 1 or s.dim() == 2 and s.shape[0] == K):
        raise ValueError(f"span: (2,) for one tube, ({K}, 2) for {K}")
    return K


def _check_out(o, c: DeviceFrames, device):
    if o is not None and (not isinstance(o, DeviceFrames) or (o.T, o.h, o.w, o.pix_fmt) != (c.T, c.h, c.w, c.pix_fmt) or o.data.device != device):
        raise ValueError("out: DeviceFrames of the clip's geometry and pixel format on its device")
