"""Boxes that follow the object's pixels between sampled frames (td_tube_follow, csrc/tube_follow.hip): ``follow``."""
from __future__ import annotations

from typing import NamedTuple, Optional, Sequence, Tuple, Union

import torch

from .. import _hip
from ..frame_jobs import MAX_RECTS, _check_geometry, _describe, _int_in, _launch_pooled, _planes, _put_planes
from .clips import _as_list, _boxes_K, _check_clip, _check_K, _clips_of, _dev_tensor, _device_of, _per_clip
from .dense import MAX_DENSE_STEP, MAX_DENSE_T, MAX_FRAME_NO, DenseTubes
from .frames import DeviceFrames
from .shots import Shots

MAX_FOLLOW_RADIUS = 16
MAX_FOLLOW_REACH = 64
MAX_FOLLOW_ACCEPT = 1 << 20


class FollowedTubes(NamedTuple):
    """What ``follow`` returns for one clip; ``boxes`` go to ``annotate`` / ``annotate_tubes`` / ``crop_tubes`` / ``redact`` with
    frame_map = None."""
    boxes: torch.Tensor   # fp32 (T, 4) or (T, K, 4): the input's boxes, the accepted ones moved by their offset
    offset: torch.Tensor  # int32 (T, 2) or (T, K, 2): (dy, dx); (0, 0) where the box was copied or the match rejected
    cost: torch.Tensor    # int32 (T,) or (T, K) holding uint32: the best candidate's sum of 256 absolute luma differences
    status: torch.Tensor  # uint8 (T,) or (T, K): 0 copied, 1 accepted, 2 rejected


def _accept(v) -> Tuple[int, int]:
    """``accept`` of ``follow``: grey levels per sample, an integer or a (numerator, denominator) pair."""
    if isinstance(v, (tuple, list)):
        try:
            num, den = v
        except (TypeError, ValueError):
            raise ValueError(f"accept {v!r}: an integer, or two integers (numerator, denominator)") from None
    else:
        num, den = v, 1
    return _int_in("accept numerator", num, 0, MAX_FOLLOW_ACCEPT), _int_in("accept denominator", den, 1, MAX_FOLLOW_ACCEPT)


def _follow_what(radius, reach, accept):
    return (_int_in("radius", radius, 0, MAX_FOLLOW_RADIUS), _int_in("reach", reach, 1, MAX_FOLLOW_REACH)) + _accept(accept)


def follow_job(src: int, T: int, sh: int, sw: int, boxes: int, anchor: int, out: int, K: int = 1, pix_fmt: str = "rgb24", shot: Optional[int] = None, radius: int = 8,
               reach: int = 3, accept=24, offset: Optional[int] = None, cost: Optional[int] = None, status: Optional[int] = None,
               src_planes: Optional[Sequence[int]] = None, src_pitches: Optional[Sequence[int]] = None, src_frame_stride: Optional[int] = None):
    """One ``td_follow_job``: T frames of sh x sw in ``pix_fmt`` at device address ``src`` (planes, pitches and frame stride as in
    ``overlay_job``); ``boxes`` (fp32 [T][K][4]), ``anchor`` (bytes [T]) and ``out`` (fp32 [T][K][4]; may be ``boxes``) are device
    addresses, ``shot`` (int32 [T]), ``offset`` (int32 [T][K][2]), ``cost`` (uint32 [T][K]) and ``status`` (bytes [T][K]) device
    addresses or None.  ``accept`` is an integer or a (numerator, denominator) pair."""
    T, sh, sw, K = int(T), int(sh), int(sw), int(K)
    _check_geometry(pix_fmt, T, sh, sw)
    radius, reach, num, den = _follow_what(radius, reach, accept)
    if not 1 <= K <= MAX_RECTS:
        raise ValueError(f"K = {K}: 1..{MAX_RECTS} rectangles per frame")
    if not boxes or not anchor or not out:
        raise ValueError("boxes, anchor and out are device addresses, not None")
    fmt, tight, sizes = _planes(pix_fmt, sh, sw)
    j = _hip.FollowJob()
    _put_planes(j, "src", _describe(src, sizes, tight, src_planes, src_pitches, src_frame_stride))
    j.fmt, j.T, j.sh, j.sw, j.K = fmt, T, sh, sw, K
    j.boxes, j.anchor, j.shot = boxes, anchor, shot
    j.radius, j.reach, j.accept_num, j.accept_den = radius, reach, num, den
    j.out, j.offset, j.cost, j.status = out, offset, cost, status
    return j


def anchors(row_frame=None, first: int = 0, step: int = 1, T: Optional[int] = None, t0: int = 0, n_tube: Optional[int] = None, device=None) -> torch.Tensor:
    """The ``anchor`` vector of ``follow`` for the T dense frames t0 .. t0 + T - 1, uint8 (T,) on the device: 1 where the frame is
    a sampled one, whose boxes are the model's own.  The arguments are ``densify``'s: ``row_frame`` holds the frame number of every
    tube row (an int32 tensor on the device, or a host sequence of integers); None: row r was sampled at first + r * step, for
    r >= 0 (and r < ``n_tube``, when given).  A few torch operators, no synchronisation with a device table: this is not on the
    hot path - a caller with a fixed sampling pattern builds the vector once and keeps it."""
    T, t0 = _int_in("T", T, 0, MAX_DENSE_T), _int_in("t0", t0, -MAX_FRAME_NO, MAX_FRAME_NO)
    if row_frame is None:
        first, step = _int_in("first", first, -MAX_FRAME_NO, MAX_FRAME_NO), _int_in("step", step, 1, MAX_DENSE_STEP)
        if n_tube is not None:
            n_tube = _int_in("n_tube", n_tube, 1, MAX_DENSE_T)
    elif not torch.is_tensor(row_frame):
        row_frame = [_int_in("row_frame entry", v, -MAX_FRAME_NO, MAX_FRAME_NO) for v in row_frame]
    elif row_frame.dtype != torch.int32 or row_frame.dim() != 1 or not row_frame.is_cuda:
        raise ValueError("row_frame: an int32 (n_tube,) tensor on the device, or a host sequence of integers")
    if torch.is_tensor(row_frame):
        device = row_frame.device
    elif device is None:
        device = torch.device("cuda", torch.cuda.current_device())
    if row_frame is None:
        r = torch.arange(t0 - first, t0 - first + T, device=device)
        a = (r >= 0) & (r % step == 0)
        if n_tube is not None:
            a &= r < n_tube * step
        return a.to(torch.uint8)
    if not torch.is_tensor(row_frame):
        row_frame = torch.tensor(row_frame, dtype=torch.int32, device=device)
    i = row_frame.long() - t0
    a = torch.zeros(T + 1, dtype=torch.uint8, device=device)  # entry T takes the rows outside the T frames
    a[torch.where((i >= 0) & (i < T), i, torch.full_like(i, T))] = 1
    return a[:T]


def follow(frames: Union[DeviceFrames, Sequence[DeviceFrames]], boxes, anchor, shots=None, radius=8, reach=3, accept=24, in_place: bool = False):
    """Move the boxes of the frames between two sampled ones onto the object they belong to, by block matching in the decoded
    frames' luma: ONE launch for one clip or for a list of clips (``boxes``, ``anchor`` and ``shots`` are then lists too;
    ``radius``, ``reach`` and ``accept`` may be lists or one value for all).  Per clip:
      boxes    fp32 (T, 4) or (T, K, 4) xyxy on the device, one row per decoded frame, or the ``DenseTubes`` that ``densify``
               returned (four NaNs: no box);
      anchor   uint8 or bool (T,) on the device: non-zero where the frame's boxes are the model's own (``anchors`` makes it);
      shots    what ``shot_cuts`` returned for the clip (a ``Shots``) or its int32 (T,) tensor: no frame is matched against an
               anchor in another shot; None: one shot;
      radius   0..16 pixels searched around the interpolated position; reach 1..64 frames searched for an anchor;
      accept   the largest mean absolute luma difference per sample, in grey levels, at which a match moves the box: an integer
               or a (numerator, denominator) pair.  24 is a starting value that nobody has tried on real footage;
      in_place write into ``boxes`` (a contiguous tensor) instead of a new one: anchor boxes are never changed.
    A frame is matched against the nearest anchor frame (never against its neighbour: nothing drifts), translation only, on a
    16 x 16 grid of samples inside the anchor box; a rejected match leaves the interpolated box.  The rule is integers and stated in
    include/tubedetr_hip.h.  Returns ``FollowedTubes`` (a list for a list), whose boxes go to ``annotate`` / ``annotate_tubes`` /
    ``crop_tubes`` / ``redact`` with frame_map = None.  Nothing here synchronises or copies to the host, and bad arguments are
    refused before the device is touched."""
    single, clips = _clips_of(frames, lists_only=True)
    n = len(clips)
    if n == 0:
        return []
    # (a tuple is ONE accept value, the pair: only a list, for a list of clips, gives one value each)
    accept_l = _per_clip(accept, n, "accept", not single and isinstance(accept, list))
    what = [_follow_what(*v) for v in zip(_per_clip(radius, n, "radius", not single), _per_clip(reach, n, "reach", not single), accept_l)]
    device = _device_of(clips)  # (the scalars' refusals came first: they are the same on a host without a device)
    # (a DenseTubes and a Shots are tuples themselves: one clip takes them as they are)
    boxes_l, anchor_l, shots_l = ([boxes], [anchor], [shots]) if single else (_as_list(v, n, k) for v, k in ((boxes, "boxes"), (anchor, "anchor"), (shots, "shots")))
    prepared = []
    for c, b, a, s in zip(clips, boxes_l, anchor_l, shots_l):  # every refusal comes before the first allocation and the launch
        _check_clip(c, device)
        given = b.boxes if isinstance(b, DenseTubes) else b
        b = _dev_tensor(given, torch.float32, (4,), "boxes", device)
        K = _check_K(_boxes_K(b, f"boxes: ({c.T}, 4) or ({c.T}, K, 4), one row per frame of the clip", c.T), None, "boxes carry K = {K} rectangles per frame")
        if in_place and b is not given:
            raise ValueError("in_place: boxes must be a contiguous tensor")
        if torch.is_tensor(a) and a.dtype == torch.bool:
            a = a.view(torch.uint8)
        a = _dev_tensor(a, torch.uint8, (c.T,), "anchor", device)
        if a is None or a.dim() != 1:
            raise ValueError(f"anchor: a uint8 or bool ({c.T},) tensor on the device")
        s = _dev_tensor(s.shot if isinstance(s, Shots) else s, torch.int32, (c.T,), "shots", device)
        if s is not None and s.dim() != 1:
            raise ValueError(f"shots: a Shots, or an int32 ({c.T},) tensor of shot ids")
        prepared.append((c, b, a, s, K))
    jobs, keep, results = [], [], []
    for (c, b, a, s, K), (radius_i, reach_i, num, den) in zip(prepared, what):
        T = c.T
        out = b if in_place else torch.empty_like(b)
        words = torch.empty(max(T, 1) * K * 3, dtype=torch.int32, device=device)  # (T = 0 still has an address)
        status = torch.empty(max(T, 1) * K, dtype=torch.uint8, device=device)
        if T > 0:  # (a clip without frames has no bytes, and its tensors no address: it is no job)
            jobs.append(follow_job(c.data.data_ptr(), T, c.h, c.w, b.data_ptr(), a.data_ptr(), out.data_ptr(), K, c.pix_fmt, _hip.ptr(s), radius_i, reach_i, (num, den),
                                   words.data_ptr(), words.data_ptr() + 8 * T * K, status.data_ptr()))
            keep.append((c.data, b, a, s))
        one = b.dim() == 2
        results.append(FollowedTubes(out, words[:2 * T * K].view((T, 2) if one else (T, K, 2)), words[2 * T * K:3 * T * K].view((T,) if one else (T, K)),
                                     status[:T * K].view((T,) if one else (T, K))))
    return _launch_pooled("td_tube_follow", jobs, keep, results, single, device)
