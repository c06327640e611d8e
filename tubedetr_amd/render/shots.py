"""Shot cuts in decoded frames (td_frame_stats, td_shot_cuts, csrc/frame_stats.hip): ``frame_stats`` and ``shot_cuts``."""
from __future__ import annotations

from typing import NamedTuple, Optional, Sequence, Union

import torch

from .. import _hip
from ..frame_jobs import _check_geometry, _describe, _fraction, _int_in, _launch_pooled, _planes, _put_planes
from .clips import _check_clip, _clips_of, _device_of
from .frames import DeviceFrames

STAT_BINS = 64
MAX_STAT_STEP = 8
MAX_STAT_PIXELS = 1 << 24
MAX_CUT_T = 1 << 20
MAX_CUT_WINDOW = 16
MAX_CUT_FRACTION = 1 << 20


class FrameStats(NamedTuple):
    """What ``frame_stats`` returns for one clip."""
    hist: torch.Tensor  # int32 (T, 64) holding the uint32 counts: sampled pixels of frame t with luma >> 2 == b
    sad: torch.Tensor   # int32 (T,) holding the uint32 sums: |luma_t - luma_(t-1)| over the sampled pixels; 0 for frame 0, and for a repeated frame
    n: int              # sampled pixels per frame


class Shots(NamedTuple):
    """What ``shot_cuts`` returns for one clip; ``densify(..., shots=...)`` takes it."""
    cut: torch.Tensor    # bool (T,): frame t is the first of a new shot
    shot: torch.Tensor   # int32 (T,): the shot of frame t, counted from 0
    count: torch.Tensor  # int32 (1,) on the device: the number of shots
    d: torch.Tensor      # int32 (T,) holding uint32: the histogram distance to the frame before


def sampled_pixels(sh: int, sw: int, step: int = 1) -> int:
    """N of td_frame_stats: the pixels (y, x) with y % step == 0 and x % step == 0."""
    return ((sh + step - 1) // step) * ((sw + step - 1) // step)


def _stats_what(sh, sw, step):
    step = _int_in("step", step, 1, MAX_STAT_STEP)
    if sh * sw > MAX_STAT_PIXELS:
        raise ValueError(f"frame size {sh} x {sw}: at most {MAX_STAT_PIXELS} pixels (the sum of differences is 32 bits wide)")
    return step


def stats_job(src: int, T: int, sh: int, sw: int, pix_fmt: str = "rgb24", step: int = 1, hist: Optional[int] = None, sad: Optional[int] = None,
              src_planes: Optional[Sequence[int]] = None, src_pitches: Optional[Sequence[int]] = None, src_frame_stride: Optional[int] = None):
    """One ``td_stats_job``: T frames of sh x sw in ``pix_fmt`` at device address ``src`` (planes, pitches and frame stride as in
    ``overlay_job``), every ``step``-th pixel of every ``step``-th row; ``hist`` (uint32 [T][64]) and ``sad`` (uint32 [T]) are
    device addresses, one of them may be None."""
    T, sh, sw = int(T), int(sh), int(sw)
    _check_geometry(pix_fmt, T, sh, sw)
    step = _stats_what(sh, sw, step)
    if not hist and not sad:
        raise ValueError("hist and sad are device addresses: at least one of them")
    fmt, tight, sizes = _planes(pix_fmt, sh, sw)
    j = _hip.StatsJob()
    _put_planes(j, "src", _describe(src, sizes, tight, src_planes, src_pitches, src_frame_stride))
    j.fmt, j.T, j.sh, j.sw, j.step = fmt, T, sh, sw, step
    j.hist, j.sad = hist, sad
    return j


def _cuts_what(hist, sad, peak, window):
    return _fraction("hist", hist, MAX_CUT_FRACTION) + _fraction("sad", sad, MAX_CUT_FRACTION) + _fraction("peak", peak, MAX_CUT_FRACTION) + (_int_in("window", window, 0, MAX_CUT_WINDOW),)


def cuts_job(hist: int, sad: int, T: int, n: int, cut: int, shot: int, n_shots: int, d: Optional[int] = None, hist_thr=(1, 4), sad_thr=(8, 1), peak=(3, 1),
             window: int = 4):
    """One ``td_cuts_job``: the statistics ``hist`` (uint32 [T][64]) and ``sad`` (uint32 [T]) of T frames of ``n`` sampled pixels
    decided into ``cut`` (bytes [T]), ``shot`` (int32 [T]), ``n_shots`` (int32 [1]) and, optionally, ``d`` (uint32 [T]): device
    addresses.  The thresholds are (numerator, denominator) pairs, ``window`` the peak test's radius in frames."""
    T, n = _int_in("T", T, 0, MAX_CUT_T), _int_in("n", n, 1, MAX_STAT_PIXELS)
    what = _cuts_what(hist_thr, sad_thr, peak, window)
    if not (hist and sad and cut and shot and n_shots):
        raise ValueError("hist, sad, cut, shot and n_shots are device addresses, not None")
    j = _hip.CutsJob()
    j.hist, j.sad, j.T, j.N = hist, sad, T, n
    j.hist_num, j.hist_den, j.sad_num, j.sad_den, j.peak_num, j.peak_den, j.w = what
    j.d, j.cut, j.shot, j.n_shots = d, cut, shot, n_shots
    return j


def frame_stats(frames: Union[DeviceFrames, Sequence[DeviceFrames]], step: int = 1):
    """A luma histogram per frame and the sum of absolute luma differences to the frame before, read from the decoded planes in
    ONE launch for one clip or for a list of clips (mixed sizes and formats).  ``step`` in 1..8 takes every ``step``-th pixel of
    every ``step``-th row, and the bytes read fall with it.  The rule is integers and stated in include/tubedetr_hip.h; a long
    video done in chunks overlaps them by one frame.  Returns ``FrameStats`` (a list for a list).  Nothing here synchronises or
    copies to the host, and bad arguments are refused before the device is touched."""
    single, clips = _clips_of(frames)
    if not clips:
        return []
    device = _device_of(clips)
    for c in clips:  # every refusal comes before the first allocation and the launch
        _check_clip(c, device)
        _stats_what(c.h, c.w, step)
    jobs, keep, results = [], [], []
    for c in clips:
        out = torch.empty(max(c.T, 1) * (STAT_BINS + 1), dtype=torch.int32, device=device)  # (T = 0 still has an address)
        hist, sad = out[:c.T * STAT_BINS], out[c.T * STAT_BINS:c.T * (STAT_BINS + 1)]
        if c.T > 0:  # (a clip without frames has no bytes, and its tensor no address: it is no job)
            jobs.append(stats_job(c.data.data_ptr(), c.T, c.h, c.w, c.pix_fmt, step, out.data_ptr(), out.data_ptr() + 4 * c.T * STAT_BINS))
            keep.append((c.data,))
        results.append(FrameStats(hist.view(c.T, STAT_BINS), sad, sampled_pixels(c.h, c.w, step)))
    return _launch_pooled("td_frame_stats", jobs, keep, results, single, device)


def shot_cuts(frames_or_stats, step: int = 1, hist=(1, 4), sad=(8, 1), peak=(3, 1), window: int = 4):
    """Where the hard cuts of decoded clips are: ``frames_or_stats`` is a ``DeviceFrames`` (``frame_stats`` with ``step`` runs
    first), a ``FrameStats``, or a list of either kind.  Frame t starts a new shot when its histogram distance d[t] to the frame
    before exceeds ``hist`` = (num, den) of its maximum 2 n, its sum of differences exceeds ``sad`` = (num, den) grey levels per
    sampled pixel, and d[t] is the first largest value within ``window`` frames and more than ``peak`` = (num, den) times the
    mean of the others there - the rule, in integers, is stated in include/tubedetr_hip.h.  A one-frame flash gives one cut, at
    its first frame; fades and wipes give none.  The defaults are starting values tried on synthetic clips only: no footage has
    validated them.  Returns ``Shots`` (a list for a list); nothing synchronises, ``Shots.count`` stays on the device."""
    single, items = _clips_of(frames_or_stats, (DeviceFrames, FrameStats))
    if len(items) == 0:
        return []
    _cuts_what(hist, sad, peak, window)
    if all(isinstance(v, DeviceFrames) for v in items):
        _int_in("step", step, 1, MAX_STAT_STEP)
        items = frame_stats(items, step)
    prepared = []
    for v in items:  # every refusal comes before the first allocation and the launch
        if not isinstance(v, FrameStats):
            raise ValueError("frames_or_stats: DeviceFrames or FrameStats, one kind per call")
        h, s = v.hist, v.sad
        if not (torch.is_tensor(h) and torch.is_tensor(s) and h.is_cuda and s.device == h.device and h.dtype == torch.int32 and s.dtype == torch.int32
                and h.dim() == 2 and h.shape[1] == STAT_BINS and s.dim() == 1 and s.shape[0] == h.shape[0]):
            raise ValueError(f"FrameStats: hist int32 (T, {STAT_BINS}) and sad int32 (T,) on the device")
        if h.device != items[0].hist.device:
            raise ValueError("frames_or_stats: statistics on one device")
        prepared.append((h.contiguous(), s.contiguous(), _int_in("T", h.shape[0], 0, MAX_CUT_T), _int_in("FrameStats.n", v.n, 1, MAX_STAT_PIXELS)))
    device = prepared[0][0].device
    jobs, keep, results = [], [], []
    for h, s, T, n in prepared:
        words = torch.empty(2 * max(T, 1) + 1, dtype=torch.int32, device=device)
        flags = torch.empty(max(T, 1), dtype=torch.bool, device=device)
        d, shot, count = words[:T], words[max(T, 1):max(T, 1) + T], words[2 * max(T, 1):]
        # (a tensor without elements has no address: T = 0 still hands addresses over, and none of them is read or written but n_shots)
        jobs.append(cuts_job(h.data_ptr() or words.data_ptr(), s.data_ptr() or words.data_ptr(), T, n, flags.data_ptr(), words.data_ptr() + 4 * max(T, 1),
                             words.data_ptr() + 8 * max(T, 1), words.data_ptr(), hist, sad, peak, window))
        keep.append((h, s))
        results.append(Shots(flags[:T], shot, count, d))
    return _launch_pooled("td_shot_cuts", jobs, keep, results, single, device)
