"""Grounded tubes interpolated to every decoded frame (td_tube_densify, td_tube_densify_shots, csrc/tube_dense.hip): ``densify``."""
from __future__ import annotations

from typing import NamedTuple, Optional, Tuple

import torch

from .. import _hip
from ..frame_jobs import MAX_MAP, MAX_RECTS, _grid_ok, _heat_grid, _int_in, _launch_pooled
from .clips import _as_list, _dev_tensor, _boxes_K, _check_K, _per_clip, _tube_tensors
from .shots import Shots

DENSE_MODES = ("hold", "lerp", "hull")
MAX_SMOOTH = 16
MAX_DENSE_T = 1 << 20
MAX_FRAME_NO = 1 << 23
MAX_DENSE_STEP = 1 << 16


class DenseTubes(NamedTuple):
    """What ``densify`` returns for one clip: the tube at the decoded rate.  An absent box is four NaNs, which ``annotate``,
    ``crop_tubes`` and ``redact`` take as "no box": pass ``boxes`` (and ``heat``) with frame_map = None."""
    boxes: torch.Tensor           # fp32 (T, 4) or (T, K, 4)
    span: torch.Tensor            # int64 (2,) or (K, 2): first and last dense frame of the span (``annotate``'s dim layer)
    valid: torch.Tensor           # bool (T,) or (T, K): False where the box is absent or not finite
    heat: Optional[torch.Tensor]  # uint8 (T, mh, mw), or None


def _dense_what(T, t0, first, step, mode, smooth, has_table: bool):
    if mode not in DENSE_MODES:
        raise ValueError(f"mode {mode!r}: one of {DENSE_MODES}")
    T, t0 = _int_in("T", T, 0, MAX_DENSE_T), _int_in("t0", t0, -MAX_FRAME_NO, MAX_FRAME_NO)
    if has_table:
        first, step = 0, 1
    else:
        first, step = _int_in("first", first, -MAX_FRAME_NO, MAX_FRAME_NO), _int_in("step", step, 1, MAX_DENSE_STEP)
    return T, t0, first, step, DENSE_MODES.index(mode), _int_in("smooth", smooth, 0, MAX_SMOOTH)


def dense_job(boxes: int, n_tube: int, T: int, dense: int, K: int = 1, span: Optional[int] = None, row_frame: Optional[int] = None, first: int = 0, step: int = 1,
              t0: int = 0, heat: Optional[int] = None, heat_hw: Tuple[int, int] = (0, 0), mode: str = "lerp", smooth: int = 0, valid: Optional[int] = None,
              dense_span: Optional[int] = None, dense_heat: Optional[int] = None):
    """One ``td_dense_job``: the tube ``boxes`` (fp32 [n_tube][K][4]) sampled at the frame numbers ``row_frame`` (int32 [n_tube];
    None: row r at first + r step) interpolated to the T frames t0 .. t0 + T - 1 into ``dense`` (fp32 [T][K][4]).  ``span`` (int64
    [K][2]), ``heat`` (uint8 [n_tube][heat_hw[0]][heat_hw[1]]), ``valid`` (bytes [T][K]), ``dense_span`` (int64 [K][2]) and
    ``dense_heat`` (uint8 [T][mh][mw], with ``heat``) are device addresses or None."""
    n_tube, K = int(n_tube), int(K)
    T, t0, first, step, code, smooth = _dense_what(T, t0, first, step, mode, smooth, row_frame is not None)
    if n_tube < 1:
        raise ValueError(f"n_tube = {n_tube}: at least one tube row")
    if not 1 <= K <= MAX_RECTS:
        raise ValueError(f"K = {K}: 1..{MAX_RECTS} rectangles per tube row")
    if not boxes or not dense:
        raise ValueError("boxes and dense are device addresses, not None")
    if (heat is None) != (dense_heat is None):
        raise ValueError("heat and dense_heat come together")
    mh, mw = _heat_grid(heat_hw, heat is not None)
    j = _hip.DenseJob()
    j.boxes, j.span, j.row_frame, j.heat = boxes, span, row_frame, heat
    j.n_tube, j.K, j.T, j.t0, j.first, j.step, j.mode, j.smooth, j.mh, j.mw = n_tube, K, T, t0, first, step, code, smooth, mh, mw
    j.dense, j.valid, j.dense_span, j.dense_heat = dense, valid, dense_span, dense_heat
    return j


def densify(boxes, T, row_frame=None, first=0, step=1, t0=0, span=None, heat=None, mode: str = "lerp", smooth=0, shots=None, shots_t0=0):
    """Interpolate grounded tubes from the sampled frames to every decoded frame: ONE launch for one clip or for a list of
    clips (``boxes`` a list: ``row_frame``, ``span`` and ``heat`` are then lists too, or None, and ``T``, ``first``, ``step``,
    ``t0``, ``mode`` and ``smooth`` may be lists or one value for all).  Per clip:
      boxes      fp32 (n_tube, 4) or (n_tube, K, 4) xyxy on the device: what ``PostProcess`` returned, one row per sampled frame;
      T, t0      dense frame i of T has frame number t0 + i (a long video is done in chunks);
      row_frame  the frame number of every tube row, increasing: an int32 (n_tube,) tensor on the device, or a host sequence of
                 integers (uploaded with the job table, asynchronously); None: row r was sampled at first + r * step;
      span       int64 (2,) or (K, 2) tube rows, as ``redact`` takes them; None: all rows;
      heat       uint8 (n_tube, mh, mw) from ``heat_from_attention``; None: no maps;
      mode       "hold" (what a frame_map does), "lerp" (straight lines between two rows) or "hull" (the cover of both rows: for ``redact``);
      smooth     a radius in tube rows, 0..16: every row becomes the mean of the present rows around it first;
      shots      what ``shot_cuts`` returned for the clip (a ``Shots``), or its int32 (n,) shot id per frame on the device, entry i
                 for frame number ``shots_t0`` + i (a list of either, or of None, for a list of clips): the tube stops at the
                 cuts (``td_tube_densify_shots``) - no box is interpolated, smoothed or covered across one, the row on the frame's
                 own side of a cut stands alone.  Frames outside the array match every shot, so every chunk of a long video takes
                 the whole video's array.  None: the call is what it was.
    The rule is exact - numpy float32 reproduces every bit - and stated in include/tubedetr_hip.h.  Returns ``DenseTubes`` (a
    list for a list), whose boxes, span and heat go to ``annotate`` / ``crop_tubes`` / ``redact`` with frame_map = None.  Nothing
    here synchronises or copies to the host, and bad arguments are refused before the device is touched."""
    multi = isinstance(boxes, (list, tuple))
    clips = list(boxes) if multi else [boxes]
    n = len(clips)
    if n == 0:
        return []
    if multi:
        frames_l, span_l, heat_l = (_as_list(v, n, k) for v, k in ((row_frame, "row_frame"), (span, "span"), (heat, "heat")))
    else:
        frames_l, span_l, heat_l = [row_frame], [span], [heat]
    scalars = [_per_clip(v, n, k, multi) for v, k in ((T, "T"), (t0, "t0"), (first, "first"), (step, "step"), (mode, "mode"), (smooth, "smooth"))]
    if shots is None:
        shots_l = None
    else:
        shots_l = _as_list(shots, n, "shots") if multi else [shots]
        shots_l = [sh.shot if isinstance(sh, Shots) else sh for sh in shots_l]
        shots_t0_l = [_int_in("shots_t0", v, -MAX_FRAME_NO, MAX_FRAME_NO) for v in _per_clip(shots_t0, n, "shots_t0", multi)]
    if not torch.is_tensor(clips[0]) or not clips[0].is_cuda:
        # the scalars' refusals do not need a device: give them first, so that they are the same on a host without one
        for i in range(n):
            _dense_what(*(s[i] for s in scalars), has_table=frames_l[i] is not None)
        raise ValueError("boxes: a torch.float32 tensor (n_tube, 4) or (n_tube, K, 4) on the device per clip")
    device = clips[0].device
    prepared = []
    for i, (b, f, s, h) in enumerate(zip(clips, frames_l, span_l, heat_l)):  # every refusal comes before the first allocation and the launch
        Ti, t0i, firsti, stepi, _, smoothi = _dense_what(*(sc[i] for sc in scalars), has_table=f is not None)
        b, s, h, _ = _tube_tensors(b, s, h, None, 0, device)
        K = _check_K(_boxes_K(b, "boxes (n_tube, 4) or (n_tube, K, 4) with n_tube >= 1"), s, "boxes carry K = {K} rectangles per tube row")
        n_tube = int(b.shape[0])
        if h is not None and (h.dim() != 3 or h.shape[0] != n_tube or not _grid_ok(h.shape[1], h.shape[2])):
            raise ValueError(f"heat: uint8 ({n_tube}, mh, mw) with mh and mw in 1..{MAX_MAP}")
        if torch.is_tensor(f):
            f = _dev_tensor(f, torch.int32, (n_tube,), "row_frame", device)
            if f.dim() != 1:
                raise ValueError(f"row_frame: int32 ({n_tube},)")
        elif f is not None:
            f = [_int_in("row_frame entry", v, -MAX_FRAME_NO, MAX_FRAME_NO) for v in f]
            if len(f) != n_tube:
                raise ValueError(f"row_frame has {len(f)} entries for {n_tube} tube rows")
        if shots_l is not None and shots_l[i] is not None:
            sh = shots_l[i] = _dev_tensor(shots_l[i], torch.int32, (), "shots", device)
            if sh.dim() != 1 or sh.numel() > MAX_DENSE_T:
                raise ValueError(f"shots: a Shots, or an int32 (n,) tensor of shot ids with n <= {MAX_DENSE_T}")
        prepared.append((b, f, s, h, n_tube, K, Ti, i))
    jobs, keep, results, uploads = [], [], [], []
    for b, f, s, h, n_tube, K, Ti, i in prepared:
        dense = torch.empty(max(Ti, 1) * K * 4, dtype=torch.float32, device=device)[:Ti * K * 4]  # (T = 0 still has an address)
        valid = torch.empty(max(Ti, 1) * K, dtype=torch.bool, device=device)[:Ti * K]
        dspan = torch.empty((K, 2), dtype=torch.int64, device=device)
        dheat = None
        if h is not None:
            mb = int(h.shape[1] * h.shape[2])
            dheat = torch.empty(max(Ti, 1) * mb, dtype=torch.uint8, device=device)[:Ti * mb]
        table = f if torch.is_tensor(f) else None
        j = dense_job(b.data_ptr(), n_tube, Ti, dense.data_ptr(), K, _hip.ptr(s), _hip.ptr(table), scalars[2][i], scalars[3][i], scalars[1][i], _hip.ptr(h),
                      tuple(h.shape[1:]) if h is not None else (0, 0), scalars[4][i], scalars[5][i], valid.data_ptr(), dspan.data_ptr(), _hip.ptr(dheat))
        if f is not None and table is None:  # a host sequence: it travels with the table, and the launch puts its address into the job
            uploads.append((j, "row_frame", torch.tensor(f, dtype=torch.int32)))
        jobs.append(j)
        keep.append((b, s, h, table, shots_l[i] if shots_l is not None else None))
        one = b.dim() == 2
        results.append(DenseTubes(dense.view(Ti, 4) if one else dense.view(Ti, K, 4), dspan.view(2) if one else dspan, valid.view(Ti) if one else valid.view(Ti, K),
                                  dheat.view(Ti, h.shape[1], h.shape[2]) if h is not None else None))
    if shots_l is None:
        return _launch_pooled("td_tube_densify", jobs, keep, results, not multi, device, uploads)
    sarr = (_hip.DenseShots * n)(*[_hip.DenseShots(_hip.ptr(sh), t, sh.numel() if sh is not None else 0) for sh, t in zip(shots_l, shots_t0_l)])
    return _launch_pooled("td_tube_densify_shots", jobs, keep, results, not multi, device, uploads, (sarr,))
