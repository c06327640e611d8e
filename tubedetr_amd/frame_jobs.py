"""What the frame-job wrappers share on the Python side: the counterpart of csrc/frame_jobs.h.

A frame-job kernel (td_tube_overlay, td_tube_overlay_multi, td_tube_crop, td_tube_redact, td_tube_densify and its shot-cut
variant, td_frame_stats, td_shot_cuts, td_tube_follow, td_frame_export, and the two resamplers of csrc/augment.hip) takes an
array of job records and a (pinned, device) pair of table buffers.  Here are, once each: the pixel formats and the geometry of
their planes, the description of a plane set in a job record, the checks of the scalars that several records carry, the pool of
table pairs, the two ways to launch (fresh tables, pooled tables) and the raw launchers.  ``tubedetr_amd.render``,
``tubedetr_amd.augment`` and ``tubedetr_amd.models.postprocessors`` build on it; nothing here touches the library at import time."""
from __future__ import annotations

from typing import List, Sequence, Tuple

import torch

from . import _hip

_PIX_FMTS = ("rgb24", "yuv420p", "nv12")
_MATRICES = ("bt601", "bt709")
MAX_SIDE = 16384
MAX_MAP = 256
MAX_RECTS = 8
MAX_MARGIN_DEN = 1024


# ---- scalars that several job records carry ------------------------------------------------------------------------------------
def _rgb3(name: str, c) -> Tuple[int, int, int]:
    c = tuple(c)
    if len(c) != 3 or any(int(v) != v or not 0 <= v <= 255 for v in c):
        raise ValueError(f"{name} {c!r}: three integers in 0..255")
    return tuple(int(v) for v in c)


def _alpha(name: str, a) -> int:
    if int(a) != a or not 0 <= a <= 256:
        raise ValueError(f"{name} {a!r}: an integer in [0, 256]")
    return int(a)


def _int_in(name: str, v, lo: int, hi: int) -> int:
    try:
        ok = not isinstance(v, bool) and int(v) == v and lo <= int(v) <= hi
    except (TypeError, ValueError):
        ok = False
    if not ok:
        raise ValueError(f"{name} = {v!r}: an integer in {lo}..{hi}")
    return int(v)


def _fraction(name: str, v, hi: int) -> Tuple[int, int]:
    try:
        num, den = v
    except (TypeError, ValueError):
        raise ValueError(f"{name} {v!r}: two integers (numerator, denominator)") from None
    return _int_in(name + " numerator", num, 0, hi), _int_in(name + " denominator", den, 1, hi)


def _check_margin(num: int, den: int):
    if not 1 <= den <= MAX_MARGIN_DEN:
        raise ValueError(f"margin denominator {den}: 1..{MAX_MARGIN_DEN}")
    if not 0 <= num <= 4 * den:
        raise ValueError(f"margin {num}/{den}: between 0 and 4")


def _grid_ok(mh: int, mw: int) -> bool:
    """The sides of a heat map (the decoder's token grid)."""
    return 1 <= mh <= MAX_MAP and 1 <= mw <= MAX_MAP


def _heat_grid(hw, present: bool = True) -> Tuple[int, int]:
    mh, mw = int(hw[0]), int(hw[1])
    if present and not _grid_ok(mh, mw):
        raise ValueError(f"token grid {mh} x {mw}: sides in 1..{MAX_MAP}")
    return mh, mw


def _thickness(v) -> int:
    if int(v) != v or v < 1:
        raise ValueError(f"thickness {v!r}: an integer >= 1")
    return int(v)


# ---- frames: formats, plane geometry, and their description in a job record ---------------------------------------------------
def _frame_bytes(pix_fmt: str, h: int, w: int) -> int:
    if pix_fmt == "rgb24":
        return 3 * w * h
    return w * h + 2 * ((w + 1) // 2) * ((h + 1) // 2)


def _check_geometry(pix_fmt: str, T: int, h: int, w: int):
    if pix_fmt not in _PIX_FMTS:
        raise ValueError(f"pix_fmt {pix_fmt!r}: one of {_PIX_FMTS}")
    if T < 0:
        raise ValueError(f"T = {T} is negative")
    if not (1 <= h <= MAX_SIDE and 1 <= w <= MAX_SIDE):
        raise ValueError(f"frame size {h} x {w}: sides in 1..{MAX_SIDE}")


def _planes(pix_fmt: str, sh: int, sw: int):
    """(fmt code, tight pitches, plane sizes) of one frame."""
    ch, cw = (sh + 1) // 2, (sw + 1) // 2
    if pix_fmt == "rgb24":
        return _hip.TD_SRC_RGB24, [3 * sw], [3 * sw * sh]
    if pix_fmt == "yuv420p":
        return _hip.TD_SRC_I420, [sw, cw, cw], [sw * sh, cw * ch, cw * ch]
    if pix_fmt == "nv12":
        return _hip.TD_SRC_NV12, [sw, 2 * cw], [sw * sh, 2 * cw * ch]
    raise ValueError(f"pix_fmt {pix_fmt!r}: one of {_PIX_FMTS}")


def _describe(base, sizes, tight, planes, pitches, frame_stride):
    pitches = list(tight if pitches is None else pitches)
    if planes is None:
        planes = [base + sum(sizes[:i]) for i in range(len(sizes))]
        if frame_stride is None:
            frame_stride = sum(sizes)
    if len(planes) != len(sizes) or len(pitches) != len(sizes) or frame_stride is None:
        raise ValueError("one address and one pitch per plane, and the frame stride")
    return list(planes) + [None] * (3 - len(sizes)), pitches + [0] * (3 - len(sizes)), int(frame_stride)


def _put_planes(j, stem: str, described):
    """Write what ``_describe`` returned into job ``j`` under the field stem "src", "dst", or "" (plane0 / pitch0 / frame_stride)."""
    planes, pitches, stride = described  # (plain attribute stores, spelled out per stem: this runs once or twice per job of every launch)
    if stem == "src":
        (j.src0, j.src1, j.src2), (j.src_pitch0, j.src_pitch1, j.src_pitch2), j.src_frame_stride = planes, pitches, stride
    elif stem == "dst":
        (j.dst0, j.dst1, j.dst2), (j.dst_pitch0, j.dst_pitch1, j.dst_pitch2), j.dst_frame_stride = planes, pitches, stride
    else:
        (j.plane0, j.plane1, j.plane2), (j.pitch0, j.pitch1, j.pitch2), j.frame_stride = planes, pitches, stride
    return described


def _put_src_dst(j, src, dst, sizes, tight, src_planes, src_pitches, src_frame_stride, dst_planes, dst_pitches, dst_frame_stride):
    """The src* and dst* fields of an overlay or redact job; neither ``dst`` nor ``dst_planes``: in place."""
    s = _put_planes(j, "src", _describe(src, sizes, tight, src_planes, src_pitches, src_frame_stride))
    _put_planes(j, "dst", s if dst is None and dst_planes is None else _describe(dst, sizes, tight, dst_planes, dst_pitches, dst_frame_stride))


# ---- the pool of job tables ----------------------------------------------------------------------------------------------------
# (pinned, device, event recorded behind the launch).  A table is taken again only once its event has completed (a query, never a
# wait); otherwise a new one is made, so the pool grows to the number of launches in flight.
_tables: List[tuple] = []


def take_table(nb: int, device) -> tuple:
    """A (pinned, device, event) triple of at least ``nb`` bytes on ``device``, out of the pool or new; ``release_table`` gives it back."""
    for i, (host, dev, ev) in enumerate(_tables):
        if host.numel() >= nb and dev.device == device and ev.query():
            return _tables.pop(i)
    n = max(nb, 4096)
    return torch.empty(n, dtype=torch.uint8, pin_memory=True), torch.empty(n, dtype=torch.uint8, device=device), torch.cuda.Event()


def release_table(triple: tuple):
    """Record the triple's event on the current stream - behind the last launch that reads its device side - and pool it."""
    triple[2].record()
    _tables.append(triple)


def tables_pooled() -> int:
    """How many tables lie in the pool; for tests/test_render_refusals_gpu.py, which checks that the pool does not grow."""
    return len(_tables)


# ---- launching -----------------------------------------------------------------------------------------------------------------
_JOB_TYPES = {entry: _hip._SIGS[entry][0]._type_.__name__ for entry in (
    "td_tube_overlay", "td_tube_overlay_multi", "td_tube_crop", "td_tube_redact", "td_tube_densify", "td_frame_stats", "td_shot_cuts", "td_tube_follow",
    "td_frame_export")}  # entry point -> its record in _hip


def _enqueue(entry: str, jobs: Sequence, host: torch.Tensor, dev: torch.Tensor, nbytes: int, *second):
    """Call ``entry`` on the current stream; ``second``: the record array that td_tube_densify_shots takes behind the jobs (or None)."""
    arr = (_hip._SIGS[entry][0]._type_ * len(jobs))(*jobs)
    _hip.check(getattr(_hip.lib(), entry)(arr, *second, len(jobs), host.data_ptr(), dev.data_ptr(), nbytes, _hip.stream_ptr()), entry)


def _launch_fresh(entry: str, jobs: Sequence, device, *second) -> tuple:
    """One launch on the current stream with freshly allocated job tables; returns them."""
    nb = int(getattr(_hip.lib(), entry + "_table_bytes")(len(jobs)))
    host = torch.empty(max(nb, 256), dtype=torch.uint8, pin_memory=True)
    dev = torch.empty(max(nb, 256), dtype=torch.uint8, device=device)
    _enqueue(entry, jobs, host, dev, nb, *second)
    return host, dev


def _launch_pooled(entry: str, jobs: Sequence, keep: Sequence, results: list, single: bool, device, uploads: Sequence = (), second: tuple = ()):
    """One launch on the current stream with a pooled job table; ``keep`` holds, per clip, the tensors that the launch reads;
    returns ``results`` (its only entry for a single clip).  Without jobs nothing is launched.
    ``uploads``: (job, field, host tensor) - small host inputs of the jobs travel in the table's memory behind the table, 16
    bytes apart at least, and are guarded by its event; the job's field gets the device address.  ``second``: as for ``_enqueue``."""
    if not jobs:
        return results[0] if single else results
    nb = int(getattr(_hip.lib(), entry + "_table_bytes")(len(jobs)))
    sizes = [(t.numel() * t.element_size() + 15) // 16 * 16 for _, _, t in uploads]
    triple = host, dev, _ = take_table(nb + sum(sizes), device)
    if uploads:
        off = nb
        for (j, field, t), size in zip(uploads, sizes):
            host[off:off + t.numel() * t.element_size()].copy_(t.view(-1).view(torch.uint8))
            setattr(j, field, dev.data_ptr() + off)
            off += size
        dev[nb:off].copy_(host[nb:off], non_blocking=True)
    _enqueue(entry, jobs, host, dev, host.numel(), *second)
    release_table(triple)
    stream = torch.cuda.current_stream(device)
    for group in keep:  # contiguous() may have made copies: the allocator must not hand them out before the launch has run
        for t in group:
            if t is not None:
                t.record_stream(stream)
    return results[0] if single else results


def _fresh_launcher(name: str, entry: str, wrapper: str = None, doc: str = None):
    """``name(jobs, device)``: ``_launch_fresh`` bound to ``entry``; ``wrapper`` names the function that pools its tables instead."""
    def launch(jobs: Sequence, device) -> tuple:
        return _launch_fresh(entry, jobs, device)

    launch.__name__ = launch.__qualname__ = name
    launch.__doc__ = doc or (f"One {entry} launch on the current stream with freshly allocated job tables; returns them: the caller keeps\n"
                             f"    them alive until the stream has passed the launch (``{wrapper}`` recycles its own instead).")
    return launch


tube_overlay = _fresh_launcher("tube_overlay", "td_tube_overlay", "annotate")
tube_overlay_multi = _fresh_launcher("tube_overlay_multi", "td_tube_overlay_multi", "annotate_tubes")
tube_crop = _fresh_launcher("tube_crop", "td_tube_crop", "crop_tubes")
tube_redact = _fresh_launcher("tube_redact", "td_tube_redact", "redact")
tube_densify = _fresh_launcher("tube_densify", "td_tube_densify", "densify")
launch_frame_stats = _fresh_launcher("launch_frame_stats", "td_frame_stats", "frame_stats")
launch_shot_cuts = _fresh_launcher("launch_shot_cuts", "td_shot_cuts", doc="One td_shot_cuts launch, as ``launch_frame_stats``.")
tube_follow = _fresh_launcher("tube_follow", "td_tube_follow", "follow")
frame_export = _fresh_launcher("frame_export", "td_frame_export", "export")
clip_resample = _fresh_launcher("clip_resample", "td_clip_resample", "ClipPipeline.stage_raw")
clip_resample_src = _fresh_launcher("clip_resample_src", "td_clip_resample_src", doc="``clip_resample`` for ``resample_src_job`` jobs (td_clip_resample_src).")


def tube_densify_shots(jobs: Sequence, shots, device) -> tuple:
    """One td_tube_densify_shots launch, as ``tube_densify``; ``shots`` holds one ``_hip.DenseShots`` per job, or is None."""
    return _launch_fresh("td_tube_densify_shots", jobs, device, (_hip.DenseShots * len(jobs))(*shots) if shots is not None else None)
