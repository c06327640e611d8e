"""The refusals that td_tube_overlay, td_tube_crop and td_tube_redact have in common (csrc/frame_jobs.h: plane geometry, plane
checks, in place or apart, workspace, margin), pinned to the letter: the texts are part of the interface - callers log them and
the Python layer forwards them.  One violating job per check; nothing is launched on these paths, so the addresses are made up
and no device is needed."""
import ctypes

import pytest

SRC, DST, BOXES = 1 << 20, 1 << 24, 1 << 26
T, SH, SW = 2, 6, 8  # yuv420p: Y 6 rows of 8 bytes, U and V 3 rows of 4; 72 bytes per frame.  rgb24: 6 rows of 24; 144 per frame


def _job(entry, fmt="yuv420p", **kw):
    from tubedetr_amd import render

    if entry == "overlay":
        args = dict(src=SRC, T=T, sh=SH, sw=SW, dst=DST, pix_fmt=fmt, boxes=BOXES, n_tube=2)
    elif entry == "crop":
        args = dict(src=SRC, T=T, sh=SH, sw=SW, boxes=BOXES, n_tube=2, dst=DST, size=(4, 4), pix_fmt=fmt)
    else:
        args = dict(src=SRC, T=T, sh=SH, sw=SW, boxes=BOXES, n_tube=2, dst=DST, pix_fmt=fmt, mode="fill")
    args.update(kw)
    return getattr(render, entry + "_job")(**args)


def _with(job, **fields):
    for k, v in fields.items():
        setattr(job, k, v)
    return job


def _call(entry, jobs, n_jobs=None, host=True, dev=4096, nbytes=4096):
    from tubedetr_amd import _hip

    L = _hip.lib()
    table = ctypes.create_string_buffer(4096)
    kind = {"overlay": _hip.OverlayJob, "crop": _hip.CropJob, "redact": _hip.RedactJob}[entry]
    arr = (kind * max(len(jobs), 1))(*jobs)
    rc = getattr(L, "td_tube_" + entry)(arr, len(jobs) if n_jobs is None else n_jobs, ctypes.addressof(table) if host else None, ctypes.c_void_p(dev) if dev else None,
                                        nbytes, None)
    return rc, L.td_last_error().decode()


def _violation(entry, key):
    """(jobs, keyword arguments of _call) of violation ``key`` for one entry point."""
    src_dst = entry != "crop"
    name = lambda stem, what: f"{stem}_{what}" if src_dst else what  # noqa: E731
    fields = {
        "fmt": dict(fmt=7), "T<0": dict(T=-1), "sh=0": dict(sh=0), "sh>max": dict(sh=16385), "sw=0": dict(sw=0), "sw>max": dict(sw=16385 if src_dst else 8193),
        "margin_den=0": dict(margin_den=0), "margin_den>max": dict(margin_den=1025), "margin_num<0": dict(margin_num=-1), "margin_num>4den": dict(margin_den=3, margin_num=13),
    }
    for stem in ("src", "dst") if src_dst else ("src",):
        for k, row in enumerate((8, 4, 4)):
            fields[f"{stem}{k} null"] = {f"{stem}{k}" if src_dst else f"plane{k}": None}
            fields[f"{stem} pitch{k}"] = {name(stem, f"pitch{k}"): row - 1}
        fields[f"{stem} stride, plane 0"] = {name(stem, "frame_stride"): 47}
        fields[f"{stem} stride, plane 2"] = {name(stem, "pitch2"): 100}
    if key in fields:
        return [_with(_job(entry), **fields[key])], {}
    if key == "job 1 after a job without frames":
        return [_job(entry, T=0), _with(_job(entry), fmt=7)], {}
    if key == "dst shifted by one byte":
        return [_job(entry, "rgb24", dst=SRC + 1)], {}
    if key == "dst frame over the next src frame":
        return [_job(entry, "rgb24", dst=SRC + 144)], {}
    if key == "dst1 inside src0":
        return [_job(entry, dst_planes=[DST, SRC + 50, 1 << 25], dst_pitches=[8, 4, 4], dst_frame_stride=1 << 12)], {}
    if key == "blur in place":
        return [_job(entry, mode="blur", dst=None)], {}
    if key == "blur in place, no frames":
        return [_job(entry, mode="blur", dst=None, T=0)], {}
    from tubedetr_amd import _hip

    call = {"no host table": dict(host=False), "no device table": dict(dev=0), "n_jobs=0": dict(n_jobs=0), "more than 65536 jobs": dict(n_jobs=65537),
            "table one byte short": dict(nbytes=int(getattr(_hip.lib(), f"td_tube_{entry}_table_bytes")(1)) - 1)}[key]
    return [_job(entry)], call


_PLANES = {
    "{s}0 null": "{who}: job 0: {p}0 is null", "{s}1 null": "{who}: job 0: {p}1 is null", "{s}2 null": "{who}: job 0: {p}2 is null",
    "{s} pitch0": "{who}: job 0: {f}pitch0 = 7 is below its row of 8 bytes", "{s} pitch1": "{who}: job 0: {f}pitch1 = 3 is below its row of 4 bytes",
    "{s} pitch2": "{who}: job 0: {f}pitch2 = 3 is below its row of 4 bytes",
    "{s} stride, plane 0": "{who}: job 0: {f}frame_stride 47 is smaller than plane 0 needs (6 rows of pitch 8)",
    "{s} stride, plane 2": "{who}: job 0: {f}frame_stride 72 is smaller than plane 2 needs (3 rows of pitch 100)",
}
_COMMON = {
    "fmt": "{who}: job 0: unknown fmt 7", "T<0": "{who}: job 0: negative frame count T = -1",
    "job 1 after a job without frames": "{who}: job 1: unknown fmt 7",
    "no host table": "{who}: job-table workspace missing or smaller than {who}_table_bytes(1)",
    "no device table": "{who}: job-table workspace missing or smaller than {who}_table_bytes(1)",
    "table one byte short": "{who}: job-table workspace missing or smaller than {who}_table_bytes(1)",
    "n_jobs=0": "{who}: no jobs (or more than 65536)", "more than 65536 jobs": "{who}: no jobs (or more than 65536)",
}
_SIDES = {"sh=0": "{who}: job 0: sh x sw = 0 x 8 outside 1..16384", "sh>max": "{who}: job 0: sh x sw = 16385 x 8 outside 1..16384",
          "sw=0": "{who}: job 0: sh x sw = 6 x 0 outside 1..16384", "sw>max": "{who}: job 0: sh x sw = 6 x 16385 outside 1..16384"}
_APART = {"dst shifted by one byte": "{who}: job 0: dst0 overlaps src0 without being the same plane (pointer, pitch and frame stride)",
          "dst frame over the next src frame": "{who}: job 0: dst0 overlaps src0 without being the same plane (pointer, pitch and frame stride)",
          "dst1 inside src0": "{who}: job 0: dst1 overlaps src0 without being the same plane (pointer, pitch and frame stride)"}
_MARGIN = {"margin_den=0": "{who}: job 0: margin_den = 0 outside 1..1024", "margin_den>max": "{who}: job 0: margin_den = 1025 outside 1..1024",
           "margin_num<0": "{who}: job 0: margin_num = -1 outside 0..4 margin_den = 4", "margin_num>4den": "{who}: job 0: margin_num = 13 outside 0..4 margin_den = 12"}


def _texts(who, *tables, **names):
    return {k.format(**names): v.format(who=who, **names) for t in tables for k, v in t.items()}


def _planes(who, s, p, f):
    return _texts(who, _PLANES, s=s, p=p, f=f)


# recorded from the library before the shared header existed: every text below is what the three entry points said then
TEXTS = {
    "overlay": {**_texts("td_tube_overlay", _COMMON, _SIDES, _APART), **_planes("td_tube_overlay", "src", "src", "src_"), **_planes("td_tube_overlay", "dst", "dst", "dst_")},
    "crop": {**_texts("td_tube_crop", _COMMON, _MARGIN), **_planes("td_tube_crop", "src", "plane", ""),
             "sh=0": "td_tube_crop: job 0: sh = 0 outside 1..16384", "sh>max": "td_tube_crop: job 0: sh = 16385 outside 1..16384",
             "sw=0": "td_tube_crop: job 0: sw = 0 outside 1..8192 (a window can be the whole row)",
             "sw>max": "td_tube_crop: job 0: sw = 8193 outside 1..8192 (a window can be the whole row)"},
    "redact": {**_texts("td_tube_redact", _COMMON, _SIDES, _APART, _MARGIN), **_planes("td_tube_redact", "src", "src", "src_"), **_planes("td_tube_redact", "dst", "dst", "dst_"),
               "blur in place": "td_tube_redact: job 0: dst0 is its source plane: TD_REDACT_BLUR cannot run in place (it reads neighbours that are already rewritten)",
               "blur in place, no frames": "td_tube_redact: job 0: dst0 is its source plane: TD_REDACT_BLUR cannot run in place (it reads neighbours that are already rewritten)"},
}


@pytest.mark.parametrize("entry,key", [(e, k) for e, t in TEXTS.items() for k in t])
def test_refusal_text_is_what_it_was(entry, key):
    jobs, kw = _violation(entry, key)
    rc, msg = _call(entry, jobs, **kw)
    assert rc != 0 and msg == TEXTS[entry][key]


@pytest.mark.parametrize("entry", list(TEXTS))
def test_jobs_without_frames_pass_every_check_and_launch_nothing(entry):
    """A job with T = 0 is checked like any other and then skipped; a table of such jobs returns TD_OK with a null stream and
    without a device.  (A job WITH frames behind or in front of one would be launched: that order is the GPU suites'; here the
    job behind a T = 0 one is a refused one, "job 1 after a job without frames" above.)"""
    for fmt in ("rgb24", "yuv420p", "nv12"):
        for n in (1, 2, 3):
            rc, msg = _call(entry, [_job(entry, fmt, T=0) for _ in range(n)])
            assert rc == 0, msg
    if entry != "crop":
        rc, msg = _call(entry, [_job(entry, T=0, dst=None), _job(entry, "rgb24", T=0, dst=SRC + 1)])  # in place; shifted, but no bytes to overlap
        assert rc == 0, msg
