"""td_tube_redact without a GPU: properties of the numpy reference that pin the rule's intent (tests/redact_ref.py), the
library's own refusals (nothing is launched: no device is needed), and the ctypes mirror against the header."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from redact_ref import luma_selection, redact_ref, snapped_rect
from test_overlay_gpu import as_rows, make_planes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FMTS = ["rgb24", "yuv420p", "nv12"]
SH, SW = 37, 53
BOXES = np.array([[[10.3, 5.5, 31.2, 22.7], [25.5, 15.0, 47.5, 30.1]],
                  [[-3.0, -2.0, 12.0, 9.0], [40.0, 30.0, 60.0, 45.0]],
                  [[1.0, 1.0, 2.0, 2.0], [20.2, 0.0, 33.3, 37.0]]], dtype=np.float32)  # (3, 2, 4)


def planes_of(fmt, T=3, seed=0, sh=SH, sw=SW):
    return make_planes(np.random.default_rng(seed), T, sh, sw, fmt)


def same(a, b, fmt):
    return all(np.array_equal(x, y) for x, y in zip(as_rows(a, fmt), as_rows(b, fmt)))


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("cell", [2, 6, 16, 256])
def test_mosaic_is_idempotent(fmt, cell):
    kw = dict(boxes=BOXES, mode="mosaic", cell=cell)
    once = redact_ref(planes_of(fmt), fmt, **kw)
    assert same(redact_ref(once, fmt, **kw), once, fmt)
    assert not same(once, planes_of(fmt), fmt)


@pytest.mark.parametrize("fmt", FMTS)
def test_blur_and_mosaic_of_a_constant_frame_return_it(fmt):
    flat = planes_of(fmt)
    flat = np.full_like(flat, 77) if fmt == "rgb24" else tuple(np.full_like(p, 60 + 30 * i) for i, p in enumerate(flat))
    for kw in (dict(mode="mosaic", cell=6), dict(mode="mosaic", cell=256), dict(mode="blur", radius=1), dict(mode="blur", radius=3), dict(mode="blur", radius=64)):
        for invert in (False, True):
            assert same(redact_ref(flat, fmt, boxes=BOXES, invert=invert, **kw), flat, fmt), (kw, invert)


def test_fill_changes_the_same_luma_set_in_every_format_and_whole_chroma_blocks():
    T = 3
    for margin in ((0, 1), (1, 4)):
        sel = luma_selection(T, SH, SW, BOXES, mode="fill", margin=margin)
        assert sel.any() and not sel.all()
        changed = {}
        for fmt in FMTS:
            src = planes_of(fmt, T)
            luma = src if fmt == "rgb24" else src[0]
            # no single colour differs from every source byte: fill twice, a byte is changed when either fill changed it
            a = redact_ref(src, fmt, boxes=BOXES, mode="fill", color=(0, 0, 0), margin=margin)
            b = redact_ref(src, fmt, boxes=BOXES, mode="fill", color=(255, 255, 255), margin=margin)
            la, lb = (a, b) if fmt == "rgb24" else (a[0], b[0])
            ch = (la != luma) | (lb != luma)
            changed[fmt] = ch.any(-1) if fmt == "rgb24" else ch
            if fmt != "rgb24":
                ca, cb, cs = as_rows(a, fmt)[1], as_rows(b, fmt)[1], as_rows(src, fmt)[1]
                cch = (ca != cs) | (cb != cs)
                cch = cch.reshape(T, (SH + 1) // 2, (SW + 1) // 2, -1).any(-1)
                for t, i, j in zip(*np.nonzero(cch)):  # a selected chroma sample: every luma pixel of its block that exists is selected
                    assert sel[t, 2 * i : 2 * i + 2, 2 * j : 2 * j + 2].all()
                assert np.array_equal(cch, sel[:, 0::2, 0::2])
        assert np.array_equal(changed["rgb24"], sel) and np.array_equal(changed["yuv420p"], sel) and np.array_equal(changed["nv12"], sel)


@pytest.mark.parametrize("fmt", FMTS)
def test_invert_changes_exactly_the_complement(fmt):
    src = planes_of(fmt)
    for kw in (dict(mode="fill"), dict(mode="mosaic", cell=6)):
        sel = luma_selection(3, SH, SW, BOXES, **kw)
        inv = luma_selection(3, SH, SW, BOXES, invert=True, **kw)
        assert np.array_equal(inv, ~sel)
    a0, a1 = (redact_ref(src, fmt, boxes=BOXES, mode="fill", color=c) for c in ((0, 0, 0), (255, 255, 255)))
    b0, b1 = (redact_ref(src, fmt, boxes=BOXES, mode="fill", color=c, invert=True) for c in ((0, 0, 0), (255, 255, 255)))
    for s, x0, x1, y0, y1 in zip(as_rows(src, fmt), as_rows(a0, fmt), as_rows(a1, fmt), as_rows(b0, fmt), as_rows(b1, fmt)):
        plain, inverted = (x0 != s) | (x1 != s), (y0 != s) | (y1 != s)
        assert np.array_equal(inverted, ~plain) and plain.any() and inverted.any()


@pytest.mark.parametrize("fmt", FMTS)
def test_k_rectangles_equal_k_single_rectangle_fills_in_sequence(fmt):
    src = planes_of(fmt)
    span = np.array([[0, 1], [1, 2]])
    together = redact_ref(src, fmt, boxes=BOXES, span=span, mode="fill", color=(9, 99, 199), margin=(1, 4))
    step = src
    for k in range(2):
        step = redact_ref(step, fmt, boxes=BOXES[:, k], span=span[k], mode="fill", color=(9, 99, 199), margin=(1, 4))
    assert same(together, step, fmt) and not same(together, src, fmt)


@pytest.mark.parametrize("fmt", FMTS)
def test_a_frame_whose_tube_row_is_out_of_range_is_a_copy_or_fully_redacted(fmt):
    src = planes_of(fmt, T=4)
    fmap = [0, -1, 3, 1]
    color = (11, 22, 33)
    plain = redact_ref(src, fmt, boxes=BOXES, frame_map=fmap, mode="fill", color=color)
    inv = redact_ref(src, fmt, boxes=BOXES, frame_map=fmap, mode="fill", color=color, invert=True)
    for t in (1, 2):
        for k, (s, p, i) in enumerate(zip(as_rows(src, fmt), as_rows(plain, fmt), as_rows(inv, fmt))):
            assert np.array_equal(p[t], s[t])
            want = np.array(color, dtype=np.uint8) if fmt == "rgb24" else np.array(color[1:]) if (fmt == "nv12" and k == 1) else np.array([color[k]])
            assert (i[t].reshape(i.shape[1], -1, len(want)) == want).all()
    assert not np.array_equal(as_rows(plain, fmt)[0][0], as_rows(src, fmt)[0][0])
    outside = redact_ref(src, fmt, boxes=BOXES, span=[[5, 9], [7, 7]], mode="fill", color=color, invert=True)  # outside every span: nothing is left in the clear
    assert same(outside, redact_ref(src, fmt, boxes=BOXES, frame_map=[-1] * 4, mode="fill", color=color, invert=True), fmt)


def test_nan_infinite_and_degenerate_boxes_are_absent():
    for box in ([np.nan, 1, 9, 9], [1, 1, np.inf, 9], [-np.inf, 1, 9, 9], [5, 1, 5.4, 9], [1, 6, 9, 5], [60, 1, 70, 9], [-9, -9, -4, -4], [2.0, 1.0, 2.3, 9.0]):
        for mode in ("fill", "mosaic", "blur"):
            assert snapped_rect(box, SH, SW, mode, 6, (1, 4)) is None, box
    assert snapped_rect([-9, -9, -1, -1], SH, SW, "fill", 6, (1, 4)) == (0, 2, 0, 2)  # the margin of 2 brings one pixel into the frame: its block
    assert snapped_rect([-1e30, -1e30, 1e30, 1e30], SH, SW, "fill", 6, (4, 1)) == (0, SW, 0, SH)  # finite: clamped, then the frame
    assert snapped_rect([10.5, 3.5, 11.5, 4.5], SH, SW, "fill", 6, (0, 1)) == (10, 12, 4, 6)  # x.5 rounds up; one pixel snaps to its 2 x 2 block
    assert snapped_rect([10.5, 3.5, 11.5, 4.5], SH, SW, "mosaic", 6, (0, 1)) == (6, 12, 0, 6)
    assert snapped_rect([50.0, 30.0, 53.0, 37.0], SH, SW, "mosaic", 16, (0, 1)) == (48, SW, 16, SH)  # the far cells are cut off at the frame
    src = planes_of("yuv420p")
    boxes = np.array([[np.nan, 1, 9, 9]] * 3, dtype=np.float32)
    assert same(redact_ref(src, "yuv420p", boxes=boxes, mode="blur", radius=3), src, "yuv420p")


# ---- the library's refusals: no launch happens ---------------------------------------------------------------------------
def _call(job, nbytes=4096):
    from tubedetr_amd import _hip

    L = _hip.lib()
    table = ctypes.create_string_buffer(4096)
    arr = (_hip.RedactJob * 1)(job)
    rc = L.td_tube_redact(arr, 1, ctypes.addressof(table), ctypes.c_void_p(4096), nbytes, None)
    return rc, L.td_last_error()


def _job(**kw):
    from tubedetr_amd.render import redact_job

    args = dict(src=1 << 20, T=2, sh=6, sw=8, boxes=1 << 26, n_tube=2, dst=1 << 24)
    args.update(kw)
    return redact_job(**args)


@pytest.mark.parametrize("field,value,mode,name", [
    ("cell", 7, "mosaic", b"cell"), ("cell", 0, "mosaic", b"cell"), ("cell", 258, "mosaic", b"cell"),
    ("radius", 0, "blur", b"radius"), ("radius", 65, "blur", b"radius"),
    ("K", 0, "fill", b"K = "), ("K", 9, "fill", b"K = "),
    ("margin_den", 0, "fill", b"margin_den"), ("margin_num", 5, "fill", b"margin_num"),
    ("boxes", None, "fill", b"boxes"), ("sh", 0, "fill", b"sh"), ("sw", 16385, "fill", b"sw"),
    ("n_tube", 0, "fill", b"n_tube"), ("mode", 3, "fill", b"mode"), ("invert", 2, "fill", b"invert"), ("fmt", 7, "fill", b"fmt"),
])
def test_library_refuses_a_violated_limit_and_names_the_field(field, value, mode, name):
    job = _job(mode=mode)
    setattr(job, field, value)
    rc, msg = _call(job)
    assert rc != 0 and name in msg, msg


def test_library_refuses_blur_in_place_and_partial_overlap_and_ignores_the_unused_parameters():
    from tubedetr_amd import _hip

    L = _hip.lib()
    rc, msg = _call(_job(mode="blur", dst=None))
    assert rc != 0 and b"dst0" in msg and b"in place" in msg
    rc, msg = _call(_job(mode="blur", dst=None, T=0))  # refused whatever the frame count
    assert rc != 0 and b"dst0" in msg
    rc, msg = _call(_job(mode="fill", dst=(1 << 20) + 1))  # shifted by one byte: neither in place nor apart
    assert rc != 0 and b"overlaps" in msg and b"dst0" in msg
    rc, msg = _call(_job(mode="mosaic", dst=(1 << 20) + 6 * 8 * 3))  # frame t written over frame t + 1
    assert rc != 0 and b"overlaps" in msg
    rc, msg = _call(_job(mode="fill", pix_fmt="yuv420p", dst_planes=[1 << 24, (1 << 20) + 50, 1 << 25], dst_pitches=[8, 4, 4], dst_frame_stride=1 << 12))  # dst1 inside src
    assert rc != 0 and b"overlaps" in msg and b"dst1" in msg
    # T = 0: everything is checked, nothing is launched, and the call succeeds; so does a job whose unused parameters are out of range
    for kw in (dict(mode="fill"), dict(mode="mosaic", dst=None), dict(mode="blur")):
        job = _job(T=0, **kw)
        if kw["mode"] != "mosaic":
            job.cell = 7
        if kw["mode"] != "blur":
            job.radius = 0
        rc, msg = _call(job)
        assert rc == 0, msg
    rc, msg = _call(_job(), nbytes=L.td_tube_redact_table_bytes(1) - 1)
    assert rc != 0 and b"table" in msg
    assert L.td_tube_redact(None, 0, None, None, 0, None) != 0 and b"no jobs" in L.td_last_error()
    assert L.td_tube_redact_table_bytes(0) == 0 and L.td_tube_redact_table_bytes(3) % 256 == 0 and L.td_tube_redact_table_bytes(3) > 0
    assert L.td_tube_redact_table_bytes(16) <= 4096  # a batch of clips fits the smallest pooled table


def test_redact_job_mirror_matches_the_header_and_the_abi_is_still_11():
    from tubedetr_amd import _hip

    src = open(os.path.join(ROOT, "include", "tubedetr_hip.h")).read()
    flat = " ".join(re.sub(r"/\*.*?\*/", "", src, flags=re.S).split())
    body = re.search(r"typedef struct td_redact_job \{(.*?)\} td_redact_job;", flat).group(1)
    names = [re.sub(r"\[\d+\]", "", part).split()[-1].lstrip("*") for decl in body.split(";") if decl.strip() for part in decl.split(",")]
    assert names == [n for n, _ in _hip.RedactJob._fields_], "td_redact_job and its ctypes mirror list different fields"
    assert _hip.EXPECTED_ABI == 11 and _hip.lib().td_abi_version() == 11
    assert "td_tube_redact" in _hip.EXPORTS and "td_tube_redact_table_bytes" in _hip.EXPORTS
    assert re.search(r"int td_tube_redact\(const td_redact_job\* jobs, int n_jobs, void\* table_host, void\* table_dev, size_t table_bytes, td_stream_t stream\);", flat)
    assert flat.index("td_tube_crop(") < flat.index("typedef struct td_redact_job")  # an addition: nothing above it changed
    for name, code in (("FILL", _hip.TD_REDACT_FILL), ("MOSAIC", _hip.TD_REDACT_MOSAIC), ("BLUR", _hip.TD_REDACT_BLUR)):
        assert re.search(rf"#define TD_REDACT_{name} {code}\b", src)
    assert "redact.hip" in __import__("tubedetr_amd.build", fromlist=["SOURCES"]).SOURCES


def test_python_layer_refuses_bad_arguments_before_the_device_is_touched():
    from tubedetr_amd.render import DeviceFrames, redact, redact_job

    ok = redact_job(4096, 2, 5, 7, boxes=1 << 20, n_tube=2, pix_fmt="yuv420p")
    assert (ok.dst0, ok.dst1, ok.dst2) == (ok.src0, ok.src1, ok.src2) == (4096, 4096 + 35, 4096 + 35 + 12) and ok.src_frame_stride == ok.dst_frame_stride == 59
    assert (ok.mode, ok.cell, ok.K, ok.invert, ok.margin_num, ok.margin_den) == (1, 16, 1, 0, 0, 1)
    for kw in ({"mode": "pixelate"}, {"mode": "mosaic", "cell": 7}, {"mode": "mosaic", "cell": 0}, {"mode": "mosaic", "cell": 258}, {"mode": "blur", "radius": 0},
               {"mode": "blur", "radius": 65}, {"K": 0}, {"K": 9}, {"margin": (1, 0)}, {"margin": (5, 1)}, {"boxes": None}, {"n_tube": 0}, {"color": (0, 0, 256)},
               {"sh": 0}, {"pix_fmt": "yuv444p"}, {"invert": 2}):
        with pytest.raises(ValueError):
            redact_job(**{"src": 4096, "T": 1, "sh": 4, "sw": 4, "boxes": 1 << 20, "n_tube": 1, **kw})
    # a clip that lives on no device: DeviceFrames refuses it, so the object is made without its checks - redact must raise
    # for blur in place from its arguments alone, before it allocates, looks for the library's device or enqueues anything
    frames = object.__new__(DeviceFrames)
    frames.data, frames.T, frames.h, frames.w, frames.pix_fmt, frames.matrix, frames.full_range = torch.zeros(2 * 3 * 4 * 6, dtype=torch.uint8), 2, 4, 6, "rgb24", "bt601", False
    boxes = torch.tensor([[0.0, 0.0, 3.0, 3.0]] * 2)
    with pytest.raises(ValueError, match="in place"):
        redact(frames, boxes, mode="blur", out=frames)
    with pytest.raises(ValueError, match="in place"):
        redact([frames], [boxes], mode="blur", radius=64, out=[frames])
    assert not frames.data.any()
    with pytest.raises(ValueError):
        redact(frames, boxes.view(2, 1, 4), span=torch.zeros(2, 2, dtype=torch.int64))  # K = 1 with two spans
    with pytest.raises(ValueError):
        redact(frames, torch.zeros(2, 9, 4))  # K = 9
