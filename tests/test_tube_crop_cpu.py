"""Tube crops without a GPU: the numpy restatement of the rule (tests/tube_crop_ref.py) against windows worked out by hand from
include/tubedetr_hip.h, the ABI, argument checking in the library and in Python, and the condition the GPU float64 test puts
on its own inputs (checked here because it depends on the reference alone)."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from test_augment_cpu import resample_f64
from tube_crop_ref import EMPTY, box_window, compose, out_size, round_coord, tube_windows

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# the float64 check of tests/test_tube_crop_gpu.py: (frame h x w, box xyxy, output size, expected window, seed)
F64_CASES = {
    "up": ((21, 30), (7.0, 5.0, 20.0, 14.0), (64, 64), (5, 7, 9, 13, 64, 64), 0),
    "down": ((70, 100), (4.0, 6.0, 94.0, 66.0), (7, 11), (6, 4, 60, 90, 7, 11), 0),
}


def f64_frames(name):
    (sh, sw), _, _, _, seed = F64_CASES[name]
    return np.random.default_rng(seed).integers(0, 256, (2, sh, sw, 3), dtype=np.uint8)


def test_rule_by_hand_37x51():
    # floorf(v + 0.5): 10.4 -> 10, 5.5 -> 6, 30.6 -> 31, 20.49 -> 20: columns [10, 31), rows [6, 20); 21 / 4 = 5, 14 / 4 = 3:
    # columns [5, 36), rows [3, 23), inside the frame; 31 * 16 >= 20 * 16: rw = 16, rh = (2 * 20 * 16 + 31) / 62 = 671 / 62 = 10
    assert [round_coord(v) for v in (10.4, 5.5, 30.6, 20.49)] == [10, 6, 31, 20]
    assert box_window((10.4, 5.5, 30.6, 20.49), 37, 51, 16, 16, (1, 4), True) == (3, 5, 20, 31, 10, 16)
    assert box_window((10.4, 5.5, 30.6, 20.49), 37, 51, 16, 16, (1, 4), False) == (3, 5, 20, 31, 16, 16)
    assert box_window((10.4, 5.5, 30.6, 20.49), 37, 51, 16, 16, (0, 1), True) == (6, 10, 14, 21, 11, 16)  # (2 * 14 * 16 + 21) / 42 = 469 / 42 = 11


def test_rule_edges_empties_and_margins():
    sh, sw = 37, 51
    w = lambda box, margin=(0, 1), keep=False: box_window(box, sh, sw, 8, 8, margin, keep)  # noqa: E731
    assert w((-5, 10, 7, 20)) == (10, 0, 10, 7, 8, 8)      # across the left edge
    assert w((45, 10, 60, 20)) == (10, 45, 10, 6, 8, 8)    # right
    assert w((10, -4, 20, 6)) == (0, 10, 6, 10, 8, 8)      # top
    assert w((10, 30, 20, 44)) == (30, 10, 7, 10, 8, 8)    # bottom
    for box in ((60, 5, 70, 9), (-20, 5, -3, 9), (5, 40, 9, 50), (5, -9, 9, -1)):  # wholly outside
        assert w(box) == EMPTY
    assert w((51, 5, 60, 9)) == EMPTY and w((-9, 5, 0, 9)) == EMPTY  # touching the edge from outside
    assert w((7, 9, 8, 10)) == (9, 7, 1, 1, 8, 8) and w((7, 9, 8, 10), keep=True) == (9, 7, 1, 1, 8, 8)  # 1 x 1
    assert w((0, 0, 51, 37)) == (0, 0, 37, 51, 8, 8) and w((-0.4, -0.4, 51.4, 37.4)) == (0, 0, 37, 51, 8, 8)  # the whole frame
    assert w((0, 0, 51, 37), keep=True) == (0, 0, 37, 51, 6, 8)  # (2 * 37 * 8 + 51) / 102 = 643 / 102 = 6
    for bad in (np.nan, np.inf, -np.inf):
        for k in range(4):
            box = [10.0, 10.0, 20.0, 20.0]
            box[k] = bad
            assert w(box) == EMPTY
    assert w((10, 5, 10, 9)) == EMPTY and w((10.4, 5, 9.6, 9)) == EMPTY and w((3, 9, 8, 9)) == EMPTY and w((3, 9, 8, 8)) == EMPTY  # x1 == x0, y1 <= y0
    assert w((20, 15, 30, 22), (4, 1)) == (0, 0, 37, 51, 8, 8)  # 40 and 28 of margin: clamped to the whole frame
    assert w((20, 15, 30, 22), (1, 1)) == (8, 10, 21, 30, 8, 8)
    assert w((1e9, 1e9, 2e9, 2e9)) == EMPTY and w((-3e38, -3e38, 3e38, 3e38), (4, 1)) == (0, 0, 37, 51, 8, 8)  # clamped to +-2^20 first


def test_tube_rows_span_and_frame_map():
    boxes = np.array([[1, 1, 5, 5], [np.nan, 1, 5, 5], [2, 2, 6, 7], [3, 3, 3, 9]], dtype=np.float32)
    valid, win = tube_windows(boxes, 6, 10, 12, 4, 4, keep_aspect=False)
    assert valid.tolist() == [True, False, True, False, False, False]  # rows 4, 5 do not exist
    assert win[0].tolist() == [1, 1, 4, 4, 4, 4] and win[2].tolist() == [2, 2, 5, 4, 4, 4] and not win[[1, 3, 4, 5]].any()
    valid, _ = tube_windows(boxes, 4, 10, 12, 4, 4, span=(2, 3))
    assert valid.tolist() == [False, False, True, False]
    valid, _ = tube_windows(boxes, 5, 10, 12, 4, 4, span=(0, 2), frame_map=[0, 0, 2, -1, 9])
    assert valid.tolist() == [True, True, True, False, False]
    assert win.dtype == np.int32 and valid.dtype == bool


def test_keep_aspect_sizes_stay_inside_the_output_and_are_at_least_one():
    sides = [1, 2, 3, 7, 100, 719, 4096, 8192, 16384]
    outs = [1, 2, 5, 16, 33, 224, 4096]
    for ch in sides:
        for cw in sides:
            if cw > 8192:
                continue
            for oh in outs:
                for ow in outs:
                    rh, rw = out_size(ch, cw, oh, ow, True)
                    assert 1 <= rh <= oh and 1 <= rw <= ow and (rh == oh or rw == ow), (ch, cw, oh, ow, rh, rw)
                    assert out_size(ch, cw, oh, ow, False) == (oh, ow)
    assert out_size(1, 8192, 224, 224, True) == (1, 224) and out_size(16384, 1, 224, 224, True) == (224, 1)
    assert out_size(1, 16384, 16, 16, True) == (1, 16)  # the rule itself has no width limit
    assert out_size(20, 31, 16, 16, True) == (10, 16) and out_size(31, 20, 16, 16, True) == (16, 10)
    assert out_size(5, 5, 7, 9, True) == (7, 7) and out_size(3, 2, 33, 17, True) == (26, 17)  # (2 * 3 * 17 + 2) / 4 = 26


def test_composer_pads_bottom_right_and_zeroes_empty_frames():
    rng = np.random.default_rng(0)
    frames = rng.integers(0, 256, (2, 6, 8, 3), dtype=np.uint8)
    win = np.array([[1, 2, 3, 4, 3, 4], [0, 0, 0, 0, 0, 0]], dtype=np.int32)
    pixels, mask = compose(frames, win, 5, 6, lambda t, sub, rh, rw: sub)
    assert np.array_equal(pixels[0, :, :3, :4], frames[0, 1:4, 2:6].transpose(2, 0, 1))
    assert not pixels[0, :, 3:].any() and not pixels[0, :, :, 4:].any() and not pixels[1].any()
    assert mask[1].all() and not mask[0, :3, :4].any() and mask[0, 3:].all() and mask[0, :, 4:].all()


def test_float64_check_inputs_meet_the_near_tie_cap():
    """_check_single (tests/test_augment_gpu.py) asserts that at most 1 % of the float64 values lie within 1e-3 of a tie: a
    condition on the inputs alone.  The seeds of F64_CASES are chosen so that it holds."""
    for name, ((sh, sw), box, (oh, ow), want, _) in F64_CASES.items():
        assert box_window(box, sh, sw, oh, ow, (0, 1), False) == want
        wy0, wx0, ch, cw, rh, rw = want
        v = resample_f64(f64_frames(name)[:, wy0 : wy0 + ch, wx0 : wx0 + cw], rh, rw)
        near = np.abs(v - np.floor(v) - 0.5) < 1e-3
        print(name, near.sum(), near.size)
        assert near.sum() <= 0.01 * near.size, (name, int(near.sum()), near.size)


def test_crop_job_mirror_matches_the_header_and_the_abi_is_still_11():
    from tubedetr_amd import _hip

    src = open(os.path.join(ROOT, "include", "tubedetr_hip.h")).read()
    flat = " ".join(re.sub(r"/\*.*?\*/", "", src, flags=re.S).split())
    body = re.search(r"typedef struct td_crop_job \{(.*?)\} td_crop_job;", flat).group(1)
    names = [part.split()[-1].lstrip("*") for decl in body.split(";") if decl.strip() for part in decl.split(",")]
    assert names == [n for n, _ in _hip.CropJob._fields_], "td_crop_job and its ctypes mirror list different fields"
    assert _hip.EXPECTED_ABI == 11 and _hip.lib().td_abi_version() == 11
    assert "td_tube_crop" in _hip.EXPORTS and "td_tube_crop_table_bytes" in _hip.EXPORTS
    assert re.search(r"size_t td_tube_crop_table_bytes\(int n_jobs\);", flat)
    assert re.search(r"int td_tube_crop\(const td_crop_job\* jobs, int n_jobs, void\* table_host, void\* table_dev, size_t table_bytes, td_stream_t stream\);", flat)
    assert flat.index("td_sted_topk(") < flat.index("typedef struct td_crop_job")


def test_library_refuses_with_the_field_named_and_without_a_launch():
    from tubedetr_amd import _hip
    from tubedetr_amd.render import crop_job

    L = _hip.lib()
    table = ctypes.create_string_buffer(4096)

    def call(job, nbytes=4096):
        arr = (_hip.CropJob * 1)(job)
        rc = L.td_tube_crop(arr, 1, ctypes.addressof(table), ctypes.c_void_p(4096), nbytes, None)  # refused before anything is launched: no device is needed
        return rc, L.td_last_error()

    def job(fmt="rgb24"):
        return crop_job(1 << 20, 2, 6, 8, boxes=1 << 26, n_tube=2, dst=1 << 24, size=(4, 4), pix_fmt=fmt)

    cases = [("plane0", None, b"plane0"), ("boxes", None, b"boxes"), ("dst", None, b"dst"), ("fmt", 7, b"fmt"), ("sh", 0, b"sh"), ("sw", 8193, b"sw"),
             ("oh", 0, b"oh"), ("ow", 4097, b"ow"), ("n_tube", 0, b"n_tube"), ("margin_den", 0, b"margin_den"), ("margin_num", -1, b"margin_num"),
             ("margin_num", 5, b"margin_num"), ("keep_aspect", 2, b"keep_aspect"), ("T", -1, b"frame count T"), ("oh", 4097, b"oh"), ("sh", 16385, b"sh"),
             ("margin_den", 1025, b"margin_den"), ("pitch0", 23, b"pitch0"), ("frame_stride", 100, b"frame_stride")]
    for field, value, name in cases:
        j = job()
        setattr(j, field, value)
        rc, msg = call(j)
        assert rc != 0 and name in msg, (field, value, msg)
    for field, value, name in (("matrix", 2, b"matrix"), ("full_range", 2, b"full_range"), ("plane1", None, b"plane1"), ("plane2", None, b"plane2"), ("pitch1", 3, b"pitch1")):
        j = job("yuv420p")
        setattr(j, field, value)
        rc, msg = call(j)
        assert rc != 0 and name in msg, (field, value, msg)
    j = job()
    j.margin_den, j.margin_num = 3, 13  # 4 * den + 1
    rc, msg = call(j)
    assert rc != 0 and b"margin_num" in msg
    j.margin_num = 12
    j.T = 0  # a legal job without frames: nothing to launch
    assert call(j)[0] == 0
    j = job()
    j.sw, j.pitch0, j.frame_stride, j.ow = 8192, 3 * 8192, 3 * 8192 * 6, 4096
    rc, msg = call(j)
    assert rc != 0 and b"LDS" in msg and b"sw" in msg and b"ow" in msg
    rc, msg = call(job(), nbytes=L.td_tube_crop_table_bytes(1) - 1)
    assert rc != 0 and b"table" in msg
    assert L.td_tube_crop(None, 0, None, None, 0, None) != 0 and b"no jobs" in L.td_last_error()
    assert L.td_tube_crop_table_bytes(0) == 0 and L.td_tube_crop_table_bytes(3) % 256 == 0 and L.td_tube_crop_table_bytes(3) > 0
    assert L.td_tube_crop_table_bytes(16) <= 4096  # a batch of clips fits the smallest pooled table


def test_python_layer_refuses_bad_arguments():
    from tubedetr_amd import render
    from tubedetr_amd.render import TubeCrops, crop_job

    assert TubeCrops._fields == ("pixels", "mask", "valid", "windows")
    ok = crop_job(4096, 2, 5, 7, boxes=1 << 20, n_tube=3, dst=1 << 21, pix_fmt="yuv420p", size=(9, 11), margin=(1, 4))
    assert (ok.plane0, ok.plane1, ok.plane2) == (4096, 4096 + 35, 4096 + 35 + 12) and ok.frame_stride == 59 and (ok.pitch0, ok.pitch1, ok.pitch2) == (7, 4, 4)
    assert (ok.oh, ok.ow, ok.margin_num, ok.margin_den, ok.keep_aspect, ok.n_tube, ok.fmt) == (9, 11, 1, 4, 1, 3, 1)
    assert (ok.span, ok.frame_map, ok.mask, ok.valid, ok.windows) == (None,) * 5
    pitched = crop_job(0, 2, 5, 7, boxes=1 << 20, n_tube=3, dst=1 << 21, pix_fmt="nv12", planes=[4096, 8192], pitches=[16, 24], frame_stride=9000)
    assert (pitched.plane0, pitched.plane1, pitched.plane2, pitched.pitch0, pitched.pitch1, pitched.frame_stride) == (4096, 8192, None, 16, 24, 9000)
    base = {"src": 4096, "T": 1, "sh": 4, "sw": 4, "boxes": 1 << 20, "n_tube": 1, "dst": 1 << 21}
    for kw in ({"size": (0, 4)}, {"size": (4, 4097)}, {"size": (4,)}, {"size": 4}, {"size": (4.5, 4)}, {"margin": (-1, 4)}, {"margin": (5, 1)}, {"margin": (1, 0)},
               {"margin": (1, 1025)}, {"margin": 1}, {"margin": (0.25, 1)}, {"keep_aspect": 2}, {"pix_fmt": "yuv444p"}, {"sh": 0}, {"sw": 8193}, {"T": -1},
               {"n_tube": 0}, {"boxes": None}, {"dst": None}, {"matrix": "bt2020"}, {"planes": [4096, 8192]}):
        with pytest.raises(ValueError):
            crop_job(**{**base, **kw})
    # crop_tubes checks its lists and tensors before it builds a job; a stand-in for DeviceFrames keeps this on the host
    class Clip(render.DeviceFrames):
        def __post_init__(self):
            pass

    clip = Clip(torch.zeros(2 * 3 * 4 * 4, dtype=torch.uint8), 2, 4, 4, "rgb24")
    boxes = torch.zeros(2, 4)
    for args, kw in ((([clip, clip], [boxes]), {}), (([clip], [boxes]), {"span": [None, None]}), ((clip, boxes.double()), {}), ((clip, torch.zeros(2, 5)), {}),
                     ((clip, torch.zeros(4)), {}), ((clip, torch.zeros(0, 4)), {}), ((clip, None), {}), ((clip, boxes), {"span": torch.zeros(2, dtype=torch.int32)}),
                     ((clip, boxes), {"frame_map": torch.zeros(3, dtype=torch.int32)}), ((clip, boxes), {"frame_map": torch.zeros(2, dtype=torch.int64)}),
                     ((clip, boxes), {"size": (0, 4)}), ((clip, boxes), {"margin": (9, 2)}), ((clip, boxes.to("meta")), {}), (([clip, "clip"], [boxes, boxes]), {}),
                     (("clip", boxes), {})):
        with pytest.raises(ValueError):
            render.crop_tubes(*args, **kw)
    assert render.crop_tubes([], []) == []
