"""Grounded-tube overlay without a GPU: the numpy reference (tests/overlay_ref.py) against bytes worked out by hand from
the rule in include/tubedetr_hip.h, the colour conversion, argument checking in Python and in the library, and the ABI."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from overlay_ref import overlay_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_reference_rgb24_6x5_thickness_1_box_by_hand():
    rng = np.random.default_rng(0)
    src = rng.integers(0, 256, (1, 6, 5, 3), dtype=np.uint8)
    # floorf(v + 0.5): 0.6 -> 1, 1.4 -> 1, 3.5 -> 4, 4.5 -> 5: columns [1, 4), rows [1, 5); the inner [2, 3) x [2, 4) stays
    box = np.array([[0.6, 1.4, 3.5, 4.5]], dtype=np.float32)
    outline = np.array([[0, 0, 0, 0, 0],
                        [0, 1, 1, 1, 0],
                        [0, 1, 0, 1, 0],
                        [0, 1, 0, 1, 0],
                        [0, 1, 1, 1, 0],
                        [0, 0, 0, 0, 0]], dtype=bool)
    want = src.copy()
    want[0][outline] = (250, 255, 0)
    got = overlay_ref(src, "rgb24", boxes=box, thickness=1, box_color=(250, 255, 0))
    assert got.dtype == np.uint8 and np.array_equal(got, want)
    # thickness 2 >= half the 3-column box: filled
    filled = src.copy()
    filled[0, 1:5, 1:4] = (250, 255, 0)
    assert np.array_equal(overlay_ref(src, "rgb24", boxes=box, thickness=2), filled)


def test_reference_yuv420p_5x7_last_row_and_column_share_chroma_by_hand():
    Y, U, V = np.full((1, 5, 7), 100, np.uint8), np.full((1, 3, 4), 50, np.uint8), np.full((1, 3, 4), 200, np.uint8)
    box = np.array([[4, 2, 7, 5]], dtype=np.float32)  # columns [4, 7), rows [2, 5); thickness 1 leaves pixel (3, 5)
    gy, gu, gv = overlay_ref((Y, U, V), "yuv420p", boxes=box, thickness=1, box_color=(200, 100, 0))
    wy = np.full((5, 7), 100)
    wy[2, 4:7] = wy[4, 4:7] = 200
    wy[3, 4] = wy[3, 6] = 200
    assert np.array_equal(gy[0], wy)
    # block (1, 2): 3 of its 4 pixels drawn, a = (768 + 2) / 4 = 192: U = (50 64 + 100 192 + 128) >> 8 = 88, V = (200 64 + 128) >> 8 = 50;
    # block (1, 3) has 2 pixels (column 6), block (2, 2) has 2 (row 4), block (2, 3) has 1: all drawn, a = 256
    assert np.array_equal(gu[0], [[50, 50, 50, 50], [50, 50, 88, 100], [50, 50, 100, 100]])
    assert np.array_equal(gv[0], [[200, 200, 200, 200], [200, 200, 50, 0], [200, 200, 0, 0]])
    # a 1 x 1 map of 255: h = (256 256 255 + 32768) >> 16 = 255, a = (255 128 + 127) / 255 = 128 on every pixel and every block;
    # frame 1 lies outside the span (0, 0) and is dimmed first: a = 64 towards (0, 128, 128), then the heat
    Y2, U2, V2 = (np.concatenate([p, p]) for p in (Y, U, V))
    hy, hu, hv = overlay_ref((Y2, U2, V2), "yuv420p", span=(0, 0), heat=np.full((2, 1, 1), 255, np.uint8), heat_alpha=128, heat_color=(40, 60, 80),
                             dim_alpha=64, dim_color=(0, 128, 128))
    assert (hy[0] == (100 * 128 + 40 * 128 + 128) >> 8).all() and (hy[0] == 70).all()
    assert (hu[0] == 55).all() and (hv[0] == 140).all()
    # dim: Y (100 192 + 128) >> 8 = 75, U (50 192 + 128 64 + 128) >> 8 = 70, V (200 192 + 128 64 + 128) >> 8 = 182; then heat at 128
    assert (hy[1] == (75 * 128 + 40 * 128 + 128) >> 8).all() and (hy[1] == 58).all()
    assert (hu[1] == (70 * 128 + 60 * 128 + 128) >> 8).all() and (hv[1] == (182 * 128 + 80 * 128 + 128) >> 8).all()


def test_reference_frame_map_span_and_degenerate_boxes():
    rng = np.random.default_rng(1)
    src = rng.integers(0, 256, (4, 6, 8, 3), dtype=np.uint8)
    boxes = np.array([[1, 1, 5, 5], [np.nan, 1, 5, 5], [3, 3, 3, 9], [1, 1, np.inf, 5]], dtype=np.float32)
    got = overlay_ref(src, "rgb24", boxes=boxes, frame_map=[0, 1, 2, 7], thickness=1)
    assert not np.array_equal(got[0], src[0]) and np.array_equal(got[1:], src[1:])  # NaN, x1 <= x0, row 7 of 4: nothing drawn
    got = overlay_ref(src, "rgb24", boxes=boxes, frame_map=[0, 0, 0, 9], span=(1, 2), dim_alpha=256, dim_color=(9, 8, 7))
    assert (got[:3] == (9, 8, 7)).all() and np.array_equal(got[3], src[3])  # row 0 lies outside the span: dimmed, no box; row 9 of 4: a plain copy


@pytest.mark.parametrize("full_range", [False, True], ids=["limited", "full"])
@pytest.mark.parametrize("matrix", ["bt601", "bt709"])
def test_color_in_space_within_0p502_of_the_float64_formula(matrix, full_range):
    from tubedetr_amd.render import color_in_space

    kr, kb = (0.299, 0.114) if matrix == "bt601" else (0.2126, 0.0722)
    kg = 1 - kr - kb
    sy, sc, yo = (1.0, 1.0, 0.0) if full_range else (219 / 255, 224 / 255, 16.0)
    worst = 0.0
    levels = list(range(0, 256, 15)) + [1, 254]
    for r in levels:
        for g in levels:
            for b in levels:
                y = kr * r + kg * g + kb * b
                want = np.clip([yo + sy * y, 128 + sc * (b - y) / (2 * (1 - kb)), 128 + sc * (r - y) / (2 * (1 - kr))], 0, 255)
                got = color_in_space((r, g, b), "yuv420p", matrix, full_range)
                assert got == color_in_space((r, g, b), "nv12", matrix, full_range)
                worst = max(worst, np.abs(np.array(got) - want).max())
    assert worst <= 0.502, worst
    assert color_in_space((1, 2, 3), "rgb24") == (1, 2, 3)
    if not full_range:
        assert color_in_space((0, 0, 0), "yuv420p", matrix) == (16, 128, 128) and color_in_space((255, 255, 255), "yuv420p", matrix) == (235, 128, 128)


def test_python_layer_refuses_bad_arguments():
    from tubedetr_amd.render import DeviceFrames, TubeStyle, color_in_space, overlay_job

    assert TubeStyle().box_color == (0xFA, 0xFF, 0x00) and TubeStyle().thickness == 2 and TubeStyle().heat_alpha == 0 and TubeStyle().dim_alpha == 0
    for kw in ({"thickness": 0}, {"heat_alpha": 257}, {"dim_alpha": -1}, {"box_color": (1, 2)}, {"heat_color": (1, 2, 256)}):
        with pytest.raises(ValueError):
            TubeStyle(**kw)
    buf = torch.zeros(3 * 4 * 4, dtype=torch.uint8)
    for args in ((buf, 1, 4, 4, "bgr24"), (buf, 1, 0, 4, "rgb24"), (buf, 1, 4, 20000, "rgb24"), (buf, 1, 4, 4, "rgb24", "bt2020"), (buf, 1, 4, 4, "rgb24"),
                 (buf.float(), 1, 4, 4, "rgb24")):
        with pytest.raises(ValueError):  # the last two: a well-formed clip that is not a uint8 tensor on the device
            DeviceFrames(*args)
    ok = overlay_job(4096, 2, 5, 7, pix_fmt="yuv420p", thickness=1)
    assert (ok.dst0, ok.dst1, ok.dst2) == (ok.src0, ok.src1, ok.src2) == (4096, 4096 + 35, 4096 + 35 + 12) and ok.src_frame_stride == ok.dst_frame_stride == 59
    for kw in ({"pix_fmt": "yuv444p"}, {"sh": 0}, {"sw": 16385}, {"thickness": 0}, {"heat_alpha": 300}, {"dim_alpha": -3}, {"T": -1},
               {"heat": 4096, "heat_hw": (0, 3)}, {"heat": 4096, "heat_hw": (2, 257)}, {"box_color": (0, 0, 300)}):
        with pytest.raises(ValueError):
            overlay_job(**{"src": 4096, "T": 1, "sh": 4, "sw": 4, **kw})
    with pytest.raises(ValueError):
        color_in_space((0, 0, 0), "yuv410p")


def test_library_refuses_with_its_own_message():
    from tubedetr_amd import _hip
    from tubedetr_amd.render import overlay_job

    L = _hip.lib()
    table = ctypes.create_string_buffer(4096)

    def call(job):
        arr = (_hip.OverlayJob * 1)(job)
        rc = L.td_tube_overlay(arr, 1, ctypes.addressof(table), ctypes.c_void_p(4096), 4096, None)
        return rc, L.td_last_error()

    job = overlay_job(1 << 20, 2, 6, 8, dst=1 << 24, boxes=1 << 26, n_tube=2)
    job.fmt = 7
    rc, msg = call(job)
    assert rc != 0 and b"fmt" in msg
    job = overlay_job(1 << 20, 2, 6, 8, dst=1 << 24, boxes=1 << 26, n_tube=2)
    job.thickness = 0
    rc, msg = call(job)
    assert rc != 0 and b"thickness" in msg
    job = overlay_job(1 << 20, 2, 6, 8, dst=(1 << 20) + 1)  # shifted by one byte: neither in place nor apart
    rc, msg = call(job)
    assert rc != 0 and b"overlaps" in msg and b"dst0" in msg
    job = overlay_job(1 << 20, 2, 6, 8, dst=(1 << 20) + 6 * 8 * 3, pix_fmt="rgb24")  # frame t written over frame t + 1
    rc, msg = call(job)
    assert rc != 0 and b"overlaps" in msg
    for field, name in (("heat_alpha", b"heat_alpha"), ("dim_alpha", b"dim_alpha")):
        job = overlay_job(1 << 20, 2, 6, 8, dst=1 << 24)
        setattr(job, field, 257)
        rc, msg = call(job)
        assert rc != 0 and name in msg
    job = overlay_job(1 << 20, 2, 6, 8, dst=1 << 24, heat=1 << 26, heat_hw=(2, 2), n_tube=2)
    job.mw = 257
    rc, msg = call(job)
    assert rc != 0 and b"mw" in msg
    job = overlay_job(1 << 20, 2, 6, 8, dst=1 << 24)
    job.sw = 16385
    rc, msg = call(job)
    assert rc != 0 and b"sw" in msg
    assert L.td_tube_overlay(None, 0, None, None, 0, None) != 0 and b"no jobs" in L.td_last_error()
    assert L.td_tube_overlay_table_bytes(0) == 0 and L.td_tube_overlay_table_bytes(3) % 256 == 0 and L.td_tube_overlay_table_bytes(3) > 0


def test_overlay_job_mirror_matches_the_header_and_the_abi_is_still_11():
    from tubedetr_amd import _hip

    src = open(os.path.join(ROOT, "include", "tubedetr_hip.h")).read()
    flat = " ".join(re.sub(r"/\*.*?\*/", "", src, flags=re.S).split())
    body = re.search(r"typedef struct td_overlay_job \{(.*?)\} td_overlay_job;", flat).group(1)
    names = [re.sub(r"\[\d+\]", "", part).split()[-1].lstrip("*") for decl in body.split(";") if decl.strip() for part in decl.split(",")]
    assert names == [n for n, _ in _hip.OverlayJob._fields_], "td_overlay_job and its ctypes mirror list different fields"
    assert _hip.EXPECTED_ABI == 11 and _hip.lib().td_abi_version() == 11
    assert "td_tube_overlay" in _hip.EXPORTS and "td_tube_overlay_table_bytes" in _hip.EXPORTS
