"""td_tube_overlay_multi without a GPU: the numpy restatement of its rule (tests/overlay_multi_ref.py) against
tests/overlay_ref.py for K = 1 and against bytes worked out by hand from the text in include/tubedetr_hip.h, the label font,
argument checking in Python and in the library, and the ABI."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from overlay_multi_ref import cursor_columns, overlay_multi_ref, timeline_row
from overlay_ref import overlay_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def planes_of(rng, T, sh, sw, fmt):
    ch, cw = (sh + 1) // 2, (sw + 1) // 2
    if fmt == "rgb24":
        return rng.integers(0, 256, (T, sh, sw, 3), dtype=np.uint8)
    Y = rng.integers(0, 256, (T, sh, sw), dtype=np.uint8)
    if fmt == "yuv420p":
        return (Y, rng.integers(0, 256, (T, ch, cw), dtype=np.uint8), rng.integers(0, 256, (T, ch, cw), dtype=np.uint8))
    return (Y, rng.integers(0, 256, (T, ch, cw, 2), dtype=np.uint8))


def same(a, b):
    a, b = (a if isinstance(a, tuple) else (a,)), (b if isinstance(b, tuple) else (b,))
    return all(x.dtype == np.uint8 and np.array_equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("fmt", ["rgb24", "yuv420p", "nv12"])
def test_oracle_with_one_tube_is_the_overlay_oracle(fmt):
    for seed, (sh, sw) in enumerate([(5, 7), (12, 9), (21, 30)]):
        rng = np.random.default_rng(seed)
        T = 5
        planes = planes_of(rng, T, sh, sw, fmt)
        x0, y0 = rng.uniform(-2, sw * 0.5, T), rng.uniform(-2, sh * 0.5, T)
        boxes = np.stack([x0, y0, x0 + rng.uniform(1.5, sw * 0.7, T), y0 + rng.uniform(1.5, sh * 0.7, T)], 1).astype(np.float32)
        boxes[3, 0] = np.nan
        heat = rng.integers(0, 256, (T, 3, 4), dtype=np.uint8)
        kw = dict(heat_color=(40, 60, 220), dim_color=(16, 128, 128), thickness=1 + seed, heat_alpha=160, dim_alpha=96)
        for span, fmap in ((None, None), ((1, 2), None), ((2, 9), [4, 0, 7, 2, -1])):
            want = overlay_ref(planes, fmt, boxes=boxes, span=span, frame_map=fmap, heat=heat, box_color=(200, 90, 30), **kw)
            got = overlay_multi_ref(planes, fmt, boxes=boxes[:, None, :], span=None if span is None else [span], frame_map=fmap, heat=heat,
                                    tube_color=((200, 90, 30),) + ((1, 2, 3),) * 7, **kw)
            assert same(got, want)
        assert same(overlay_multi_ref(planes, fmt, boxes=boxes[:, None, :], tube_color=((9, 9, 9),) * 8, thickness=2), overlay_ref(planes, fmt, boxes=boxes, box_color=(9, 9, 9)))


def test_oracle_rgb24_6x8_two_overlapping_boxes_by_hand():
    rng = np.random.default_rng(0)
    src = rng.integers(0, 256, (1, 6, 8, 3), dtype=np.uint8)
    # tube 0: columns [1, 5), rows [1, 5); tube 1: columns [3, 7), rows [2, 6); thickness 1; tube 1 is drawn after tube 0
    boxes = np.array([[[0.6, 1.4, 4.5, 5.2], [3.0, 2.0, 7.0, 6.0]]], dtype=np.float32)
    who = np.array([[0, 0, 0, 0, 0, 0, 0, 0],
                    [0, 1, 1, 1, 1, 0, 0, 0],
                    [0, 1, 0, 2, 2, 2, 2, 0],
                    [0, 1, 0, 2, 1, 0, 2, 0],
                    [0, 1, 1, 2, 1, 0, 2, 0],
                    [0, 0, 0, 2, 2, 2, 2, 0]])
    c0, c1 = (10, 20, 30), (200, 100, 50)
    want = src.copy()
    want[0][who == 1] = c0
    want[0][who == 2] = c1
    got = overlay_multi_ref(src, "rgb24", boxes=boxes, thickness=1, tube_color=(c0, c1) + ((0, 0, 0),) * 6)
    assert got.dtype == np.uint8 and np.array_equal(got, want)
    # the span of tube 1 excludes row 0: only tube 0 is drawn, and the frame is not dimmed (it lies in tube 0's span)
    got = overlay_multi_ref(src, "rgb24", boxes=boxes, span=[(0, 0), (1, 1)], thickness=1, dim_alpha=200, tube_color=(c0, c1) + ((0, 0, 0),) * 6)
    only0 = src.copy()
    only0[0, 1, 1:5] = only0[0, 4, 1:5] = only0[0, 1:5, 1] = only0[0, 1:5, 4] = c0
    assert np.array_equal(got, only0)
    # outside every span: dimmed, no box
    got = overlay_multi_ref(src, "rgb24", boxes=boxes, span=[(1, 1), (2, 5)], thickness=1, dim_alpha=256, dim_color=(9, 8, 7))
    assert (got == (9, 8, 7)).all()


def test_oracle_tag_2x3_at_scale_2_flips_below_the_edge_and_is_clipped_by_hand():
    """Grey frames of 100, tube colour 200, text colour 0, plate alpha 128: outline 200; plate (100 128 + 200 128 + 128) >> 8 = 150
    (200 on the outline); glyph a = (256 m + 127) / 255: m = 255 -> 256 -> 0; m = 0 -> unchanged; m = 128 -> a = 129: 150 ->
    (150 127 + 128) >> 8 = 74; m = 7 -> a = 7: 150 -> (150 249 + 128) >> 8 = 146."""
    src = np.full((1, 8, 10, 3), 100, np.uint8)
    style = dict(thickness=1, tube_color=((200, 200, 200),) * 8, tag_scale=2, tag_alpha=128, tag_text_color=(0, 0, 0))
    # box columns [6, 10), rows [2, 7): y0 - PH = 2 - 4 < 0, so the plate starts AT y0 = 2: rows [2, 6), columns [6, 12) cut at 10;
    # the third tag column is outside the frame
    tags = np.array([[[255, 0, 77], [0, 255, 77]]], dtype=np.uint8)
    got = overlay_multi_ref(src, "rgb24", boxes=np.array([[[6, 2, 10, 7]]], dtype=np.float32), tags=tags, **style)
    want = np.full((8, 10), 100)
    want[2] = [100] * 6 + [0, 0, 200, 200]
    want[3] = [100] * 6 + [0, 0, 150, 200]
    want[4] = [100] * 6 + [200, 150, 0, 0]
    want[5] = [100] * 6 + [200, 150, 0, 0]
    want[6] = [100] * 6 + [200, 200, 200, 200]
    assert all(np.array_equal(got[0, :, :, k], want) for k in range(3))
    # box columns [1, 5), rows [5, 8): there is room above, the plate is rows [1, 5), columns [1, 7)
    tags = np.array([[[128, 7, 0], [0, 0, 255]]], dtype=np.uint8)
    got = overlay_multi_ref(src, "rgb24", boxes=np.array([[[1, 5, 5, 8]]], dtype=np.float32), tags=tags, **style)
    want = np.full((8, 10), 100)
    want[1] = want[2] = [100, 74, 74, 146, 146, 150, 150, 100, 100, 100]
    want[3] = want[4] = [100, 150, 150, 150, 150, 0, 0, 100, 100, 100]
    want[5] = want[7] = [100, 200, 200, 200, 200, 100, 100, 100, 100, 100]
    want[6] = [100, 200, 100, 100, 200, 100, 100, 100, 100, 100]
    assert all(np.array_equal(got[0, :, :, k], want) for k in range(3))
    # a tube outside its span draws neither box nor tag
    assert np.array_equal(overlay_multi_ref(src, "rgb24", boxes=np.array([[[1, 5, 5, 8]]], dtype=np.float32), span=[(3, 4)], tags=tags, **style), src)


def test_oracle_yuv420p_5x7_one_row_lane_cursor_and_segment_edge_in_one_chroma_block_by_hand():
    Y, U, V = np.full((1, 5, 7), 100, np.uint8), np.full((1, 3, 4), 50, np.uint8), np.full((1, 3, 4), 200, np.uint8)
    # n_tube = sw = 7: column x is tube row x.  The frame is tube row 3; the span is rows 0..2.  The strip is luma row 4, alone in chroma row 2.
    gy, gu, gv = overlay_multi_ref((Y, U, V), "yuv420p", span=[(0, 2)], frame_map=[3], n_tube=7, K=1, lane_h=1, bar_color=(0, 128, 128), bar_alpha=128,
                                   seg_alpha=256, tube_color=((200, 100, 0),) * 8, cursor_color=(255, 60, 70))
    wy = np.full((5, 7), 100)
    wy[4] = [200, 200, 200, 255, 50, 50, 50]  # bar: (100 128 + 128) >> 8 = 50; segment on columns 0..2; cursor on column 3
    assert np.array_equal(gy[0], wy)
    # bar at 128: U (50 128 + 128 128 + 128) >> 8 = 89, V (200 128 + 128 128 + 128) >> 8 = 164.  Segment: block 0 (columns 0, 1) a = 256:
    # U 100, V 0; block 1 (columns 2, 3) a = (256 + 1) / 2 = 128: U (89 128 + 100 128 + 128) >> 8 = 95, V (164 128 + 128) >> 8 = 82.  Cursor:
    # block 1, a = 128: U (95 128 + 60 128 + 128) >> 8 = 78, V (82 128 + 70 128 + 128) >> 8 = 76.  Block 3 is column 6 alone.
    assert np.array_equal(gu[0], [[50] * 4, [50] * 4, [100, 78, 89, 89]])
    assert np.array_equal(gv[0], [[200] * 4, [200] * 4, [0, 76, 164, 164]])
    # a frame whose tube row is out of range gets no timeline
    out = overlay_multi_ref((Y, U, V), "yuv420p", frame_map=[7], n_tube=7, K=1, lane_h=1, bar_alpha=128, seg_alpha=256)
    assert same(out, (Y, U, V))
    # the dim layer comes first, the timeline last: frame 3 lies outside the span
    dy, _, _ = overlay_multi_ref((Y, U, V), "yuv420p", span=[(0, 2)], frame_map=[3], n_tube=7, K=1, lane_h=1, bar_alpha=0, seg_alpha=0, dim_alpha=256, dim_color=(7, 7, 7),
                                 cursor_color=(255, 60, 70))
    assert (dy[0, :4] == 7).all() and list(dy[0, 4]) == [7, 7, 7, 255, 7, 7, 7]


def test_timeline_columns_for_fewer_as_many_and_more_tube_rows_than_columns():
    sw = 8
    assert [timeline_row(x, 3, sw) for x in range(sw)] == [0, 0, 0, 1, 1, 1, 2, 2]
    assert [cursor_columns(r, 3, sw) for r in range(3)] == [(0, 2), (2, 5), (5, 8)]
    assert [timeline_row(x, 8, sw) for x in range(sw)] == list(range(8))
    assert [cursor_columns(r, 8, sw) for r in range(8)] == [(r, r + 1) for r in range(8)]
    assert [timeline_row(x, 20, sw) for x in range(sw)] == [0, 2, 5, 7, 10, 12, 15, 17]
    assert cursor_columns(0, 20, sw) == (0, 1) and cursor_columns(7, 20, sw) == (2, 3) and cursor_columns(19, 20, sw) == (7, 8)  # never empty
    assert timeline_row(16383, 1 << 20, 16384) == (1 << 20) - 64 and cursor_columns((1 << 20) - 1, 1 << 20, 16384) == (16383, 16384)  # 2^34: past int32
    # the segment of span (1, 1) with 3 rows on 8 columns is columns 3..5; the oracle draws exactly those
    src = np.zeros((1, 2, sw, 3), np.uint8)
    got = overlay_multi_ref(src, "rgb24", span=[(1, 1)], frame_map=[0], n_tube=3, K=1, lane_h=1, bar_alpha=0, seg_alpha=256, tube_color=((255, 255, 255),) * 8,
                            cursor_color=(9, 9, 9))
    assert list(got[0, 1, :, 0]) == [9, 9, 0, 255, 255, 255, 0, 0] and (got[0, 0] == 0).all()


def test_label_tags_font():
    from tubedetr_amd.render import _FONT, label_tags

    t = label_tags(["1-", "a"])
    assert t.dtype == torch.uint8 and tuple(t.shape) == (2, 9, 13) and set(t.unique().tolist()) == {0, 255}
    one = [[0, 0, 1, 0, 0], [0, 1, 1, 0, 0], [0, 0, 1, 0, 0], [0, 0, 1, 0, 0], [0, 0, 1, 0, 0], [0, 0, 1, 0, 0], [0, 1, 1, 1, 0]]
    dash = [[0] * 5] * 3 + [[1] * 5] + [[0] * 5] * 3
    assert (t[0, 1:8, 1:6] // 255).tolist() == one and (t[0, 1:8, 7:12] // 255).tolist() == dash
    assert not t[:, 0].any() and not t[:, 8].any() and not t[:, :, 0].any() and not t[:, :, 6].any() and not t[:, :, 12].any()  # margin and gaps
    assert not t[1, :, 7:].any(), "the shorter label is padded with zeros"
    assert torch.equal(label_tags(["a"]), label_tags(["A"])) and torch.equal(label_tags(["abc xyz"]), label_tags(["ABC XYZ"]))
    chars = "0123456789ABCDEFGHIJKLMNOPQRSTUVWXYZ .:%-#"
    assert sorted(_FONT) == sorted(chars)
    glyphs = {c: label_tags([c])[0] for c in chars}
    assert all(tuple(g.shape) == (9, 7) for g in glyphs.values())
    assert all(not torch.equal(glyphs[a], glyphs[b]) for i, a in enumerate(chars) for b in chars[i + 1:])
    assert not glyphs[" "].any() and all(glyphs[c].any() for c in chars if c != " ")
    for bad in (["é"], ["a_b"], ["ok", "no!"], [], ["x"] * 9, "abc", [3], ["A" * 43]):
        with pytest.raises(ValueError):
            label_tags(bad)
    assert label_tags(["A" * 42]).shape[2] == 253 and label_tags([""]).shape == (1, 9, 1)


def test_python_layer_refuses_bad_arguments():
    from tubedetr_amd.render import PALETTE, TubeSetStyle, annotate_tubes, overlay_multi_job

    s = TubeSetStyle()
    assert s.colors[0] == (0xFA, 0xFF, 0x00) and len(s.colors) == 8 and len(set(s.colors)) == 8 and s.colors == PALETTE
    assert s.thickness == 2 and s.heat_alpha == 0 and s.dim_alpha == 0 and s.lane_h == 0
    for kw in ({"thickness": 0}, {"heat_alpha": 257}, {"dim_alpha": -1}, {"tag_alpha": 300}, {"bar_alpha": -2}, {"seg_alpha": 1.5}, {"colors": PALETTE[:7]},
               {"colors": PALETTE[:7] + ((1, 2, 256),)}, {"tag_text_color": (1, 2)}, {"bar_color": (0, 0, -1)}, {"cursor_color": "white"}, {"tag_scale": 0}, {"tag_scale": 9},
               {"lane_h": -1}, {"lane_h": 65}):
        with pytest.raises(ValueError):
            TubeSetStyle(**kw)
    ok = overlay_multi_job(4096, 2, 5, 7, pix_fmt="yuv420p", boxes=8192, n_tube=2, K=3, tags=12288, tag_hw=(9, 13), tag_scale=2, lane_h=1)
    assert (ok.dst0, ok.dst1, ok.dst2) == (ok.src0, ok.src1, ok.src2) == (4096, 4096 + 35, 4096 + 35 + 12) and ok.K == 3 and list(ok.tube_color[0]) == [0xFA, 0xFF, 0]
    base = {"src": 4096, "T": 1, "sh": 16, "sw": 16, "boxes": 8192, "n_tube": 4}
    for kw in ({"pix_fmt": "yuv444p"}, {"sh": 0}, {"sw": 16385}, {"T": -1}, {"K": 0}, {"K": 9}, {"thickness": 0}, {"heat_alpha": 300}, {"dim_alpha": -3},
               {"heat": 4096, "heat_hw": (2, 257)}, {"tags": 4096, "tag_hw": (0, 5)}, {"tags": 4096, "tag_hw": (33, 5)}, {"tags": 4096, "tag_hw": (9, 257)},
               {"tags": 4096, "tag_hw": (9, 7), "tag_scale": 0}, {"tags": 4096, "tag_hw": (9, 7), "tag_scale": 9}, {"tags": 4096, "tag_hw": (9, 7), "boxes": None},
               {"tag_alpha": 257}, {"lane_h": 65}, {"lane_h": -1}, {"lane_h": 2, "n_tube": 0}, {"lane_h": 2, "n_tube": (1 << 20) + 1}, {"lane_h": 3, "K": 6},
               {"bar_alpha": 257}, {"seg_alpha": -1}, {"tube_colors": PALETTE[:3]}, {"cursor_color": (0, 0, 300)}):
        with pytest.raises(ValueError):
            overlay_multi_job(**{**base, **kw})
    assert annotate_tubes([], None) == []
    with pytest.raises(ValueError):
        annotate_tubes([object()], [None])  # not DeviceFrames


def test_library_refuses_every_limit_with_its_own_message():
    from tubedetr_amd import _hip
    from tubedetr_amd.render import overlay_multi_job

    L = _hip.lib()
    table = ctypes.create_string_buffer(4096)

    def call(job):
        arr = (_hip.OverlayMultiJob * 1)(job)
        rc = L.td_tube_overlay_multi(arr, 1, ctypes.addressof(table), ctypes.c_void_p(4096), 4096, None)
        return rc, L.td_last_error()

    def fresh(**kw):
        return overlay_multi_job(1 << 20, 2, 16, 24, dst=1 << 24, boxes=1 << 26, n_tube=4, K=2, tags=1 << 27, tag_hw=(9, 13), tag_scale=2, tag_alpha=100, lane_h=3,
                                 bar_alpha=10, seg_alpha=20, **kw)

    # the host checks come before the launch: each of these returns its error without touching a device
    for field, value, word in (("fmt", 7, b"fmt"), ("T", -1, b"T ="), ("sw", 16385, b"sw"), ("sh", 0, b"sh"), ("n_tube", -1, b"n_tube"), ("K", 0, b"K ="), ("K", 9, b"K ="),
                               ("thickness", 0, b"thickness"), ("heat_alpha", 257, b"heat_alpha"), ("dim_alpha", -1, b"dim_alpha"), ("tag_alpha", 257, b"tag_alpha"),
                               ("bar_alpha", 257, b"bar_alpha"), ("seg_alpha", -1, b"seg_alpha"), ("tag_h", 0, b"tag_h"), ("tag_h", 33, b"tag_h"), ("tag_w", 0, b"tag_w"),
                               ("tag_w", 257, b"tag_w"), ("tag_scale", 0, b"tag_scale"), ("tag_scale", 9, b"tag_scale"), ("boxes", None, b"tags without boxes"),
                               ("lane_h", -1, b"lane_h"), ("lane_h", 65, b"lane_h"), ("n_tube", 0, b"n_tube"), ("n_tube", (1 << 20) + 1, b"n_tube"), ("lane_h", 9, b"lane_h"),
                               ("src0", None, b"src0 is null"), ("dst_pitch0", 71, b"dst_pitch0")):
        job = fresh()
        setattr(job, field, value)
        rc, msg = call(job)
        assert rc != 0 and word in msg and b"td_tube_overlay_multi: job 0" in msg, (field, value, msg)
    job = fresh()
    job.lane_h, job.K = 8, 3  # each within its own range, together 24 rows for a frame of 16
    rc, msg = call(job)
    assert rc != 0 and b"do not fit" in msg
    job = overlay_multi_job(1 << 20, 2, 6, 8, dst=1 << 24, heat=1 << 26, heat_hw=(2, 2), n_tube=2)
    job.mw = 257
    rc, msg = call(job)
    assert rc != 0 and b"mw" in msg
    job = overlay_multi_job(1 << 20, 2, 6, 8, dst=(1 << 20) + 1)  # shifted by one byte: neither in place nor apart
    rc, msg = call(job)
    assert rc != 0 and b"overlaps" in msg and b"dst0" in msg
    job = overlay_multi_job(1 << 20, 2, 6, 8, dst=(1 << 20) + 6 * 8 * 3)  # frame t written over frame t + 1
    rc, msg = call(job)
    assert rc != 0 and b"overlaps" in msg
    # limits that only count with their layer: tag fields without tags and a timeline's n_tube without a timeline are not looked at
    job = overlay_multi_job(1 << 20, 0, 6, 8, dst=1 << 24, n_tube=0)
    job.tag_scale, job.tag_h = 99, -5
    assert call(job)[0] == 0  # T = 0: accepted, nothing to launch
    assert L.td_tube_overlay_multi(None, 0, None, None, 0, None) != 0 and b"no jobs" in L.td_last_error()
    rc = L.td_tube_overlay_multi((_hip.OverlayMultiJob * 1)(fresh()), 1, ctypes.addressof(table), ctypes.c_void_p(4096), 16, None)
    assert rc != 0 and b"td_tube_overlay_multi_table_bytes" in L.td_last_error()
    nb = L.td_tube_overlay_multi_table_bytes
    assert nb(0) == 0 and nb(3) % 256 == 0 and nb(3) > 0


def test_overlay_multi_job_mirror_matches_the_header_and_the_abi_is_still_11():
    from tubedetr_amd import _hip
    from tubedetr_amd.render import _JOB_TYPES

    src = open(os.path.join(ROOT, "include", "tubedetr_hip.h")).read()
    flat = " ".join(re.sub(r"/\*.*?\*/", "", src, flags=re.S).split())
    body = re.search(r"typedef struct td_overlay_multi_job \{(.*?)\} td_overlay_multi_job;", flat).group(1)
    names = [re.sub(r"\[\d+\]", "", part).split()[-1].lstrip("*") for decl in body.split(";") if decl.strip() for part in decl.split(",")]
    assert names == [n for n, _ in _hip.OverlayMultiJob._fields_], "td_overlay_multi_job and its ctypes mirror list different fields"
    assert len(names) == 43
    # the frames side is td_overlay_job's, field for field
    assert _hip.OverlayMultiJob._fields_[:18] == _hip.OverlayJob._fields_[:18]
    assert _hip.OverlayMultiJob.tube_color.size == 24 and _hip.OverlayMultiJob.tube_color.offset + 24 == _hip.OverlayMultiJob.heat_color.offset
    assert _hip.EXPECTED_ABI == 11 and _hip.lib().td_abi_version() == 11
    assert "td_tube_overlay_multi" in _hip.EXPORTS and "td_tube_overlay_multi_table_bytes" in _hip.EXPORTS
    assert _JOB_TYPES["td_tube_overlay_multi"] == "OverlayMultiJob"
