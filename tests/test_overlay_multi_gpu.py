"""td_tube_overlay_multi and tubedetr_amd.render.annotate_tubes on the GPU.  Every comparison is bit equality (torch.equal)
of whole buffers with the numpy restatement of the header's rule (tests/overlay_multi_ref.py), or of two device results.

The buffers are those of tests/test_overlay_gpu.py: a job's planes lie in ONE buffer full of random canary bytes, 64 of them in
front of every plane of every frame (so also behind it), rows at a pitch of their length + 3 (+ 0 where a test says so); the
whole buffer is compared, so a byte written into the padding, in front of a plane or behind it shows as a difference.  Sizes are
rows x columns.  A spec's reference is computed once and shared by the modes (in place, apart, shifted by 1 byte, by 4)."""
import os
import re

import numpy as np
import pytest
import torch

from overlay_multi_ref import overlay_multi_ref
from test_overlay_gpu import DST_GAP, as_rows, edge_boxes, layout, make_planes, place

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FMTS = ["rgb24", "yuv420p", "nv12"]
SIZES = [(5, 7), (37, 53), (130, 258)]  # odd sides; 258 = 2 mod 4; 130 rows = more than one 16-row tile, 3 x 258 bytes = more than one wave
MODES = ("inplace", "apart", "shifted", "dword")
TUBE_COLORS = ((200, 90, 30), (30, 200, 90), (90, 30, 200), (250, 250, 10), (10, 250, 250), (250, 10, 250), (128, 128, 128), (255, 255, 255))
COLORS = {"tube_color": TUBE_COLORS, "heat_color": (40, 60, 220), "dim_color": (16, 128, 128), "tag_text_color": (5, 120, 140), "bar_color": (60, 70, 80), "cursor_color": (240, 16, 128)}
STYLE_KEYS = {"tube_color": "tube_colors", "heat_color": "heat_color", "dim_color": "dim_color", "tag_text_color": "tag_text_color", "bar_color": "bar_color",
              "cursor_color": "cursor_color", "thickness": "thickness", "heat_alpha": "heat_alpha", "dim_alpha": "dim_alpha", "tag_scale": "tag_scale", "tag_alpha": "tag_alpha",
              "lane_h": "lane_h", "bar_alpha": "bar_alpha", "seg_alpha": "seg_alpha"}  # the reference's keyword -> overlay_multi_job's


def spec_geometry(s):
    rows = as_rows(s["planes"], s["fmt"])
    return rows, rows[0].shape[0], rows[0].shape[1], (rows[0].shape[2] // 3 if s["fmt"] == "rgb24" else rows[0].shape[2])


def spec_K(s):
    return s.get("K", s["boxes"].shape[1] if s.get("boxes") is not None else len(s["span"]) if s.get("span") is not None else 1)


def spec_n_tube(s):
    return s.get("n_tube", len(s["boxes"]) if s.get("boxes") is not None else len(s["heat"]) if s.get("heat") is not None else 2 ** 31 - 1)


def device_inputs(s, dev):
    t = {k: None for k in ("boxes", "span", "frame_map", "heat", "tags")}
    if s.get("boxes") is not None:
        t["boxes"] = torch.from_numpy(np.ascontiguousarray(s["boxes"], dtype=np.float32)).to(dev)
    if s.get("span") is not None:
        t["span"] = torch.tensor(s["span"], dtype=torch.int64, device=dev)
    if s.get("frame_map") is not None:
        t["frame_map"] = torch.tensor(s["frame_map"], dtype=torch.int32, device=dev)
    if s.get("heat") is not None:
        t["heat"] = torch.from_numpy(np.ascontiguousarray(s["heat"])).to(dev)
    if s.get("tags") is not None:
        t["tags"] = torch.from_numpy(np.ascontiguousarray(s["tags"])).to(dev)
    return t


def reference_rows(s):
    s = dict(s)
    fmt, planes = s.pop("fmt"), s.pop("planes")
    if s.pop("T_job", None) == 0:
        return as_rows(planes, fmt)  # a job of no frames writes nothing
    return as_rows(overlay_multi_ref(planes, fmt, **s), fmt)


def run(specs, modes=MODES, pad=3):
    """One launch per mode over all specs.  spec: fmt, planes, and overlay_multi_ref's keyword arguments (numpy / tuples); T_job = 0 makes
    the job one of no frames over the same buffers, which must come back untouched.  Modes as in
    tests/test_overlay_gpu.py: "inplace" - the destination planes ARE the source planes; "apart" - another buffer of the same
    layout; "shifted" / "dword" - another buffer whose planes start 1 / 4 bytes later.  Asserts bit equality of every destination
    buffer with the reference placed into that buffer's canaries, and that a separate source is untouched.  Returns the reference
    rows per spec."""
    from tubedetr_amd.render import overlay_multi_job, tube_overlay_multi

    dev = torch.device(DEV)
    wants = [reference_rows(s) for s in specs]
    for mode in modes:
        rng = np.random.default_rng(99)
        jobs, keep, checks = [], [], []
        for s, want_rows in zip(specs, wants):
            rows, T, sh, sw = spec_geometry(s)
            slay = layout(rows, 64, pad)
            src = place(rng.integers(0, 256, slay["total"], dtype=np.uint8), rows, slay)
            d_src = torch.from_numpy(src).to(dev)
            if mode == "inplace":
                dlay, d_dst, want = slay, d_src, place(src.copy(), want_rows, slay)
            else:
                dlay = layout(rows, DST_GAP[mode], pad)
                dst = rng.integers(0, 256, dlay["total"], dtype=np.uint8)
                d_dst, want = torch.from_numpy(dst).to(dev), (dst.copy() if s.get("T_job") == 0 else place(dst.copy(), want_rows, dlay))
            t = device_inputs(s, dev)
            style = {STYLE_KEYS[k]: s[k] for k in STYLE_KEYS if k in s}
            jobs.append(overlay_multi_job(0, s.get("T_job", T), sh, sw, pix_fmt=s["fmt"], n_tube=spec_n_tube(s), K=spec_K(s), heat_hw=tuple(s["heat"].shape[1:]) if s.get("heat") is not None else (0, 0),
                                          tag_hw=tuple(s["tags"].shape[1:]) if s.get("tags") is not None else (0, 0),
                                          src_planes=[d_src.data_ptr() + o for o in slay["offs"]], src_pitches=slay["pitches"], src_frame_stride=slay["stride"],
                                          dst_planes=[d_dst.data_ptr() + o for o in dlay["offs"]], dst_pitches=dlay["pitches"], dst_frame_stride=dlay["stride"],
                                          **{k: (v.data_ptr() if v is not None else None) for k, v in t.items()}, **style))
            keep.append(t)
            checks.append((d_dst, want, None if mode == "inplace" else (d_src, src)))
        tables = tube_overlay_multi(jobs, dev)
        torch.cuda.synchronize()
        del tables
        for i, (d_dst, want, source) in enumerate(checks):
            got = d_dst.cpu()
            assert torch.equal(got, torch.from_numpy(want)), f"job {i} ({mode}): {(got.numpy() != want).sum()} of {want.size} bytes differ from the reference"
            if source is not None:
                assert torch.equal(source[0].cpu(), torch.from_numpy(source[1])), f"job {i} ({mode}): the source was written"
    return wants


def tubes(rng, n, K, sh, sw):
    """n x K boxes whose top-left corner lies in the frame's first half."""
    x0, y0 = rng.uniform(0, sw * 0.5, (n, K)), rng.uniform(0, sh * 0.5, (n, K))
    return np.stack([x0, y0, x0 + rng.uniform(1.5, sw * 0.5, (n, K)), y0 + rng.uniform(1.5, sh * 0.5, (n, K))], 2).astype(np.float32)


def labels(K):
    from tubedetr_amd.render import label_tags

    return label_tags([f"{k}:A" for k in range(K)]).numpy()  # (K, 9, 19)


def full_spec(rng, fmt, sh, sw, K, T=3, n_tube=4, heat=True, lane_h=None, tag_scale=1):
    """Every layer at once.  Tube k's span is rows k % 3 .. 2 (so tubes drop out frame by frame); tube row 3 lies outside every
    span and is dimmed."""
    if lane_h is None:
        lane_h = 0 if K > sh else 1 if K * 3 > sh else 3
    return dict(fmt=fmt, planes=make_planes(rng, T, sh, sw, fmt), boxes=tubes(rng, n_tube, K, sh, sw), span=[(k % 3, 2) for k in range(K)], frame_map=[1, 3, 0, 2][:T],
                heat=rng.integers(0, 256, (n_tube, 3, 5), dtype=np.uint8) if heat else None, tags=labels(K), thickness=2, heat_alpha=160, dim_alpha=96, tag_scale=tag_scale,
                tag_alpha=200, lane_h=lane_h, bar_alpha=150, seg_alpha=230, **COLORS)


@pytest.mark.parametrize("K", [1, 3, 8])
@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_all_layers_in_place_apart_and_shifted(size, fmt, K):
    sh, sw = size
    spec = full_spec(np.random.default_rng(sh + K), fmt, sh, sw, K, tag_scale=2 if sh > 100 else 1)
    (want,) = run([spec])
    assert any(not np.array_equal(x, y) for x, y in zip(want, as_rows(spec["planes"], fmt))), "the overlay changed nothing"


def kernel_tile_cols(sw):
    """The column tile that td_tube_overlay_multi gives a frame of sw columns, from the kernel's constant and the host's arithmetic."""
    src = open(os.path.join(ROOT, "tubedetr_amd", "csrc", "overlay_multi.hip")).read()
    max_cols = int(re.search(r"constexpr int kMaxTileCols = (\d+);", src).group(1))
    ntx = -(-sw // max_cols)
    return (-(-sw // ntx) + 31) & ~31, int(re.search(r"constexpr int kTileRows = (\d+);", src).group(1))


@pytest.mark.parametrize("fmt", FMTS)
def test_a_frame_wider_than_the_column_tile_with_tags_and_outlines_across_the_tile_edges(fmt):
    sh, sw = 18, 2100
    tw, tr = kernel_tile_cols(sw)
    assert 0 < tw < sw and 0 < tr < sh, "the frame must span two tiles in both directions"
    # tube 0: its left bar (thickness 3) and its tag start one column before the column edge and cross it; its top bar crosses the row edge;
    # tube 1: its right bar crosses the column edge from the left, its tag (above the box, no room: inside it) crosses the row edge;
    # tube 2: spans every tile
    boxes = np.array([[[tw - 1, tr - 2, tw + 300, sh + 3], [tw - 400, 3, tw + 1, sh - 1], [40.4, 1.2, sw - 40.6, sh - 1.4]]], dtype=np.float32)
    rng = np.random.default_rng(sw)
    from tubedetr_amd.render import label_tags

    spec = dict(fmt=fmt, planes=make_planes(rng, 1, sh, sw, fmt), boxes=boxes, tags=label_tags(["TILE 0", "EDGE-1", "2"]).numpy(), heat=rng.integers(0, 256, (1, 2, 3), dtype=np.uint8),
                thickness=3, heat_alpha=100, tag_scale=2, tag_alpha=180, lane_h=2, bar_alpha=128, seg_alpha=256, **COLORS)
    run([spec], ("inplace", "shifted"))
    run([dict(spec, heat=None)], ("apart",))  # without the heat layer most runs are copied untouched


@pytest.mark.parametrize("fmt", FMTS)
def test_rows_at_multiples_of_16_bytes(fmt):
    """Pitches that are multiples of 16 (64 columns) and of 8 (80: chroma rows of 40 bytes) without row padding: whole 16-byte runs, and
    the U and V rows of yuv420p walked together."""
    for sh, sw in ((36, 64), (36, 80)):
        spec = full_spec(np.random.default_rng(sw), fmt, sh, sw, 3)
        run([spec], MODES, pad=0)
        run([dict(spec, heat=None, span=None)], ("apart",), pad=0)


@pytest.mark.parametrize("fmt", FMTS)
def test_boxes_across_every_edge_outside_degenerate_and_non_finite_with_tags(fmt):
    sh, sw = 37, 53
    e = edge_boxes(sh, sw)
    boxes = np.concatenate([e, e[:1]]).reshape(4, 4, 4)  # 16 boxes: 4 tube rows of K = 4
    planes = make_planes(np.random.default_rng(7), 4, sh, sw, fmt)
    spec = dict(fmt=fmt, planes=planes, boxes=boxes, tags=labels(4), tag_scale=2, tag_alpha=190, **COLORS)
    out = run([dict(spec, thickness=th) for th in (1, 3, 10000)], ("apart",))
    run([dict(spec, thickness=3)], ("inplace",))
    # tube row 2 = boxes 8..11 (x1 <= x0, y1 < y0, NaN, inf): nothing at all is drawn, neither box nor tag
    src = as_rows(planes, fmt)
    for rows in out:
        assert all(np.array_equal(r[2], s[2]) for r, s in zip(rows, src))


@pytest.mark.parametrize("fmt", FMTS)
def test_overlapping_tags_and_boxes(fmt):
    sh, sw = 37, 53
    rng = np.random.default_rng(14)
    boxes = np.array([[[10, 20, 40, 35], [12, 22, 45, 30], [14, 12, 30, 36]], [[3, 3, 20, 20], [3, 3, 20, 20], [5, 5, 50, 9]]], dtype=np.float32)
    spec = dict(fmt=fmt, planes=make_planes(rng, 2, sh, sw, fmt), boxes=boxes, tags=labels(3), tag_scale=1, tag_alpha=128, thickness=2, **COLORS)
    run([spec, dict(spec, tag_scale=3, tag_alpha=256), dict(spec, tag_alpha=0)], ("apart", "inplace"))


@pytest.mark.parametrize("fmt", FMTS)
def test_spans_that_drop_some_tubes_all_tubes_and_none(fmt):
    sh, sw, T, K = 37, 53, 4, 3
    rng = np.random.default_rng(8)
    planes, boxes = make_planes(rng, T, sh, sw, fmt), tubes(rng, T, K, sh, sw)
    specs = [dict(fmt=fmt, planes=planes, boxes=boxes, span=span, dim_alpha=da, lane_h=2, bar_alpha=99, seg_alpha=201, **COLORS)
             for span in (None, [(0, 1), (1, 2), (2, 2)], [(1, 1), (-1, -1), (5, 2)], [(-(2 ** 62), 2 ** 62), (3, 2 ** 40), (0, 0)]) for da in (0, 96)]
    out = run(specs, ("apart",))
    assert all(np.array_equal(a, b) for a, b in zip(out[0], out[1]))  # no span: dim_alpha plays no part
    assert not np.array_equal(out[2][0][3], out[3][0][3])  # frame 3 lies outside (0, 1), (1, 2), (2, 2): dimmed
    run(specs[5:6], ("inplace",))


@pytest.mark.parametrize("fmt", FMTS)
def test_frame_map_with_rows_out_of_range_and_timelines_with_fewer_and_more_tube_rows_than_columns(fmt):
    sh, sw, K = 37, 53, 2
    rng = np.random.default_rng(9)
    planes = make_planes(rng, 4, sh, sw, fmt)
    few = dict(fmt=fmt, planes=planes, boxes=tubes(rng, 3, K, sh, sw), span=[(0, 1), (2, 2)], frame_map=[0, 2, 3, -1], heat=rng.integers(0, 256, (3, 2, 3), dtype=np.uint8),
               heat_alpha=128, dim_alpha=96, lane_h=4, bar_alpha=140, seg_alpha=256, **COLORS)
    many = dict(few, boxes=tubes(rng, 300, K, sh, sw), heat=None, span=[(17, 130), (131, 299)], frame_map=[0, 150, 299, 300])
    one = dict(fmt=fmt, planes=planes, n_tube=1, K=8, lane_h=4, bar_alpha=256, seg_alpha=77, **COLORS)  # no boxes, no span: a timeline of 8 full lanes, cursor = every column
    out = run([few, many, one], ("apart", "inplace"))
    src = as_rows(planes, fmt)
    assert all(np.array_equal(r[2], s[2]) and np.array_equal(r[3], s[3]) for r, s in zip(out[0], src)), "rows 3 of 3 and -1: plain copies, no timeline"
    assert all(np.array_equal(r[3], s[3]) for r, s in zip(out[1], src)) and all(np.array_equal(r[1:], s[1:]) for r, s in zip(out[2], src))


def test_one_launch_jobs_of_mixed_formats_and_K_with_an_empty_job():
    rng = np.random.default_rng(11)
    specs = []
    for fmt, (sh, sw), K, T in zip(FMTS + ["yuv420p"], [(37, 53), (130, 258), (5, 7), (37, 53)], (3, 8, 1, 2), (3, 2, 3, 0)):
        specs.append(full_spec(rng, fmt, sh, sw, K, T=max(T, 2)))
        if T == 0:
            specs[-1]["T_job"] = 0
    together = run(specs, ("apart",))
    for s, rows in zip(specs[:3], together):
        (alone,) = run([s], ("inplace",))
        assert all(np.array_equal(a, b) for a, b in zip(rows, alone))


def _launch_pair(fmt, sh, sw, T, seed):
    """Two packed device copies of the same random frames."""
    from tubedetr_amd.render import _frame_bytes

    g = torch.Generator().manual_seed(seed)
    data = torch.randint(0, 256, (T * _frame_bytes(fmt, sh, sw),), dtype=torch.uint8, generator=g)
    return data, data.to(DEV), data.to(DEV)


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("size", [(37, 53), (130, 258)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_identity_one_tube_equals_td_tube_overlay_on_the_device(size, fmt):
    from tubedetr_amd.render import overlay_job, overlay_multi_job, tube_overlay, tube_overlay_multi

    sh, sw = size
    T, n_tube = 4, 3
    rng = np.random.default_rng(sw)
    dev = torch.device(DEV)
    src, a, b = _launch_pair(fmt, sh, sw, T, 5)
    t = device_inputs(dict(boxes=tubes(rng, n_tube, 1, sh, sw), span=[(1, 1)], frame_map=[0, 1, 2, 3], heat=rng.integers(0, 256, (n_tube, 7, 11), dtype=np.uint8)), dev)
    common = dict(pix_fmt=fmt, boxes=t["boxes"].data_ptr(), n_tube=n_tube, span=t["span"].data_ptr(), frame_map=t["frame_map"].data_ptr(), heat=t["heat"].data_ptr(),
                  heat_hw=(7, 11), heat_color=(40, 60, 220), dim_color=(16, 128, 128), thickness=3, heat_alpha=160, dim_alpha=96)
    one = tube_overlay([overlay_job(a.data_ptr(), T, sh, sw, box_color=(200, 90, 30), **common)], dev)
    multi = tube_overlay_multi([overlay_multi_job(b.data_ptr(), T, sh, sw, K=1, tube_colors=((200, 90, 30),) + ((1, 2, 3),) * 7, **common)], dev)
    torch.cuda.synchronize()
    del one, multi
    assert torch.equal(a, b) and not torch.equal(a.cpu(), src)


@pytest.mark.parametrize("fmt", FMTS)
def test_identity_three_tubes_equal_three_in_place_td_tube_overlay_launches(fmt):
    from tubedetr_amd.render import overlay_job, overlay_multi_job, tube_overlay, tube_overlay_multi

    sh, sw, T, K = 130, 258, 4, 3
    rng = np.random.default_rng(21)
    dev = torch.device(DEV)
    src, a, b = _launch_pair(fmt, sh, sw, T, 6)
    boxes, span = tubes(rng, T, K, sh, sw), [(0, 2), (1, 3), (3, 3)]
    t = device_inputs(dict(boxes=boxes, span=span), dev)
    per_tube = [device_inputs(dict(boxes=boxes[:, k], span=span[k]), dev) for k in range(K)]
    keep = []
    for k in range(K):  # k ascending, each in place on the result of the one before
        keep.append(tube_overlay([overlay_job(a.data_ptr(), T, sh, sw, pix_fmt=fmt, boxes=per_tube[k]["boxes"].data_ptr(), n_tube=T, span=per_tube[k]["span"].data_ptr(),
                                              box_color=TUBE_COLORS[k], thickness=4, dim_alpha=0)], dev))
    keep.append(tube_overlay_multi([overlay_multi_job(b.data_ptr(), T, sh, sw, pix_fmt=fmt, boxes=t["boxes"].data_ptr(), n_tube=T, K=K, span=t["span"].data_ptr(),
                                                      tube_colors=TUBE_COLORS, thickness=4)], dev))
    torch.cuda.synchronize()
    assert torch.equal(a, b) and not torch.equal(a.cpu(), src)


def _packed_clip(fmt, T, sh, sw, seed):
    from tubedetr_amd.augment import DecodedClip
    from tubedetr_amd.render import DeviceFrames

    planes = make_planes(np.random.default_rng(seed), T, sh, sw, fmt)
    packed = planes.reshape(-1) if fmt == "rgb24" else np.concatenate([np.concatenate([p[t].ravel() for p in planes]) for t in range(T)])
    return planes, DeviceFrames.from_decoded(DecodedClip(packed.copy(), T, sh, sw, fmt, matrix="bt709"), torch.device(DEV))


def _pack(planes, fmt):
    if fmt == "rgb24":
        return torch.from_numpy(planes.reshape(-1))
    return torch.from_numpy(np.concatenate([np.concatenate([p[t].ravel() for p in planes]) for t in range(planes[0].shape[0])]))


def _style_kwargs(style, fmt):
    from tubedetr_amd.render import color_in_space

    space = (fmt, "bt709", False)
    kw = {k: color_in_space(getattr(style, k), *space) for k in ("heat_color", "dim_color", "tag_text_color", "bar_color", "cursor_color")}
    kw.update({k: getattr(style, k) for k in ("thickness", "heat_alpha", "dim_alpha", "tag_scale", "tag_alpha", "lane_h", "bar_alpha", "seg_alpha")})
    kw["tube_color"] = tuple(color_in_space(c, *space) for c in style.colors)
    return kw


@pytest.mark.parametrize("fmt", ["yuv420p", "rgb24"])
def test_end_to_end_densify_two_tubes_into_annotate_tubes_with_string_tags(fmt):
    from tubedetr_amd.render import TubeSetStyle, annotate_tubes, densify, label_tags

    dev = torch.device(DEV)
    T, sh, sw, rows = 4, 45, 79, [0, 3]
    planes, frames = _packed_clip(fmt, T, sh, sw, 31)
    tube = np.array([[[5.2, 20.1, 30.3, 40.4], [40.0, 12.0, 70.5, 30.5]], [[15.2, 14.1, 44.3, 33.4], [30.0, 22.0, 60.5, 44.5]]], dtype=np.float32)
    style = TubeSetStyle(thickness=2, tag_scale=1, tag_alpha=200, lane_h=3, bar_alpha=160, seg_alpha=256, dim_alpha=90)
    d_tube, d_span, d_tags = torch.from_numpy(tube).to(dev), torch.tensor([[0, 1], [0, 0]], device=dev), label_tags(["CAT 1", "dog-2"], dev)
    torch.cuda.synchronize()
    mode = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")  # neither stage may synchronise, labels given as strings included
    try:
        dense = densify(d_tube, T, row_frame=rows, span=d_span, mode="lerp")
        drawn = annotate_tubes(frames, dense.boxes, span=dense.span, tags=["cat 1", "DOG-2"], style=style)
        again = annotate_tubes([frames], [dense.boxes], span=[dense.span], tags=[d_tags], style=style, out=[frames])[0]
    finally:
        torch.cuda.set_sync_debug_mode(mode)
    torch.cuda.synchronize()
    assert again is frames and drawn is not frames and (drawn.T, drawn.h, drawn.w, drawn.pix_fmt, drawn.matrix) == (T, sh, sw, fmt, "bt709")
    assert dense.boxes.shape == (T, 2, 4) and dense.span.shape == (2, 2)
    want = overlay_multi_ref(planes, fmt, boxes=dense.boxes.cpu().numpy(), span=dense.span.cpu().tolist(), tags=label_tags(["CAT 1", "DOG-2"]).numpy(), **_style_kwargs(style, fmt))
    assert torch.equal(drawn.data.cpu(), _pack(want, fmt)) and torch.equal(frames.data.cpu(), _pack(want, fmt))
    assert not torch.equal(_pack(want, fmt), _pack(planes, fmt))


def test_end_to_end_moments_topk_pairs_as_spans_with_a_timeline():
    from tubedetr_amd.models.postprocessors import moments_topk
    from tubedetr_amd.render import TubeSetStyle, annotate_tubes

    dev = torch.device(DEV)
    fmt, T, sh, sw, k = "yuv420p", 4, 45, 79, 3
    planes, frames = _packed_clip(fmt, T, sh, sw, 32)
    n_tube = 12
    steds = torch.randn(1, n_tube, 2, generator=torch.Generator().manual_seed(3)).to(dev)
    moments = moments_topk(steds, k=k)
    boxes = torch.from_numpy(tubes(np.random.default_rng(4), n_tube, 1, sh, sw)[:, 0]).to(dev)  # ONE tube, k candidate moments
    fmap = torch.tensor([0, 4, 8, 11], dtype=torch.int32, device=dev)
    style = TubeSetStyle(lane_h=2, bar_alpha=200, seg_alpha=256, thickness=1)
    drawn = annotate_tubes(frames, boxes, span=moments.pairs[0], frame_map=fmap, style=style)
    torch.cuda.synchronize()
    pairs = moments.pairs[0].cpu().tolist()
    assert len(pairs) == k and pairs[0] != [-1, -1]
    want = overlay_multi_ref(planes, fmt, boxes=np.repeat(boxes.cpu().numpy()[:, None, :], k, 1), span=pairs, frame_map=fmap.cpu().tolist(), **_style_kwargs(style, fmt))
    assert torch.equal(drawn.data.cpu(), _pack(want, fmt)) and not torch.equal(drawn.data.cpu(), frames.data.cpu())
    # a row of (-1, -1) never draws: with every pair absent the frames are only dimmed (here: alpha 0) and carry the bar and the cursor
    none = annotate_tubes(frames, boxes, span=torch.full((k, 2), -1, dtype=torch.int64, device=dev), frame_map=fmap, style=style)
    torch.cuda.synchronize()
    want = overlay_multi_ref(planes, fmt, boxes=np.repeat(boxes.cpu().numpy()[:, None, :], k, 1), span=[(-1, -1)] * k, frame_map=fmap.cpu().tolist(), **_style_kwargs(style, fmt))
    assert torch.equal(none.data.cpu(), _pack(want, fmt))


def test_annotate_tubes_refuses_before_it_allocates():
    from tubedetr_amd.render import TubeSetStyle, annotate_tubes

    dev = torch.device(DEV)
    _, frames = _packed_clip("rgb24", 2, 12, 16, 33)
    boxes = torch.zeros(2, 3, 4, device=dev)
    cases = (dict(boxes=boxes.double()), dict(boxes=boxes.cpu()), dict(boxes=torch.zeros(2, 9, 4, device=dev)), dict(boxes=boxes, span=torch.zeros(2, 2, dtype=torch.int64, device=dev)),
               dict(boxes=boxes, tags=["A", "B"]), dict(boxes=boxes, tags=["A", "B", "c_d"]), dict(boxes=None, tags=["A"]), dict(boxes=boxes, tags=torch.zeros(3, 40, 5, dtype=torch.uint8, device=dev)),
               dict(boxes=boxes, style=TubeSetStyle(lane_h=5)), dict(boxes=None, style=TubeSetStyle(lane_h=1)), dict(boxes=boxes, frame_map=torch.zeros(3, dtype=torch.int32, device=dev)),
               dict(boxes=boxes, heat=torch.zeros(3, 2, 2, dtype=torch.uint8, device=dev)), dict(boxes=boxes, out=object()))
    before = torch.cuda.memory_stats(dev)["allocation.all.allocated"]  # a count of allocations: it only grows
    for kw in cases:
        kw = dict(kw)
        b = kw.pop("boxes")
        with pytest.raises(ValueError):
            annotate_tubes(frames, b, **kw)
    assert torch.cuda.memory_stats(dev)["allocation.all.allocated"] == before, "a refused call allocated device memory"
