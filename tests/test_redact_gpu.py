"""td_tube_redact and tubedetr_amd.render.redact on the GPU.  Every comparison is bit equality (torch.equal) with the numpy
restatement of the header's rule (tests/redact_ref.py).

The canary layout is tests/test_overlay_gpu.py's: a job's planes lie in ONE buffer of random bytes, 64 of them in front of every
plane of every frame, rows at a pitch of their length + 3 (+ 0 where a test says so); the whole buffer is compared, so a byte
written into the padding, in front of a plane or behind it shows, and a separate source is compared too.  Sizes are rows x columns."""
import numpy as np
import pytest
import torch

from redact_ref import redact_ref
from test_overlay_gpu import DST_GAP, as_rows, edge_boxes, layout, make_planes, place, tube

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
FMTS = ["rgb24", "yuv420p", "nv12"]
SIZES = [(5, 7), (37, 53), (130, 258)]  # smaller than a cell or a radius; odd, partial cells and chroma blocks at the far edges; more than one tile both ways, 258 = 2 mod 4
COLOR = (200, 90, 30)
# cell 256 and radius 64 exceed the small frames: the frame is one cell, the window is the plane
MODES = [dict(mode="fill", color=COLOR)] + [dict(mode="mosaic", cell=c) for c in (2, 6, 16, 256)] + [dict(mode="blur", radius=r) for r in (1, 3, 64)]
THREE = [dict(mode="fill", color=COLOR), dict(mode="mosaic", cell=6), dict(mode="blur", radius=3)]


def rows_of(planes, fmt):
    """``as_rows`` that also takes a clip of no frames: every plane as (T, rows, row bytes)."""
    planes = (planes,) if fmt == "rgb24" else planes
    return [p.reshape(p.shape[0], p.shape[1], int(np.prod(p.shape[2:]))) for p in planes]


def run(specs, dest, pad=3):
    """ONE launch.  spec: fmt, planes, and redact_ref's keyword arguments (numpy / tuples).  dest "inplace": the destination
    planes ARE the source planes; "apart": another buffer of the same layout; "shifted": another buffer whose planes start one
    byte later (source and destination rows differ in alignment); "dword": 4 bytes later (they agree modulo 4, not modulo 16).
    ``pad``: row pitch - row length.  Asserts bit equality of every destination buffer with the reference placed into that
    buffer's canaries, and that a separate source is untouched.  The reference of a spec is computed once and kept in it."""
    from tubedetr_amd.render import redact_job, tube_redact

    dev = torch.device(DEV)
    rng = np.random.default_rng(99)
    jobs, keep, checks = [], [], []
    for s in specs:
        if "_want" not in s:
            s["_want"] = redact_ref(s["planes"], s["fmt"], **{k: v for k, v in s.items() if k not in ("fmt", "planes")})
        fmt, planes = s["fmt"], s["planes"]
        rows = rows_of(planes, fmt)
        T, sh, sw = rows[0].shape[0], rows[0].shape[1], (rows[0].shape[2] // 3 if fmt == "rgb24" else rows[0].shape[2])
        slay = layout(rows, 64, pad)
        src = place(rng.integers(0, 256, slay["total"], dtype=np.uint8), rows, slay)
        d_src = torch.from_numpy(src).to(dev)
        want_rows = rows_of(s["_want"], fmt)
        if dest == "inplace":
            dlay, d_dst, want = slay, d_src, place(src.copy(), want_rows, slay)
        else:
            dlay = layout(rows, DST_GAP[dest], pad)
            dst = rng.integers(0, 256, dlay["total"], dtype=np.uint8)
            d_dst, want = torch.from_numpy(dst).to(dev), place(dst.copy(), want_rows, dlay)
        boxes = np.asarray(s["boxes"], dtype=np.float32)
        t = {"boxes": torch.from_numpy(boxes).to(dev), "span": None, "frame_map": None}
        if s.get("span") is not None:
            t["span"] = torch.tensor(np.asarray(s["span"]), dtype=torch.int64, device=dev)
        if s.get("frame_map") is not None:
            t["frame_map"] = torch.tensor(s["frame_map"], dtype=torch.int32, device=dev)
        what = {k: s[k] for k in ("mode", "cell", "radius", "color", "margin", "invert") if k in s}
        jobs.append(redact_job(0, T, sh, sw, pix_fmt=fmt, n_tube=boxes.shape[0], K=1 if boxes.ndim == 2 else boxes.shape[1],
                               src_planes=[d_src.data_ptr() + o for o in slay["offs"]], src_pitches=slay["pitches"], src_frame_stride=slay["stride"],
                               dst_planes=[d_dst.data_ptr() + o for o in dlay["offs"]], dst_pitches=dlay["pitches"], dst_frame_stride=dlay["stride"],
                               **{k: (v.data_ptr() if v is not None else None) for k, v in t.items()}, **what))
        keep.append(t)
        checks.append((d_dst, want, None if dest == "inplace" else (d_src, src)))
    tables = tube_redact(jobs, dev)
    torch.cuda.synchronize()
    del tables
    for i, (d_dst, want, source) in enumerate(checks):
        got = d_dst.cpu()
        assert torch.equal(got, torch.from_numpy(want)), f"job {i} ({specs[i].get('mode')}, {dest}): {(got.numpy() != want).sum()} of {want.size} bytes differ from the reference"
        if source is not None:
            assert torch.equal(source[0].cpu(), torch.from_numpy(source[1])), f"job {i} ({dest}): the source was written"


def in_place_ok(specs):
    return [s for s in specs if s["mode"] != "blur"]


def changed(spec):
    return any(not np.array_equal(a, b) for a, b in zip(as_rows(spec["_want"], spec["fmt"]), as_rows(spec["planes"], spec["fmt"])))


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_every_mode_in_place_apart_and_at_two_misalignments(size, fmt):
    sh, sw = size
    rng = np.random.default_rng(sh)
    T = 3
    planes, boxes = make_planes(rng, T, sh, sw, fmt), tube(rng, T, sh, sw)
    specs = [dict(fmt=fmt, planes=planes, boxes=boxes, **m) for m in MODES]
    run(specs, "apart")
    run(in_place_ok(specs), "inplace")
    run(specs, "shifted")
    run(specs, "dword")
    assert all(changed(s) for s in specs)


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("size", [(36, 64), (36, 80)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_rows_at_multiples_of_16_bytes(size, fmt):
    """Pitch = row length: rows are whole 16-byte runs (64) or start at multiples of 8 (80: chroma rows of 40 bytes), the layout of
    real decoder output."""
    sh, sw = size
    rng = np.random.default_rng(sw)
    T = 3
    planes, boxes = make_planes(rng, T, sh, sw, fmt), tube(rng, T, sh, sw)
    specs = [dict(fmt=fmt, planes=planes, boxes=boxes, **m) for m in MODES]
    for dest in ("apart", "dword", "shifted"):
        run(specs, dest, pad=0)
    run(in_place_ok(specs), "inplace", pad=0)


def all_boxes(sh, sw):
    extra = np.array([[sw * 0.4, sh * 0.4, sw * 0.4 + 1, sh * 0.4 + 1],      # one pixel
                      [1.5, 0.5, sw - 1.5, sh - 2.5],                        # every coordinate at x.5
                      [2.5, 1.5, 3.5, 2.5]], dtype=np.float32)
    return np.concatenate([edge_boxes(sh, sw), extra])


@pytest.mark.parametrize("invert", [False, True], ids=["plain", "inverted"])
@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_boxes_inside_across_every_edge_outside_one_pixel_degenerate_non_finite_and_at_half(size, fmt, invert):
    sh, sw = size
    boxes = all_boxes(sh, sw)  # one box per frame
    planes = make_planes(np.random.default_rng(7), len(boxes), sh, sw, fmt)
    specs = [dict(fmt=fmt, planes=planes, boxes=boxes, margin=margin, invert=invert, **m) for m in THREE for margin in ((0, 1), (1, 4))]
    run(specs, "apart")
    run(in_place_ok(specs), "inplace")
    src = as_rows(planes, fmt)
    for k in (6, 7, 8, 9, 10, 11, 12):  # wholly outside, degenerate, NaN, +-inf: absent - a copy, or with invert the whole frame
        for s in specs:
            if s["margin"] == (0, 1) and s["mode"] == "fill":
                got = as_rows(s["_want"], fmt)
                assert all((not np.array_equal(g[k], p[k])) if invert else np.array_equal(g[k], p[k]) for g, p in zip(got, src)), k


@pytest.mark.parametrize("invert", [False, True], ids=["plain", "inverted"])
@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("size", SIZES[1:], ids=lambda s: f"{s[0]}x{s[1]}")
def test_three_rectangles_with_spans_and_a_frame_map(size, fmt, invert):
    """K = 3: rectangles 0 and 1 overlap, rectangle 2 is absent in tube row 1 (NaN) and small elsewhere; every rectangle has its own
    span, with tube rows inside and outside it; the frame map repeats rows and has -1 and n_tube."""
    sh, sw = size
    n_tube = 4
    boxes = np.empty((n_tube, 3, 4), dtype=np.float32)
    for r in range(n_tube):
        boxes[r, 0] = [sw * 0.1 + r, sh * 0.15, sw * 0.55 + r, sh * 0.6]
        boxes[r, 1] = [sw * 0.4, sh * 0.4 + r, sw * 0.9, sh * 0.85 + r]
        boxes[r, 2] = [sw * 0.8, 1.0, sw * 0.8 + 3.0, 4.0]
    boxes[1, 2, 0] = np.nan
    span = np.array([[0, 2], [1, 3], [1, 1]])
    fmap = [0, 0, 1, 1, -1, 2, 3, n_tube, 3, 2]
    planes = make_planes(np.random.default_rng(8), len(fmap), sh, sw, fmt)
    specs = [dict(fmt=fmt, planes=planes, boxes=boxes, span=span, frame_map=fmap, invert=invert, **m) for m in THREE]
    specs.append(dict(fmt=fmt, planes=planes, boxes=boxes, span=None, frame_map=fmap, invert=invert, margin=(1, 4), mode="mosaic", cell=16))
    specs.append(dict(fmt=fmt, planes=planes[:n_tube] if fmt == "rgb24" else tuple(p[:n_tube] for p in planes), boxes=boxes, span=span, invert=invert, mode="blur", radius=64))
    run(specs, "apart")
    run(in_place_ok(specs), "inplace")
    assert all(changed(s) for s in specs)


@pytest.mark.parametrize("fmt", FMTS)
def test_rows_wider_than_one_column_tile_of_every_mode(fmt):
    """Not in the issue's list: a FILL workgroup takes at most 1024 samples of a row (csrc/redact.hip), so 1100 columns are split
    into two tiles for rgb24 and luma; MOSAIC and BLUR tiles are at most 256 wide, so these rows have five and more."""
    sh, sw = 19, 1100
    rng = np.random.default_rng(sw)
    boxes = np.array([[sw * 0.25 - 3, 0.6, sw * 0.97, sh - 0.6]], dtype=np.float32)  # crosses every tile boundary
    planes = make_planes(rng, 1, sh, sw, fmt)
    specs = [dict(fmt=fmt, planes=planes, boxes=boxes, **m) for m in THREE + [dict(mode="blur", radius=64), dict(mode="mosaic", cell=256)]]
    run(specs, "shifted")
    run(in_place_ok(specs), "inplace")


def test_one_launch_several_jobs_mixing_formats_modes_and_sizes_with_an_empty_job():
    rng = np.random.default_rng(11)
    specs = []
    for fmt, (sh, sw), T, m in zip(FMTS + ["yuv420p", "rgb24"], [(37, 53), (130, 258), (5, 7), (37, 53), (130, 258)], (5, 2, 3, 0, 2),
                                   [dict(mode="mosaic", cell=6), dict(mode="blur", radius=3), dict(mode="fill", color=COLOR), dict(mode="blur", radius=1),
                                    dict(mode="mosaic", cell=16, invert=True)]):
        specs.append(dict(fmt=fmt, planes=make_planes(rng, T, sh, sw, fmt), boxes=tube(rng, max(T, 1), sh, sw), span=(0, 1), **m))
    run(specs, "apart")
    run(in_place_ok(specs), "inplace")
    for s in specs:  # alone it gives what it gave in company
        run([s], "shifted")


def test_end_to_end_redact_two_clips_without_a_synchronisation():
    """``redact`` on a list of two clips (yuv420p bt709 and rgb24), one tube and the union of two, under sync debug mode "error";
    then in place, and the inverse; all against the reference fed the same boxes and the converted colour."""
    from tubedetr_amd.augment import DecodedClip
    from tubedetr_amd.render import DeviceFrames, color_in_space, redact

    dev = torch.device(DEV)
    rng = np.random.default_rng(13)
    T, sh, sw = 6, 45, 79
    Y, U, V = make_planes(rng, T, sh, sw, "yuv420p")
    rgb = make_planes(rng, T, sh, sw, "rgb24")
    packed = np.concatenate([np.concatenate([Y[t].ravel(), U[t].ravel(), V[t].ravel()]) for t in range(T)])
    clips = [DeviceFrames.from_decoded(DecodedClip(packed, T, sh, sw, "yuv420p", matrix="bt709"), dev), DeviceFrames.from_decoded(DecodedClip(rgb.reshape(-1), T, sh, sw, "rgb24"), dev)]
    one = tube(rng, 3, sh, sw)
    two = np.stack([tube(rng, 3, sh, sw), tube(rng, 3, sh, sw)], 1)
    fmap = [0, 0, 1, 1, 2, 2]
    boxes = [torch.from_numpy(one).to(dev), torch.from_numpy(two).to(dev)]
    spans = [torch.tensor([1, 2], device=dev), torch.tensor([[0, 1], [2, 2]], device=dev)]
    fmaps = [torch.tensor(fmap, dtype=torch.int32, device=dev)] * 2
    torch.cuda.synchronize()
    mode = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")  # redact must not synchronise
    try:
        mosaic = redact(clips, boxes, span=spans, frame_map=fmaps, cell=6, margin=(1, 4))
        blurred = redact(clips[0], boxes[0], span=spans[0], frame_map=fmaps[0], mode="blur", radius=5, invert=True)
        work = [DeviceFrames(c.data.clone(), c.T, c.h, c.w, c.pix_fmt, c.matrix, c.full_range) for c in clips]
        filled = redact(work, boxes, span=spans, frame_map=fmaps, mode="fill", color=(250, 30, 60), out=work)
    finally:
        torch.cuda.set_sync_debug_mode(mode)
    torch.cuda.synchronize()
    assert filled[0] is work[0] and filled[1] is work[1] and mosaic[0] is not clips[0]
    assert (blurred.T, blurred.h, blurred.w, blurred.pix_fmt, blurred.matrix) == (T, sh, sw, "yuv420p", "bt709")

    def pack(planes, fmt):
        if fmt == "rgb24":
            return torch.from_numpy(planes.reshape(-1))
        return torch.from_numpy(np.concatenate([np.concatenate([p[t].ravel() for p in planes]) for t in range(T)]))

    kw = [dict(boxes=one, span=(1, 2), frame_map=fmap), dict(boxes=two, span=[[0, 1], [2, 2]], frame_map=fmap)]
    for i, (fmt, planes) in enumerate((("yuv420p", (Y, U, V)), ("rgb24", rgb))):
        assert torch.equal(mosaic[i].data.cpu(), pack(redact_ref(planes, fmt, mode="mosaic", cell=6, margin=(1, 4), **kw[i]), fmt))
        colour = color_in_space((250, 30, 60), fmt, "bt709" if i == 0 else "bt601", False)
        assert torch.equal(filled[i].data.cpu(), pack(redact_ref(planes, fmt, mode="fill", color=colour, **kw[i]), fmt))
        assert torch.equal(clips[i].data.cpu(), pack(planes, fmt)), "the source clip was written"
    assert torch.equal(blurred.data.cpu(), pack(redact_ref((Y, U, V), "yuv420p", mode="blur", radius=5, invert=True, **kw[0]), "yuv420p"))
    assert not torch.equal(mosaic[0].data.cpu(), pack((Y, U, V), "yuv420p"))
