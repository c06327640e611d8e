"""td_tube_overlay and tubedetr_amd.render on the GPU.  Every comparison is bit equality (torch.equal) with the numpy
restatement of the header's rule (tests/overlay_ref.py).

A job's planes lie in ONE buffer full of random canary bytes: 64 of them in front of every plane of every frame (so also
behind it), rows at a pitch of their length + 3 (+ 0 where a test says so).  The whole buffer is compared, so a byte written
into the padding, in front of a plane or behind it shows as a difference.  Sizes are rows x columns."""
import numpy as np
import pytest
import torch

from overlay_ref import overlay_ref

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
FMTS = ["rgb24", "yuv420p", "nv12"]
SIZES = [(5, 7), (37, 53), (130, 258)]  # odd sides; 258 = 2 mod 4; 130 rows = more than one 16-row tile, 3 x 258 bytes = more than one wave
COLORS = {"box_color": (200, 90, 30), "heat_color": (40, 60, 220), "dim_color": (16, 128, 128)}


def make_planes(rng, T, sh, sw, fmt):
    ch, cw = (sh + 1) // 2, (sw + 1) // 2
    if fmt == "rgb24":
        return rng.integers(0, 256, (T, sh, sw, 3), dtype=np.uint8)
    Y = rng.integers(0, 256, (T, sh, sw), dtype=np.uint8)
    if fmt == "yuv420p":
        return (Y, rng.integers(0, 256, (T, ch, cw), dtype=np.uint8), rng.integers(0, 256, (T, ch, cw), dtype=np.uint8))
    return (Y, rng.integers(0, 256, (T, ch, cw, 2), dtype=np.uint8))


def as_rows(planes, fmt):
    """Every plane as (T, rows, row bytes)."""
    planes = (planes,) if fmt == "rgb24" else planes
    return [p.reshape(p.shape[0], p.shape[1], -1) for p in planes]


def layout(rows, gap, pad=3):
    pitches = [r.shape[2] + pad for r in rows]
    offs, o = [], 0
    for r, p in zip(rows, pitches):
        o += gap
        offs.append(o)
        o += p * r.shape[1]
    return {"offs": offs, "pitches": pitches, "stride": o, "total": rows[0].shape[0] * o + gap}


def place(buf, rows, lay):
    for r, p, off in zip(rows, lay["pitches"], lay["offs"]):
        for t in range(r.shape[0]):
            for y in range(r.shape[1]):
                a = t * lay["stride"] + off + y * p
                buf[a : a + r.shape[2]] = r[t, y]
    return buf


DST_GAP = {"apart": 64, "shifted": 65, "dword": 68}


def run(specs, mode, pad=3):
    """ONE launch.  spec: fmt, planes, and overlay_ref's keyword arguments (numpy / tuples).  mode "inplace": the destination
    planes ARE the source planes; "apart": another buffer of the same layout; "shifted": another buffer whose planes start one
    byte later (source and destination rows differ in alignment); "dword": 4 bytes later (they agree modulo 4, not modulo 16).
    ``pad``: row pitch - row length.  Asserts bit equality of every destination buffer with the reference placed into that
    buffer's canaries, and that a separate source is untouched."""
    from tubedetr_amd.render import overlay_job, tube_overlay

    dev = torch.device(DEV)
    rng = np.random.default_rng(99)
    jobs, keep, checks = [], [], []
    for s in specs:
        s = dict(s)
        fmt, planes = s.pop("fmt"), s.pop("planes")
        rows = as_rows(planes, fmt)
        T, sh, sw = rows[0].shape[0], rows[0].shape[1], (rows[0].shape[2] // 3 if fmt == "rgb24" else rows[0].shape[2])
        slay = layout(rows, 64, pad)
        src = place(rng.integers(0, 256, slay["total"], dtype=np.uint8), rows, slay)
        d_src = torch.from_numpy(src).to(dev)
        want_rows = as_rows(overlay_ref(planes, fmt, **s), fmt)
        if mode == "inplace":
            dlay, d_dst, want = slay, d_src, place(src.copy(), want_rows, slay)
        else:
            dlay = layout(rows, DST_GAP[mode], pad)
            dst = rng.integers(0, 256, dlay["total"], dtype=np.uint8)
            d_dst, want = torch.from_numpy(dst).to(dev), place(dst.copy(), want_rows, dlay)
        t = {k: None for k in ("boxes", "span", "frame_map", "heat")}
        if s.get("boxes") is not None:
            t["boxes"] = torch.from_numpy(np.asarray(s["boxes"], dtype=np.float32)).to(dev)
        if s.get("span") is not None:
            t["span"] = torch.tensor(s["span"], dtype=torch.int64, device=dev)
        if s.get("frame_map") is not None:
            t["frame_map"] = torch.tensor(s["frame_map"], dtype=torch.int32, device=dev)
        if s.get("heat") is not None:
            t["heat"] = torch.from_numpy(np.ascontiguousarray(s["heat"])).to(dev)
        n_tube = s.get("n_tube", len(s["boxes"]) if s.get("boxes") is not None else len(s["heat"]) if s.get("heat") is not None else 2 ** 31 - 1)
        style = {k: s[k] for k in ("box_color", "heat_color", "dim_color", "thickness", "heat_alpha", "dim_alpha") if k in s}
        jobs.append(overlay_job(0, T, sh, sw, pix_fmt=fmt, n_tube=n_tube, heat_hw=tuple(s["heat"].shape[1:]) if s.get("heat") is not None else (0, 0),
                                src_planes=[d_src.data_ptr() + o for o in slay["offs"]], src_pitches=slay["pitches"], src_frame_stride=slay["stride"],
                                dst_planes=[d_dst.data_ptr() + o for o in dlay["offs"]], dst_pitches=dlay["pitches"], dst_frame_stride=dlay["stride"],
                                **{k: (v.data_ptr() if v is not None else None) for k, v in t.items()}, **style))
        keep.append(t)
        checks.append((d_dst, want, None if mode == "inplace" else (d_src, src), want_rows))
    tables = tube_overlay(jobs, dev)
    torch.cuda.synchronize()
    del tables
    out = []
    for i, (d_dst, want, source, want_rows) in enumerate(checks):
        got = d_dst.cpu()
        assert torch.equal(got, torch.from_numpy(want)), f"job {i} ({mode}): {(got.numpy() != want).sum()} of {want.size} bytes differ from the reference"
        if source is not None:
            assert torch.equal(source[0].cpu(), torch.from_numpy(source[1])), f"job {i} ({mode}): the source was written"
        out.append(want_rows)
    return out


def tube(rng, n, sh, sw):
    """n boxes that lie inside the frame."""
    x0, y0 = rng.uniform(0, sw * 0.5, n), rng.uniform(0, sh * 0.5, n)
    return np.stack([x0, y0, x0 + rng.uniform(1.5, sw * 0.5, n), y0 + rng.uniform(1.5, sh * 0.5, n)], 1).astype(np.float32)


@pytest.mark.parametrize("T", [1, 5])
@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_all_layers_in_place_and_out_of_place(size, fmt, T):
    sh, sw = size
    rng = np.random.default_rng(sh + T)
    spec = dict(fmt=fmt, planes=make_planes(rng, T, sh, sw, fmt), boxes=tube(rng, T, sh, sw), span=(1, 3) if T > 1 else (0, 0),
                heat=rng.integers(0, 256, (T, 7, 11), dtype=np.uint8), thickness=3, heat_alpha=160, dim_alpha=96, **COLORS)
    a = run([spec], "inplace")
    b = run([spec], "apart")
    c = run([spec], "shifted")
    for x, y, z in zip(a[0], b[0], c[0]):
        assert np.array_equal(x, y) and np.array_equal(x, z)
    assert any(not np.array_equal(x, y) for x, y in zip(a[0], as_rows(spec["planes"], fmt))), "the overlay changed nothing"


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("size", [(3, 2051), (18, 4099)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_rows_wider_than_one_column_tile(size, fmt):
    """Not in the issue's list: a workgroup takes at most 2048 columns (csrc/overlay.hip), so these rows are split into 2 and 3
    tiles whose shared dwords and chroma blocks must have one writer each."""
    sh, sw = size
    rng = np.random.default_rng(sw)
    boxes = np.array([[sw * 0.25 - 3, 0.6, sw * 0.75 + 2, sh - 0.6]], dtype=np.float32)  # crosses every tile boundary
    spec = dict(fmt=fmt, planes=make_planes(rng, 1, sh, sw, fmt), boxes=boxes, heat=rng.integers(0, 256, (1, 2, 3), dtype=np.uint8), thickness=1, heat_alpha=160, **COLORS)
    run([spec], "inplace")
    run([spec], "shifted")


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("size", [(36, 64), (36, 80)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_rows_at_multiples_of_16_bytes(size, fmt):
    """Not in the issue's list: pitches that are multiples of 16 (64) or of 8 (80: chroma rows of 40 bytes) with the planes 64 bytes
    apart, the layout of real decoder output.  Rows are then whole 16-byte runs (csrc/overlay.hip loads and stores them as such,
    or as 4 dwords when source and destination agree only modulo 4), and the U and V rows of yuv420p are walked together."""
    sh, sw = size
    rng = np.random.default_rng(sw)
    T = 3
    spec = dict(fmt=fmt, planes=make_planes(rng, T, sh, sw, fmt), boxes=tube(rng, T, sh, sw), span=(1, 1), heat=rng.integers(0, 256, (T, 7, 11), dtype=np.uint8),
                thickness=2, heat_alpha=160, dim_alpha=96, **COLORS)
    for mode in ("inplace", "apart", "dword", "shifted"):
        run([spec], mode, pad=0)
    run([dict(fmt=fmt, planes=spec["planes"], boxes=spec["boxes"], thickness=2, **COLORS)], "apart", pad=0)  # the box alone: most runs are copied untouched


def edge_boxes(sh, sw):
    inf, nan = np.inf, np.nan
    return np.array([
        [sw * 0.2, sh * 0.2, sw * 0.8, sh * 0.7],          # inside
        [-3.4, sh * 0.3, sw * 0.5, sh * 0.6],              # crosses the left edge
        [sw * 0.3, -2.5, sw * 0.6, sh * 0.5],              # the top edge
        [sw * 0.5, sh * 0.3, sw + 4.2, sh * 0.8],          # the right edge
        [sw * 0.2, sh * 0.5, sw * 0.7, sh + 2.5],          # the bottom edge
        [-2.0, -2.0, sw + 2.0, sh + 2.0],                  # all four: thickness 3 shows one line inside the frame
        [sw + 1.0, 1.0, sw + 9.0, sh - 1.0],               # fully outside
        [-9.0, -9.0, -1.0, -1.0],
        [2.0, 1.0, 2.3, sh - 1.0],                         # x1 <= x0 after rounding
        [1.0, 3.0, sw - 1.0, 2.0],                         # y1 < y0
        [nan, 1.0, 3.0, 3.0],
        [1.0, 1.0, inf, 3.0],
        [-inf, 1.0, 3.0, 3.0],
        [-1e30, -1e30, 1e30, 1e30],                        # finite: clamped to +-2^20, nothing of the outline is in the frame
        [0.0, 0.0, float(sw), float(sh)],                  # the frame itself
    ], dtype=np.float32)


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_boxes_inside_across_every_edge_outside_degenerate_and_non_finite(size, fmt):
    sh, sw = size
    boxes = edge_boxes(sh, sw)
    planes = make_planes(np.random.default_rng(7), len(boxes), sh, sw, fmt)
    # thickness 1, 3, and more than half of any box (filled); one launch
    out = run([dict(fmt=fmt, planes=planes, boxes=boxes, thickness=th, **COLORS) for th in (1, 3, 10000)], "apart")
    run([dict(fmt=fmt, planes=planes, boxes=boxes, thickness=3, **COLORS)], "inplace")
    src = as_rows(planes, fmt)
    for k in (6, 7, 8, 9, 10, 11, 12, 13):  # these draw nothing, at any thickness
        for rows in out:
            assert all(np.array_equal(r[k], s[k]) for r, s in zip(rows, src)), k
    luma = out[2][0][0]  # filled: every byte of the box is the colour
    x0, y0, x1, y1 = (int(np.floor(v + np.float32(0.5))) for v in boxes[0])
    inside = luma[y0:y1, 3 * x0 : 3 * x1].reshape(y1 - y0, x1 - x0, 3) if fmt == "rgb24" else luma[y0:y1, x0:x1]
    assert (inside == (COLORS["box_color"] if fmt == "rgb24" else COLORS["box_color"][0])).all()


@pytest.mark.parametrize("fmt", FMTS)
def test_span_null_middle_range_single_row_with_and_without_dimming(fmt):
    sh, sw, T = 37, 53, 5
    rng = np.random.default_rng(8)
    planes, boxes = make_planes(rng, T, sh, sw, fmt), tube(rng, T, sh, sw)
    specs = [dict(fmt=fmt, planes=planes, boxes=boxes, span=span, dim_alpha=da, **COLORS) for span in (None, (1, 3), (2, 2)) for da in (0, 96)]
    out = run(specs, "apart")
    src = as_rows(planes, fmt)
    assert np.array_equal(out[2][0][0], src[0][0]) and not np.array_equal(out[3][0][0], src[0][0])  # frame 0 outside (1, 3): untouched at alpha 0, dimmed at 96
    assert all(np.array_equal(a, b) for a, b in zip(out[0], out[1]))  # no span: dim_alpha plays no part
    run(specs[3:4], "inplace")


@pytest.mark.parametrize("fmt", FMTS)
def test_frame_map_three_frames_per_tube_row_and_one_entry_out_of_range(fmt):
    sh, sw = 37, 53
    rng = np.random.default_rng(9)
    fmap = [0, 0, 0, 1, 1, 1, 2, 2, 2, 3]
    planes = make_planes(rng, len(fmap), sh, sw, fmt)
    spec = dict(fmt=fmt, planes=planes, boxes=tube(rng, 3, sh, sw), heat=rng.integers(0, 256, (3, 2, 3), dtype=np.uint8), span=(1, 2), frame_map=fmap,
                heat_alpha=128, dim_alpha=96, **COLORS)
    (out,) = run([spec], "apart")
    assert all(np.array_equal(r[9], s[9]) for r, s in zip(out, as_rows(planes, fmt))), "row 3 of 3: a plain copy"
    run([dict(spec, frame_map=[2, -1, 0, 1, 2, 0, 1, 2, 0, 1])], "inplace")


@pytest.mark.parametrize("grid", [(2, 3), (7, 11)], ids=lambda g: f"{g[0]}x{g[1]}")
@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_heat_maps(size, fmt, grid):
    sh, sw = size
    rng = np.random.default_rng(10)
    planes = make_planes(rng, 2, sh, sw, fmt)
    heat = rng.integers(0, 256, (2,) + grid, dtype=np.uint8)
    zero, full, mixed = run([dict(fmt=fmt, planes=planes, heat=heat, heat_alpha=0, **COLORS),
                             dict(fmt=fmt, planes=planes, heat=np.full((2,) + grid, 255, np.uint8), heat_alpha=256, **COLORS),
                             dict(fmt=fmt, planes=planes, heat=heat, heat_alpha=200, **COLORS)], "apart")
    src = as_rows(planes, fmt)
    assert all(np.array_equal(a, b) for a, b in zip(zero, src)), "heat_alpha 0 is the identity"
    hc = COLORS["heat_color"]
    if fmt == "rgb24":
        assert (full[0].reshape(2, sh, sw, 3) == hc).all()
    elif fmt == "yuv420p":
        assert (full[0] == hc[0]).all() and (full[1] == hc[1]).all() and (full[2] == hc[2]).all()
    else:
        assert (full[0] == hc[0]).all() and (full[1].reshape(2, -1, 2) == hc[1:]).all()
    assert not np.array_equal(mixed[0], src[0])
    run([dict(fmt=fmt, planes=planes, heat=heat, heat_alpha=200, **COLORS)], "inplace")


def test_one_launch_three_jobs_three_formats():
    rng = np.random.default_rng(11)
    specs = []
    for fmt, (sh, sw), T in zip(FMTS, [(37, 53), (130, 258), (5, 7)], (5, 2, 3)):
        specs.append(dict(fmt=fmt, planes=make_planes(rng, T, sh, sw, fmt), boxes=tube(rng, T, sh, sw), span=(0, 1), heat=rng.integers(0, 256, (T, 7, 11), dtype=np.uint8),
                          thickness=2, heat_alpha=100, dim_alpha=50, **COLORS))
    together = run(specs, "apart")
    for s, rows in zip(specs, together):
        (alone,) = run([s], "inplace")
        assert all(np.array_equal(a, b) for a, b in zip(rows, alone))


def test_heat_from_attention_against_the_cpu_formula():
    from tubedetr_amd.render import heat_from_attention

    g = torch.Generator().manual_seed(12)
    ca = torch.rand(6, 1, 7 * 11 + 5, generator=g).softmax(-1)
    ca[3, 0, :77] *= 1e-3  # a frame whose attention went to the text
    got = heat_from_attention(ca.to(DEV), (7, 11))
    assert got.dtype == torch.uint8 and got.shape == (6, 7, 11) and got.is_cuda
    vis = ca[:, 0, :77].double()
    want = (vis / vis.amax(1, keepdim=True) * 255).view(6, 7, 11)
    assert (got.cpu().double() - want).abs().max().item() <= 1.0
    assert (got.view(6, -1).amax(1) == 255).all()
    assert heat_from_attention(ca.to(DEV), (7, 11), n_valid=4).shape == (4, 7, 11)


def test_end_to_end_model_postprocess_annotate():
    """T = 6, res 64, k = 2 on the synthetic model: forward under no_grad, PostProcess, sted_decode, heat_from_attention and
    annotate on a yuv420p DecodedClip; the result equals the reference fed the boxes, span and maps read back afterwards."""
    import tubedetr_amd
    from oracle.tubedetr_oracle import OracleConfig
    from oracle.weights import fill_state, state_spec, synthetic_batch
    from tubedetr_amd.augment import DecodedClip
    from tubedetr_amd.harness import FixedTokenizer, batch_to
    from tubedetr_amd.models import build_model
    from tubedetr_amd.models.postprocessors import PostProcess, sted_decode
    from tubedetr_amd.render import DeviceFrames, TubeStyle, annotate, color_in_space, heat_from_attention
    from tubedetr_amd.util.misc import NestedTensor

    dev = torch.device(DEV)
    T, res, k, L = 6, 64, 2, 5
    cfg = OracleConfig(stride=k)
    batch = synthetic_batch(T=T, res=res, k=k, L=L, seed=3)
    model, _, _ = build_model(tubedetr_amd.default_args(stride=k, compute_dtype=torch.float32))
    model.load_state_dict(fill_state(state_spec(cfg), 11), strict=True)
    model.to(dev).eval()
    model.transformer.tokenizer = FixedTokenizer(batch["input_ids"], batch["attention_mask"])
    bt = batch_to(batch, dev)
    with torch.no_grad():
        samples, fast = NestedTensor(bt["frames"], bt["frames_mask"]), NestedTensor(bt["frames_fast"], bt["fast_mask"])
        cache = model(samples, [T], ["synthetic caption"], encode_and_save=True, samples_fast=fast)
        out = model(samples, [T], ["synthetic caption"], encode_and_save=False, memory_cache=cache)
    sh, sw = 45, 79  # the decoded clip's own size: boxes are scaled to it
    boxes = PostProcess()(out, torch.tensor([[sh, sw]] * T, device=dev))
    boxes = torch.stack([b["boxes"] for b in boxes])
    span = sted_decode(out["pred_sted"])[0]
    assert out["ca_weights"].shape == (T, 1, 2 * 2 + L)
    heat = heat_from_attention(out["ca_weights"], (2, 2))
    rng = np.random.default_rng(13)
    Y, U, V = make_planes(rng, T, sh, sw, "yuv420p")
    packed = np.concatenate([np.concatenate([Y[t].ravel(), U[t].ravel(), V[t].ravel()]) for t in range(T)])
    clip = DecodedClip(packed, T, sh, sw, "yuv420p", matrix="bt709")
    frames = DeviceFrames.from_decoded(clip, dev)
    style = TubeStyle(thickness=2, heat_alpha=144, dim_alpha=96, heat_color=(255, 64, 0))
    torch.cuda.synchronize()
    mode = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")  # annotate must not synchronise
    try:
        drawn = annotate(frames, boxes, span=span, heat=heat, style=style)
        again = annotate([frames], [boxes], span=[span], heat=[heat], style=style, out=[frames])[0]
    finally:
        torch.cuda.set_sync_debug_mode(mode)
    torch.cuda.synchronize()
    assert again is frames and drawn is not frames and (drawn.T, drawn.h, drawn.w, drawn.pix_fmt, drawn.matrix) == (T, sh, sw, "yuv420p", "bt709")
    space = ("yuv420p", "bt709", False)
    want = overlay_ref((Y, U, V), "yuv420p", boxes=boxes.cpu().numpy(), span=tuple(span.cpu().tolist()), heat=heat.cpu().numpy(), thickness=2, heat_alpha=144, dim_alpha=96,
                       box_color=color_in_space(style.box_color, *space), heat_color=color_in_space(style.heat_color, *space), dim_color=color_in_space(style.dim_color, *space))
    want = torch.from_numpy(np.concatenate([np.concatenate([p[t].ravel() for p in want]) for t in range(T)]))
    assert torch.equal(drawn.data.cpu(), want) and torch.equal(frames.data.cpu(), want)
    assert not torch.equal(want, torch.from_numpy(packed))
