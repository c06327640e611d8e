"""td_tube_densify and tubedetr_amd.render.densify on the GPU.  Every comparison is exact: fp32 outputs as their bit patterns,
the rest as bytes (torch.equal), against the numpy restatement of the header's rule (tests/tube_dense_ref.py).  The rule is
integer arithmetic and correctly rounded fp32, one rounding per operation, so there is no tolerance.

Canaries: all outputs of a job lie in ONE buffer of random bytes, at least 64 of them in front of each output and behind the
last; the attention maps start 5 bytes past a multiple of 16, so their first and last 16-byte runs are partial.  The whole
buffer is compared, so a byte written in front of an output or behind it shows."""
import numpy as np
import pytest
import torch

from overlay_ref import overlay_ref
from redact_ref import redact_ref
from test_overlay_gpu import make_planes
from tube_dense_ref import QNAN_BITS, dense_floats, densify_ref

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
MODES = ["hold", "lerp", "hull"]
GAP = 64


def tube(n, K, seed=0, scale=1.0):
    rng = np.random.default_rng(seed)
    x0, y0 = rng.uniform(0, 300, (n, K)), rng.uniform(0, 200, (n, K))
    return (np.stack([x0, y0, x0 + rng.uniform(2, 300, (n, K)), y0 + rng.uniform(2, 200, (n, K))], -1) * scale).astype(np.float32)


def gaps(n, first=0, pattern=(1, 5, 7)):
    """n increasing frame numbers whose gaps cycle through ``pattern``."""
    out, f = [], first
    for r in range(n):
        out.append(f)
        f += pattern[r % len(pattern)]
    return out


def spec(boxes, T, **kw):
    return dict(boxes=boxes, T=T, **kw)


def ref_of(s):
    """The reference of a spec, computed once and kept in it."""
    if "_want" not in s:
        s["_want"] = densify_ref(**{k: v for k, v in s.items() if not k.startswith("_")})
    return s["_want"]


def run(specs):
    """ONE launch of all specs (the keyword arguments of densify_ref); asserts every job's buffer, canaries included, against
    the reference.  Returns, per job, what the device wrote: dict(dense=uint32 bits, valid, span, heat)."""
    from tubedetr_amd.render import dense_job, tube_densify

    dev = torch.device(DEV)
    rng = np.random.default_rng(5)
    jobs, keep, checks = [], [], []
    for s in specs:
        want = ref_of(s)
        boxes = np.asarray(s["boxes"], dtype=np.float32)
        boxes = boxes[:, None, :] if boxes.ndim == 2 else boxes
        n_tube, K = boxes.shape[:2]
        T, heat = s["T"], s.get("heat")
        mb = int(np.prod(heat.shape[1:])) if heat is not None else 0
        parts = [("dense", 16 * T * K, 0), ("valid", T * K, 0), ("span", 16 * K, 0)] + ([("heat", T * mb, 5)] if heat is not None else [])
        offs, o = {}, 0
        for name, size, skew in parts:
            o = (o + GAP + 15) // 16 * 16 + skew
            offs[name] = (o, size)
            o += size
        canary = rng.integers(0, 256, o + GAP, dtype=np.uint8)
        expect = canary.copy()
        for name, (a, size) in offs.items():
            expect[a:a + size] = np.ascontiguousarray(want[name]).view(np.uint8).reshape(-1)
        buf = torch.from_numpy(canary).to(dev)
        t = {"boxes": torch.from_numpy(boxes).to(dev)}
        if s.get("span") is not None:
            t["span"] = torch.tensor(np.asarray(s["span"]).reshape(K, 2), dtype=torch.int64, device=dev)
        if s.get("row_frame") is not None:
            t["row_frame"] = torch.tensor(s["row_frame"], dtype=torch.int32, device=dev)
        if heat is not None:
            t["heat"] = torch.from_numpy(np.ascontiguousarray(heat)).to(dev)
        at = lambda name: buf.data_ptr() + offs[name][0]  # noqa: E731
        jobs.append(dense_job(t["boxes"].data_ptr(), n_tube, T, at("dense"), K, span=t["span"].data_ptr() if "span" in t else None,
                              row_frame=t["row_frame"].data_ptr() if "row_frame" in t else None, first=s.get("first", 0), step=s.get("step", 1), t0=s.get("t0", 0),
                              heat=t["heat"].data_ptr() if heat is not None else None, heat_hw=heat.shape[1:] if heat is not None else (0, 0), mode=s.get("mode", "lerp"),
                              smooth=s.get("smooth", 0), valid=at("valid"), dense_span=at("span"), dense_heat=at("heat") if heat is not None else None))
        keep.append(t)
        checks.append((buf, expect, offs, K))
    tables = tube_densify(jobs, dev)
    torch.cuda.synchronize()
    del tables
    out = []
    for i, (buf, expect, offs, K) in enumerate(checks):
        got = buf.cpu().numpy()
        for name, (a, size) in offs.items():
            bad = int((got[a:a + size] != expect[a:a + size]).sum())
            assert bad == 0, f"job {i} ({specs[i].get('mode', 'lerp')}): {bad} of {size} bytes of {name} differ from the reference"
        assert np.array_equal(got, expect), f"job {i}: a byte outside the outputs was written"
        T = specs[i]["T"]
        cut = lambda name: got[offs[name][0]:offs[name][0] + offs[name][1]].copy()  # noqa: E731
        out.append(dict(dense=cut("dense").view(np.uint32).reshape(T, K, 4), valid=cut("valid").reshape(T, K), span=cut("span").view(np.int64).reshape(K, 2),
                        heat=cut("heat") if "heat" in offs else None))
    return out


@pytest.mark.parametrize("mode", MODES)
def test_smallest_shapes_one_and_eight_rectangles_with_and_without_a_table(mode):
    specs = [
        spec(tube(1, 1), 5, first=2, step=3, mode=mode),                                      # one row: no interval, one frame hits it
        spec(tube(2, 1, 1), 1, first=0, step=4, t0=3, mode=mode),                             # T = 1, strictly between two rows
        spec(tube(2, 8, 2), 1, row_frame=[7, 9], t0=9, mode=mode),                            # T = 1 on the last row
        spec(tube(61, 1, 3), 300, first=0, step=5, mode=mode),                                # 300 frames of K = 1: two workgroups
        spec(tube(90, 8, 4), 300, row_frame=gaps(90, -20), t0=10, mode=mode),                 # gaps 1, 5, 7; rows before t0 and beyond t0 + T
        spec(tube(9, 3, 5), 70, row_frame=gaps(9, 12), t0=0, mode=mode, smooth=2),            # frames before the first and after the last row
        spec(tube(4, 2, 6), 40, first=-6, step=13, t0=-9, mode=mode),                         # negative frame numbers
    ]
    got = run(specs)
    assert got[3]["valid"].all() and got[4]["valid"].all()
    assert not got[5]["valid"][:12].any() and got[5]["valid"][12:45].all() and not got[5]["valid"][45:].any()


@pytest.mark.parametrize("mode", MODES)
def test_two_chunks_equal_the_whole(mode):
    kw = dict(boxes=tube(70, 3, 7), row_frame=gaps(70, -3), span=[[0, 69], [10, 40], [33, 68]], mode=mode, smooth=1)
    rng = np.random.default_rng(8)
    kw["heat"] = rng.integers(0, 256, (70, 3, 5), dtype=np.uint8)
    whole, lo, hi = run([spec(T=300, t0=0, **kw), spec(T=150, t0=0, **kw), spec(T=150, t0=150, **kw)])
    for name in ("dense", "valid", "heat"):
        assert np.array_equal(np.concatenate([lo[name], hi[name]]), whole[name]), name
    assert np.array_equal(lo["span"], whole["span"]) and np.array_equal(hi["span"], whole["span"] - 150)


@pytest.mark.parametrize("mode", MODES)
def test_span_null_inside_clipped_by_the_row_range_and_empty(mode):
    boxes = tube(8, 4, 9)
    rf = gaps(8, 2)
    got = run([spec(boxes, 40, row_frame=rf, span=[[2, 5], [-3, 100], [5, 3], [7, 7]], mode=mode),
               spec(boxes, 40, row_frame=rf, mode=mode),
               spec(boxes[:, 0], 40, first=2, step=4, span=[1, 6], t0=-2, mode=mode)])
    assert not got[0]["valid"][:, 2].any() and got[0]["span"][2].tolist() == [0, -1]
    assert np.array_equal(got[0]["dense"][:, 1], got[1]["dense"][:, 1]) and np.array_equal(got[0]["span"][1], got[1]["span"][1])
    assert got[0]["valid"][:, 3].sum() == (1 if mode != "hull" else 1 + rf[7] - rf[6] - 1)


@pytest.mark.parametrize("smooth", [0, 2])
@pytest.mark.parametrize("mode", MODES)
def test_nan_and_infinite_rows_in_mid_span_and_an_overflow(mode, smooth):
    boxes = tube(9, 2, 10)
    boxes[3, 0, 1] = np.nan
    boxes[5, 0, 2] = np.inf
    boxes[4, 1] = [-3e38, -3e38, 3e38, 3e38]   # finite: B - A and the smoothing sums overflow; written as computed, valid = 0
    boxes[5, 1] = [3e38, 3e38, 3.4e38, 3.4e38]
    got = run([spec(boxes, 50, first=1, step=5, mode=mode, smooth=smooth), spec(boxes, 50, row_frame=gaps(9, 1), span=[[1, 7], [0, 8]], mode=mode, smooth=smooth)])
    ref = ref_of(spec(boxes, 50, first=1, step=5, mode=mode, smooth=smooth))
    assert (got[0]["dense"][16, 0] == QNAN_BITS).all() and got[0]["valid"][16, 0] == 0  # the NaN row's own frame
    if mode == "lerp":
        assert not got[0]["valid"][12:21, 0].any() and not got[0]["valid"][22:31, 0].any()  # the two intervals around the NaN row and around the Inf row
        assert not np.isfinite(dense_floats(ref)[23, 1]).all() and got[0]["valid"][23, 1] == 0
    assert got[0]["valid"][:, 0].sum() > 10


@pytest.mark.parametrize("smooth", [0, 2, 16])
@pytest.mark.parametrize("mode", MODES)
def test_smoothing_radii_on_five_rows(mode, smooth):
    boxes = tube(5, 2, 11)
    boxes[1, 1, 0] = np.nan
    run([spec(boxes, 30, first=0, step=6, mode=mode, smooth=smooth, span=[[0, 4], [0, 3]]), spec(boxes[:, 0], 30, row_frame=[0, 1, 6, 13, 14], mode=mode, smooth=smooth)])


@pytest.mark.parametrize("grid", [(3, 5), (16, 16)], ids=["3x5", "16x16"])
@pytest.mark.parametrize("mode", MODES)
def test_attention_maps(mode, grid):
    rng = np.random.default_rng(12)
    heat = rng.integers(0, 256, (12,) + grid, dtype=np.uint8)
    heat[3], heat[4] = 0, 255
    got = run([spec(tube(12, 1, 12), 70, row_frame=gaps(12, 4), heat=heat, mode=mode), spec(tube(12, 2, 13), 37, first=-5, step=4, t0=-9, heat=heat, mode=mode, span=[[3, 2], [0, 11]])])
    assert got[0]["heat"].any() and not got[0]["heat"][: 4 * grid[0] * grid[1]].any()
    assert got[1]["heat"].any()  # the maps ignore the spans


def test_tables_beyond_the_staged_rows_and_tables_that_do_not_increase():
    """Not in the issue's list.  A table of more than 1024 rows is searched in global memory (csrc/tube_dense.hip) instead of
    LDS; equal neighbours and an unsorted table give what the header's search gives, and no index leaves the table."""
    long_rf = gaps(1100, -50)
    specs = [spec(tube(1100, 2, 14), 64, row_frame=long_rf, t0=long_rf[1020] - 3, mode=m, smooth=s, span=[[0, 1099], [1000, 1030]]) for m, s in (("lerp", 0), ("hull", 3))]
    specs += [spec(tube(6, 1, 15), 30, row_frame=[0, 5, 5, 10, 10, 20], mode=m, smooth=1) for m in MODES]
    specs += [spec(tube(7, 2, 16), 40, row_frame=[0, 20, 10, 15, 30, 12, 35], mode=m, smooth=2) for m in MODES]
    run(specs)


def test_one_launch_five_jobs_of_mixed_mode_rectangles_and_length_with_an_empty_one():
    rng = np.random.default_rng(17)
    specs = [spec(tube(20, 1, 18), 300, first=3, step=16, mode="lerp", smooth=1, heat=rng.integers(0, 256, (20, 3, 5), dtype=np.uint8)),
             spec(tube(7, 8, 19), 33, row_frame=gaps(7, 2), mode="hull", span=[[k % 4, 6 - k % 3] for k in range(8)]),
             spec(tube(5, 3, 20), 0, first=10, step=5, t0=4, mode="hull", span=[[1, 3], [0, 4], [3, 1]]),  # T = 0: only dense_span
             spec(tube(3, 2, 21), 1, first=0, step=9, t0=4, mode="hold"),
             spec(tube(40, 5, 22), 130, row_frame=gaps(40, 0, (7, 1, 1, 5)), t0=-4, mode="lerp", heat=rng.integers(0, 256, (40, 16, 16), dtype=np.uint8))]
    together = run(specs)
    assert together[2]["span"].tolist() == [[10 + 1 - 4, 30 - 1 - 4], [10 - 4, 30 - 4], [0, -1]]
    for s, t in zip(specs, together):  # alone it gives what it gave in company; twice the same bits
        alone = run([s])[0]
        assert all(np.array_equal(alone[k], t[k]) for k in ("dense", "valid", "span")) and (t["heat"] is None or np.array_equal(alone["heat"], t["heat"]))


# ---- end to end: densify -> redact / annotate at 32 x 48, T = 24 -----------------------------------------------------------
SH, SW, T_CLIP = 32, 48, 24
ROWS = [0, 5, 10, 15, 20]  # the sampled frames; frames 21 .. 23 lie behind the last row


def _clip(fmt, seed):
    from tubedetr_amd.augment import DecodedClip
    from tubedetr_amd.render import DeviceFrames

    planes = make_planes(np.random.default_rng(seed), T_CLIP, SH, SW, fmt)
    if fmt == "rgb24":
        packed = planes.reshape(-1)
    else:
        packed = np.concatenate([np.concatenate([p[t].ravel() for p in planes]) for t in range(T_CLIP)])
    return planes, packed, DeviceFrames.from_decoded(DecodedClip(packed.copy(), T_CLIP, SH, SW, fmt), torch.device(DEV))


def _pack(planes, fmt):
    if fmt == "rgb24":
        return torch.from_numpy(planes.reshape(-1))
    return torch.from_numpy(np.concatenate([np.concatenate([p[t].ravel() for p in planes]) for t in range(T_CLIP)]))


def _moving_tube(K):
    boxes = np.empty((len(ROWS), K, 4), dtype=np.float32)
    for r in range(len(ROWS)):
        for k in range(K):
            x0, y0 = 2.3 + 7.5 * r + 3 * k, 3.1 + 4.2 * r - 2 * k
            boxes[r, k] = [x0, y0, x0 + 9.7 + k, y0 + 8.4]
    return boxes


@pytest.mark.parametrize("fmt", ["yuv420p", "rgb24"])
def test_redact_with_held_dense_boxes_equals_redact_with_a_frame_map(fmt):
    from tubedetr_amd.render import densify, redact

    dev = torch.device(DEV)
    _, packed, frames = _clip(fmt, 23)
    boxes = torch.from_numpy(_moving_tube(2)).to(dev)
    span = torch.tensor([[1, 3], [0, 4]], device=dev)
    fmap = torch.tensor([i // 5 if i <= ROWS[-1] else -1 for i in range(T_CLIP)], dtype=torch.int32, device=dev)
    dense = densify(boxes, T_CLIP, row_frame=ROWS, span=span, mode="hold")
    a = redact(frames, dense.boxes, mode="mosaic", cell=6, margin=(1, 4))
    b = redact(frames, boxes, span=span, frame_map=fmap, mode="mosaic", cell=6, margin=(1, 4))
    torch.cuda.synchronize()
    assert torch.equal(a.data, b.data) and not torch.equal(a.data.cpu(), torch.from_numpy(packed))
    assert dense.boxes.shape == (T_CLIP, 2, 4) and dense.span.tolist() == [[5, 15], [0, 20]] and dense.valid.dtype == torch.bool and dense.heat is None


@pytest.mark.parametrize("fmt", ["yuv420p", "rgb24"])
def test_redact_with_hull_boxes_equals_the_reference_fed_the_reference_boxes(fmt):
    from tubedetr_amd.render import color_in_space, densify, redact

    dev = torch.device(DEV)
    planes, _, frames = _clip(fmt, 24)
    tube_np = _moving_tube(2)
    tube_np[2, 1, 0] = np.nan
    span = [[1, 3], [0, 4]]
    boxes, span_t = torch.from_numpy(tube_np).to(dev), torch.tensor(span, device=dev)
    mode = torch.cuda.get_sync_debug_mode()
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")  # neither densify (with a host table to upload) nor redact may synchronise
    try:
        dense = densify(boxes, T_CLIP, row_frame=ROWS, span=span_t, mode="hull", smooth=1)
        out = redact(frames, dense.boxes, mode="fill", color=(200, 90, 30))
    finally:
        torch.cuda.set_sync_debug_mode(mode)
    torch.cuda.synchronize()
    ref = densify_ref(tube_np, T_CLIP, first=0, step=5, span=span, mode="hull", smooth=1)
    assert torch.equal(dense.boxes.cpu().view(torch.int32), torch.from_numpy(ref["dense"].view(np.int32)))
    assert torch.equal(dense.valid.cpu(), torch.from_numpy(ref["valid"].astype(bool))) and torch.equal(dense.span.cpu(), torch.from_numpy(ref["span"]))
    want = redact_ref(planes, fmt, boxes=dense_floats(ref), mode="fill", color=color_in_space((200, 90, 30), fmt))
    assert torch.equal(out.data.cpu(), _pack(want, fmt))
    held = redact_ref(planes, fmt, boxes=tube_np, span=span, frame_map=[i // 5 if i <= 20 else -1 for i in range(T_CLIP)], mode="fill", color=color_in_space((200, 90, 30), fmt))
    assert not torch.equal(_pack(held, fmt), _pack(want, fmt))  # the cover hides what a held box leaves in the clear


@pytest.mark.parametrize("fmt", ["yuv420p", "rgb24"])
def test_annotate_with_lerp_boxes_span_and_heat_equals_the_reference_likewise(fmt):
    from tubedetr_amd.render import TubeStyle, annotate, color_in_space, densify

    dev = torch.device(DEV)
    planes, _, frames = _clip(fmt, 25)
    tube_np = _moving_tube(1)[:, 0]
    heat_np = np.random.default_rng(26).integers(0, 256, (len(ROWS), 3, 5), dtype=np.uint8)
    style = TubeStyle(box_color=(200, 90, 30), thickness=2, heat_color=(40, 60, 220), heat_alpha=160, dim_color=(10, 10, 10), dim_alpha=100)
    # two clips in one pooled launch: a host table and a device table
    dense = densify([torch.from_numpy(tube_np).to(dev)] * 2, T_CLIP, row_frame=[ROWS, torch.tensor(ROWS, dtype=torch.int32, device=dev)],
                    span=[torch.tensor([1, 3], device=dev)] * 2, heat=[torch.from_numpy(heat_np).to(dev)] * 2, mode=["lerp", "lerp"])
    out = annotate(frames, dense[0].boxes, span=dense[0].span, heat=dense[0].heat, style=style)
    torch.cuda.synchronize()
    ref = densify_ref(tube_np, T_CLIP, row_frame=ROWS, span=[1, 3], heat=heat_np, mode="lerp")
    for d in dense:
        assert d.boxes.shape == (T_CLIP, 4) and d.span.shape == (2,) and d.valid.shape == (T_CLIP,) and d.heat.shape == (T_CLIP, 3, 5)
        assert torch.equal(d.boxes.cpu().view(torch.int32), torch.from_numpy(ref["dense"][:, 0].view(np.int32)))
        assert torch.equal(d.heat.cpu(), torch.from_numpy(ref["heat"])) and d.span.tolist() == ref["span"][0].tolist() == [5, 15]
    colours = {k: color_in_space(getattr(style, k), fmt) for k in ("box_color", "heat_color", "dim_color")}
    want = overlay_ref(planes, fmt, boxes=dense_floats(ref)[:, 0], span=ref["span"][0], heat=ref["heat"], thickness=2, heat_alpha=160, dim_alpha=100, **colours)
    assert torch.equal(out.data.cpu(), _pack(want, fmt))
