"""What tubedetr_amd.render's wrappers refuse, to the letter - the Python counterpart of what tests/test_frame_jobs_cpu.py pins for
the C side: callers log these texts.  One call per ``raise ValueError`` that a wrapper reaches with T = 2 frames of 6 x 8 and
n_tube = 2, the list-length refusals, and the cases where two refusals compete.  Nothing here launches a kernel but the pool
test at the end; the device is needed because ``DeviceFrames`` live on it."""
import re

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
T, H, W = 2, 6, 8


def _frames(T=T, fmt="yuv420p"):
    from tubedetr_amd.render import DeviceFrames

    nb = 144 if fmt == "rgb24" else 72
    return DeviceFrames(torch.zeros(T * nb, dtype=torch.uint8, device=DEV), T, H, W, fmt)


def _t(shape, dtype=torch.float32, device=DEV, every=1):
    return torch.zeros(shape, dtype=dtype, device=device)[..., ::every]


def _cases(live: bool):
    """id -> (wrapper name, positional arguments, keyword arguments, the full text).  ``live`` False: the same table with None for
    every frame and tensor - the ids, which pytest wants before there is a device to build the arguments on."""
    from tubedetr_amd.render import FrameStats, TubeSetStyle, TubeStyle

    def nothing(*args, **kwargs):
        return None

    mk_frames, mk = (_frames, _t) if live else (nothing, nothing)
    F, B, A = mk_frames(), mk((2, 4)), mk((2,), torch.uint8)
    B2, S1, S2 = mk((2, 2, 4)), mk((2,), torch.int64), mk((2, 2), torch.int64)
    cpu = mk((2, 4), device="cpu")
    frames = "frames: DeviceFrames on one device"
    out = "out: DeviceFrames of the clip's geometry and pixel format on its device"
    boxes_t = "boxes: a torch.float32 tensor [..., 4] on cuda:0"
    stats = FrameStats(mk((2, 64), torch.int32), mk((2,), torch.int32), 48)
    c = {}

    def add(ident, fn, args, kw, text):
        assert f"{fn}-{ident}" not in c
        c[f"{fn}-{ident}"] = (fn, args, kw, text)

    # ---- annotate
    add("clip-0", "annotate", ([5], [B]), {}, frames)  # (an AttributeError before the wrappers shared one prologue)
    add("boxes-length", "annotate", ([F, F], [B]), {}, "boxes: 1 entries for 2 clips")
    add("boxes-no-list", "annotate", ([F, F], B), {}, "boxes: a list with one entry per clip")
    add("out-length", "annotate", ([F, F], [B, B]), dict(out=[None]), "out: 1 entries for 2 clips")
    add("clip-1", "annotate", ([F, 5], [B, B]), {}, frames)
    add("boxes-host", "annotate", (F, cpu), {}, boxes_t)
    add("span-dtype", "annotate", (F, B), dict(span=mk((2,), torch.int32)), "span: a torch.int64 tensor [..., 2] on cuda:0")
    add("heat-dtype", "annotate", (F, B), dict(heat=mk((2, 2, 2))), "heat: a torch.uint8 tensor [..., ] on cuda:0")
    add("map-length", "annotate", (F, B), dict(frame_map=mk((3,), torch.int32)), "frame_map: a torch.int32 tensor [..., 2] on cuda:0")
    add("dims", "annotate", (F, B2), {}, "boxes (n_tube, 4), span (2,), heat (n_tube, mh, mw), frame_map (T,)")
    add("rows", "annotate", (F, B), dict(heat=mk((3, 2, 2), torch.uint8)), "boxes have 2 tube rows, heat has 3")
    add("out", "annotate", (F, B), dict(out=mk_frames(3)), out)
    add("out-format", "annotate", (F, B), dict(out=mk_frames(fmt="nv12")), out)
    add("grid", "annotate", (F, B), dict(heat=mk((2, 257, 1), torch.uint8)), "token grid 257 x 1: sides in 1..256")
    add("boxes-before-out", "annotate", (F, cpu), dict(out=mk_frames(3)), boxes_t)
    # ---- annotate_tubes
    add("clip-0", "annotate_tubes", ([5], [B]), {}, frames)
    add("style", "annotate_tubes", (F, B), dict(style=TubeStyle()), "style: a TubeSetStyle")
    add("frames-before-style", "annotate_tubes", ([5], [B]), dict(style=TubeStyle()), frames)
    add("tags-length", "annotate_tubes", ([F, F], [B, B]), dict(tags=[["A"]]), "tags: 1 entries for 2 clips")
    add("clip-1", "annotate_tubes", ([F, 5], [B, B]), {}, frames)
    add("boxes-host", "annotate_tubes", (F, cpu), {}, boxes_t)
    add("dims", "annotate_tubes", (F, mk((1, 2, 2, 4))), {}, "boxes (n_tube, 4) or (n_tube, K, 4), span (2,) or (K, 2), heat (n_tube, mh, mw), frame_map (T,)")
    add("K", "annotate_tubes", (F, mk((2, 9, 4))), {}, "K = 9 tubes per clip: 1..8")
    add("span", "annotate_tubes", (F, B2), dict(span=S1), "span: (2,) for one tube, (2, 2) for 2")
    add("grid", "annotate_tubes", (F, B), dict(heat=mk((2, 257, 1), torch.uint8)), "heat: uint8 (n_tube, mh, mw) with mh and mw in 1..256")
    add("rows", "annotate_tubes", (F, B), dict(heat=mk((3, 2, 2), torch.uint8)), "boxes have 2 tube rows, heat has 3")
    add("timeline-rows", "annotate_tubes", (F, None), dict(span=S1, style=TubeSetStyle(lane_h=1)), "a timeline (style.lane_h > 0) needs boxes or heat with 1..1048576 tube rows")
    add("timeline-fit", "annotate_tubes", (F, B2), dict(style=TubeSetStyle(lane_h=4)), "K lane_h = 2 x 4 rows do not fit a frame of 6 rows")
    add("tags-no-boxes", "annotate_tubes", (F, None), dict(tags=["A"]), "tags need boxes")
    add("tags-tensor", "annotate_tubes", (F, B), dict(tags=mk((2, 9, 7), torch.uint8)), "tags: uint8 (1, h, w) with h in 1..32 and w in 1..256, or 1 strings")
    add("tags-dtype", "annotate_tubes", (F, B), dict(tags=mk((1, 9, 7))), "tags: a torch.uint8 tensor [..., ] on cuda:0")
    add("tags-string", "annotate_tubes", (F, B), dict(tags="A"), "texts: a list of 1..8 strings")
    add("tags-glyph", "annotate_tubes", (F, B), dict(tags=["a!"]), "label 'A!': no glyph for '!' (digits, A-Z, space and . : % - #)")
    add("tags-long", "annotate_tubes", (F, B), dict(tags=["A" * 43]), f"label '{'A' * 43}': more than 42 characters")
    add("tags-count", "annotate_tubes", (F, B), dict(tags=["A", "B"]), "tags: 2 labels for 1 tubes")
    add("out", "annotate_tubes", (F, B), dict(out=mk_frames(3)), out)
    add("tags-before-out", "annotate_tubes", (F, B), dict(tags=["A", "B"], out=mk_frames(3)), "tags: 2 labels for 1 tubes")
    # ---- crop_tubes
    add("clip-0", "crop_tubes", ([5], [B]), {}, frames)
    add("size-int", "crop_tubes", (F, B), dict(size=5), "size 5 and margin (0, 1): two integers each")
    add("size-float", "crop_tubes", (F, B), dict(size=(2.5, 4)), "size (2.5, 4) and margin (0, 1): two integers each")
    add("size-zero", "crop_tubes", (F, B), dict(size=(0, 4)), "size 0 x 4: sides in 1..4096")
    add("margin-den", "crop_tubes", (F, B), dict(margin=(0, 0)), "margin denominator 0: 1..1024")
    add("margin", "crop_tubes", (F, B), dict(margin=(5, 1)), "margin 5/1: between 0 and 4")
    add("keep-aspect", "crop_tubes", (F, B), dict(keep_aspect=2), "keep_aspect 2: a bool")
    add("frames-before-size", "crop_tubes", ([5], [B]), dict(size=5), frames)
    add("size-before-lists", "crop_tubes", ([F, F], [B]), dict(size=5), "size 5 and margin (0, 1): two integers each")
    add("span-length", "crop_tubes", ([F, F], [B, B]), dict(span=[S1]), "span: 1 entries for 2 clips")
    add("clip-1", "crop_tubes", ([F, 5], [B, B]), {}, frames)
    add("boxes-none", "crop_tubes", (F, None), {}, "boxes: a torch.float32 tensor (n_tube, 4) per clip")
    add("boxes-host", "crop_tubes", (F, cpu), {}, boxes_t)
    add("dims", "crop_tubes", (F, mk((0, 4))), {}, "boxes (n_tube, 4) with n_tube >= 1, span (2,), frame_map (T,)")
    add("dims-K", "crop_tubes", (F, B2), {}, "boxes (n_tube, 4) with n_tube >= 1, span (2,), frame_map (T,)")
    # ---- redact
    add("clip-0", "redact", ([5], [B]), {}, frames)
    add("mode", "redact", (F, B), dict(mode="x"), "mode 'x': one of ('fill', 'mosaic', 'blur')")
    add("margin-int", "redact", (F, B), dict(margin=3), "margin 3: two integers")
    add("cell-float", "redact", (F, B), dict(cell=2.5), "cell 2.5, radius 8 and margin (0, 1): integers")
    add("cell-odd", "redact", (F, B), dict(cell=3), "cell 3: an even number in 2..256")
    add("radius", "redact", (F, B), dict(mode="blur", radius=0), "radius 0: 1..64")
    add("margin-den", "redact", (F, B), dict(margin=(0, 1025)), "margin denominator 1025: 1..1024")
    add("margin", "redact", (F, B), dict(margin=(9, 2)), "margin 9/2: between 0 and 4")
    add("invert", "redact", (F, B), dict(invert=2), "invert 2: a bool")
    add("color", "redact", (F, B), dict(color=(1, 2)), "color (1, 2): three integers in 0..255")
    add("mode-before-color", "redact", (F, B), dict(mode="x", color=(1, 2)), "mode 'x': one of ('fill', 'mosaic', 'blur')")
    add("map-length", "redact", ([F, F], [B, B]), dict(frame_map=[None]), "frame_map: 1 entries for 2 clips")
    add("clip-1", "redact", ([F, 5], [B, B]), {}, frames)
    add("boxes-none", "redact", (F, None), {}, "boxes: a torch.float32 tensor (n_tube, 4) or (n_tube, K, 4) per clip")
    add("boxes-host", "redact", (F, cpu), {}, boxes_t)
    add("dims", "redact", (F, mk((0, 4))), {}, "boxes (n_tube, 4) or (n_tube, K, 4) with n_tube >= 1, frame_map (T,)")
    add("K", "redact", (F, mk((2, 9, 4))), {}, "boxes carry K = 9 rectangles per tube row: 1..8")
    add("span", "redact", (F, B2), dict(span=S1), "span: (2,) for one tube, (2, 2) for 2")
    add("span-K", "redact", (F, B), dict(span=S2), "span: (2,) for one tube, (1, 2) for 1")
    add("out", "redact", (F, B), dict(out=mk_frames(3)), out)
    add("blur-in-place", "redact", (F, B), dict(mode="blur", out=F), 'mode "blur" cannot run in place (out is the clip itself): it reads neighbours that are already rewritten')
    # ---- densify
    add("row-frame-length", "densify", ([B, B], 4), dict(row_frame=[None]), "row_frame: 1 entries for 2 clips")
    add("T-length", "densify", ([B, B], [4]), {}, "T: 1 entries for 2 clips")
    add("shots-length", "densify", ([B, B], 4), dict(shots=[None]), "shots: 1 entries for 2 clips")
    add("shots-t0", "densify", (B, 4), dict(shots=mk((4,), torch.int32), shots_t0=1 << 24), "shots_t0 = 16777216: an integer in -8388608..8388608")
    add("host-boxes", "densify", (cpu, 4), {}, "boxes: a torch.float32 tensor (n_tube, 4) or (n_tube, K, 4) on the device per clip")
    add("mode-before-host-boxes", "densify", (cpu, 4), dict(mode="x"), "mode 'x': one of ('hold', 'lerp', 'hull')")
    add("mode", "densify", (B, 4), dict(mode="x"), "mode 'x': one of ('hold', 'lerp', 'hull')")
    add("T", "densify", (B, -1), {}, "T = -1: an integer in 0..1048576")
    add("t0", "densify", (B, 4), dict(t0=1 << 24), "t0 = 16777216: an integer in -8388608..8388608")
    add("first", "densify", (B, 4), dict(first=0.5), "first = 0.5: an integer in -8388608..8388608")
    add("step", "densify", (B, 4), dict(step=0), "step = 0: an integer in 1..65536")
    add("smooth", "densify", (B, 4), dict(smooth=17), "smooth = 17: an integer in 0..16")
    add("boxes-dtype", "densify", (mk((2, 4), torch.float64), 4), {}, boxes_t)
    add("dims", "densify", (mk((0, 4)), 4), {}, "boxes (n_tube, 4) or (n_tube, K, 4) with n_tube >= 1")
    add("K", "densify", (mk((2, 9, 4)), 4), {}, "boxes carry K = 9 rectangles per tube row: 1..8")
    add("span", "densify", (B2, 4), dict(span=S1), "span: (2,) for one tube, (2, 2) for 2")
    add("heat", "densify", (B, 4), dict(heat=mk((3, 2, 2), torch.uint8)), "heat: uint8 (2, mh, mw) with mh and mw in 1..256")
    add("row-frame-dtype", "densify", (B, 4), dict(row_frame=mk((2,), torch.int64)), "row_frame: a torch.int32 tensor [..., 2] on cuda:0")
    add("row-frame-dims", "densify", (B, 4), dict(row_frame=mk((1, 2), torch.int32)), "row_frame: int32 (2,)")
    add("row-frame-entry", "densify", (B, 4), dict(row_frame=[0, 1.5]), "row_frame entry = 1.5: an integer in -8388608..8388608")
    add("row-frame-count", "densify", (B, 4), dict(row_frame=[0]), "row_frame has 1 entries for 2 tube rows")
    add("shots", "densify", (B, 4), dict(shots=mk((2, 2), torch.int32)), "shots: a Shots, or an int32 (n,) tensor of shot ids with n <= 1048576")
    add("shots-dtype", "densify", (B, 4), dict(shots=mk((4,), torch.int64)), "shots: a torch.int32 tensor [..., ] on cuda:0")
    # ---- frame_stats
    add("clip-0", "frame_stats", ([5],), {}, frames)
    add("clip-1", "frame_stats", ([F, 5],), {}, frames)
    add("step", "frame_stats", (F,), dict(step=9), "step = 9: an integer in 1..8")
    # ---- shot_cuts
    add("hist", "shot_cuts", (F,), dict(hist=3), "hist 3: two integers (numerator, denominator)")
    add("hist-num", "shot_cuts", (F,), dict(hist=(-1, 4)), "hist numerator = -1: an integer in 0..1048576")
    add("sad-den", "shot_cuts", (F,), dict(sad=(8, 0)), "sad denominator = 0: an integer in 1..1048576")
    add("peak", "shot_cuts", (F,), dict(peak=(1, 2, 3)), "peak (1, 2, 3): two integers (numerator, denominator)")
    add("window", "shot_cuts", (F,), dict(window=17), "window = 17: an integer in 0..16")
    add("step", "shot_cuts", (F,), dict(step=0), "step = 0: an integer in 1..8")
    add("window-before-step", "shot_cuts", (F,), dict(step=0, window=17), "window = 17: an integer in 0..16")
    add("kinds", "shot_cuts", ([stats, F],), {}, "frames_or_stats: DeviceFrames or FrameStats, one kind per call")
    add("stats", "shot_cuts", (FrameStats(mk((2, 64), torch.int64), mk((2,), torch.int32), 48),), {}, "FrameStats: hist int32 (T, 64) and sad int32 (T,) on the device")
    add("stats-n", "shot_cuts", (FrameStats(mk((2, 64), torch.int32), mk((2,), torch.int32), 0),), {}, "FrameStats.n = 0: an integer in 1..16777216")
    # ---- follow
    add("radius-length", "follow", ([F, F], [B, B], [A, A]), dict(radius=[8]), "radius: 1 entries for 2 clips")
    add("accept-length", "follow", ([F, F], [B, B], [A, A]), dict(accept=[24]), "accept: 1 entries for 2 clips")
    add("radius", "follow", (F, B, A), dict(radius=17), "radius = 17: an integer in 0..16")
    add("reach", "follow", (F, B, A), dict(reach=0), "reach = 0: an integer in 1..64")
    add("accept", "follow", (F, B, A), dict(accept=(1, 2, 3)), "accept (1, 2, 3): an integer, or two integers (numerator, denominator)")
    add("accept-num", "follow", (F, B, A), dict(accept=-1), "accept numerator = -1: an integer in 0..1048576")
    add("accept-den", "follow", (F, B, A), dict(accept=(1, 0)), "accept denominator = 0: an integer in 1..1048576")
    add("radius-before-frames", "follow", (5, B, A), dict(radius=17), "radius = 17: an integer in 0..16")
    add("clip-0", "follow", (5, B, A), {}, frames)
    add("boxes-length", "follow", ([F, F], [B], [A, A]), {}, "boxes: 1 entries for 2 clips")
    add("anchor-no-list", "follow", ([F, F], [B, B], A), {}, "anchor: a list with one entry per clip")
    add("clip-1", "follow", ([F, 5], [B, B], [A, A]), {}, frames)
    add("boxes-host", "follow", (F, cpu, A), {}, boxes_t)
    add("boxes-rows", "follow", (F, mk((3, 4)), A), {}, "boxes: (2, 4) or (2, K, 4), one row per frame of the clip")
    add("boxes-none", "follow", (F, None, A), {}, "boxes: (2, 4) or (2, K, 4), one row per frame of the clip")
    add("K", "follow", (F, mk((2, 9, 4)), A), {}, "boxes carry K = 9 rectangles per frame: 1..8")
    add("in-place", "follow", (F, mk((2, 8), every=2), A), dict(in_place=True), "in_place: boxes must be a contiguous tensor")
    add("anchor-none", "follow", (F, B, None), {}, "anchor: a uint8 or bool (2,) tensor on the device")
    add("anchor-dtype", "follow", (F, B, mk((2,), torch.int32)), {}, "anchor: a torch.uint8 tensor [..., 2] on cuda:0")
    add("anchor-dims", "follow", (F, B, mk((1, 2), torch.bool)), {}, "anchor: a uint8 or bool (2,) tensor on the device")
    add("shots-dims", "follow", (F, B, A), dict(shots=mk((1, 2), torch.int32)), "shots: a Shots, or an int32 (2,) tensor of shot ids")
    add("shots-dtype", "follow", (F, B, A), dict(shots=mk((2,), torch.int64)), "shots: a torch.int32 tensor [..., 2] on cuda:0")
    # ---- export
    add("clip-0", "export", ([5],), {}, frames)
    add("multiple", "export", (F,), dict(multiple=0), "multiple = 0: an integer in 1..256")
    add("pad-color", "export", (F,), dict(pad_color=(0, 0, 256)), "pad_color (0, 0, 256): three integers in 0..255")
    add("pix-fmt", "export", (F,), dict(pix_fmt="x"), "pix_fmt 'x': one of ('rgb24', 'yuv420p', 'nv12')")
    add("frames-before-multiple", "export", ([5],), dict(multiple=0), frames)
    add("take-length", "export", ([F, F],), dict(take=[None]), "take: 1 entries for 2 clips")
    add("To-no-list", "export", ([F, F],), dict(To=2), "To: a list with one entry per clip")
    add("clip-1", "export", ([F, 5],), {}, frames)
    add("size-three", "export", (F,), dict(size=(1, 2, 3)), "size (1, 2, 3): (oh, ow) or the short side")
    add("size-oh", "export", (F,), dict(size=(7, 8)), "oh = 7: an integer in 1..6")
    add("size-ow", "export", (F,), dict(size=(6, 9)), "ow = 9: an integer in 1..8")
    add("size-short", "export", (F,), dict(size=7), "size = 7: an integer in 1..6")
    add("take-entry", "export", (F,), dict(take=[0, 1.5]), "take = 1.5: an integer in -2147483648..2147483647")
    add("take-dtype", "export", (F,), dict(take=mk((2,), torch.int64)), "take: a torch.int32 tensor [..., ] on cuda:0")
    add("take-dims", "export", (F,), dict(take=mk((1, 2), torch.int32)), "take: int32 (To,)")
    add("To-without-take", "export", (F,), dict(To=3), "To = 3 without take: it is T = 2")
    add("To", "export", (F,), dict(take=[0, 1], To=3), "To = 3: an integer in 0..2")
    return c


@pytest.fixture(scope="module")
def cases():
    return _cases(live=True)


@pytest.mark.parametrize("ident", list(_cases(live=False)))
def test_refusal_text(cases, ident):
    from tubedetr_amd import render

    fn, args, kw, text = cases[ident]
    with pytest.raises(ValueError, match="^" + re.escape(text) + "$"):
        getattr(render, fn)(*args, **kw)


@pytest.mark.parametrize("fn", ["annotate", "crop_tubes", "redact", "annotate_tubes", "follow", "export", "frame_stats"])
def test_a_bad_second_clip_is_refused_before_anything_is_allocated(fn):
    """Every check for every clip comes before the first allocation: a refusal leaves the allocator where it was."""
    from tubedetr_amd import render

    F, B, A = _frames(), _t((2, 4)), _t((2,), torch.uint8)
    bad = _t((2, 4), device="cpu")
    args = {"annotate": ([F, F], [B, bad]), "crop_tubes": ([F, F], [B, bad]), "redact": ([F, F], [B, bad]), "annotate_tubes": ([F, F], [B, bad]),
            "follow": ([F, F], [B, bad], [A, A]), "export": ([F, 5],), "frame_stats": ([F, 5],)}[fn]
    text = "frames: DeviceFrames on one device" if fn in ("export", "frame_stats") else "boxes: a torch.float32 tensor [..., 4] on cuda:0"
    before = torch.cuda.memory_allocated(), torch.cuda.memory_stats()["allocation.all.allocated"]
    with pytest.raises(ValueError, match="^" + re.escape(text) + "$"):
        getattr(render, fn)(*args)
    # (the bytes alone would not show a buffer that was made and freed again while the refusal travelled up: count the allocations too)
    assert (torch.cuda.memory_allocated(), torch.cuda.memory_stats()["allocation.all.allocated"]) == before


def test_the_table_pool_hands_the_same_pair_out_again():
    """A pooled (pinned, device, event) table is taken again once its event has completed: with a synchronise after every call
    the pool does not grow and every call gets the same pair - ``moments_topk``'s upload in between too."""
    from tubedetr_amd import frame_jobs
    from tubedetr_amd.models import postprocessors
    from tubedetr_amd.render import redact

    dev = torch.device(DEV)
    F, B = _frames(), _t((2, 4))
    torch.cuda.synchronize()
    held = [frame_jobs.take_table(1, dev) for _ in range(frame_jobs.tables_pooled())]  # what earlier tests left: every event has completed
    assert frame_jobs.tables_pooled() == 0

    def pair():
        triple = frame_jobs.take_table(1, dev)
        frame_jobs.release_table(triple)
        torch.cuda.synchronize()
        return triple[0].data_ptr(), triple[1].data_ptr()

    sizes, pairs = [], []
    for i in range(5):
        redact(F, B, mode="fill")
        torch.cuda.synchronize()
        sizes.append(frame_jobs.tables_pooled())
        pairs.append(pair())
        if i == 2:
            m = postprocessors.moments_topk(_t((2, 4, 2)), video_ids=[0, 0], k=1)
            table, triple = postprocessors._upload(torch.tensor([1, 2, 3], dtype=torch.int32), dev)
            assert (triple[0].data_ptr(), triple[1].data_ptr()) == pairs[0] and table.data_ptr() == pairs[0][1]
            postprocessors._release(triple)
            torch.cuda.synchronize()
            assert m.count.tolist() == [1] and frame_jobs.tables_pooled() == 1
    assert sizes == [1] * 5
    assert pairs == [pairs[0]] * 5
    for triple in held:
        frame_jobs.release_table(triple)
