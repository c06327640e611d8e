"""td_tube_follow and tubedetr_amd.render.follow on the GPU, against the numpy restatement of the header's rule
(tests/follow_ref.py).  Every comparison is exact: the boxes as their bit patterns, the rest as bytes; the rule is integers and
one fp32 addition per coordinate, so there is no tolerance.

Canaries: the outputs of a job lie in ONE buffer of 0xFF bytes, at least 64 of them in front of each output and behind the last,
and the whole buffer is compared - so a result that leans on what the outputs held, or a byte written beside them, shows.  The
padding of pitched source rows and between the planes and frames is random bytes that no result may depend on; the source and
the input boxes are compared with what was uploaded after every launch."""
import functools

import numpy as np
import pytest
import torch

from follow_ref import F32, corner_error, follow_ref, luma_of_planes, scene
from overlay_ref import overlay_ref
from redact_ref import redact_ref
from shots_ref import densify_shots_ref, frame_stats_ref, shot_cuts_ref
from test_overlay_gpu import as_rows, layout, place
from tube_dense_ref import dense_floats, densify_ref

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GAP = 64
PARTS = (("out", 16), ("offset", 8), ("cost", 4), ("status", 1))  # name, bytes per (t, k)


@functools.lru_cache(maxsize=None)
def the_scene(T=25, sh=96, sw=128):
    return scene(T, sh, sw)


def planes_of(luma, fmt, seed=0, colour=False):
    """Planes of ``fmt`` whose luma is ``luma`` (rgb24 with ``colour``: R, G and B get independent noise, and the luma is what the
    rule makes of them); the chroma planes are random bytes."""
    rng = np.random.default_rng(300 + seed)
    T, sh, sw = luma.shape
    ch, cw = (sh + 1) // 2, (sw + 1) // 2
    if fmt == "rgb24":
        rgb = np.repeat(luma[..., None], 3, -1)
        return np.clip(rgb.astype(np.int64) + rng.integers(-12, 13, rgb.shape), 0, 255).astype(np.uint8) if colour else rgb.copy()
    if fmt == "yuv420p":
        return (luma.copy(), rng.integers(0, 256, (T, ch, cw), dtype=np.uint8), rng.integers(0, 256, (T, ch, cw), dtype=np.uint8))
    return (luma.copy(), rng.integers(0, 256, (T, ch, cw, 2), dtype=np.uint8))


def moving_picture(T, sh, sw, seed):
    """Random luma that moves by (1, 2) pixels per frame, with +-2 levels of noise: a match has somewhere to go."""
    rng = np.random.default_rng(400 + seed)
    base = rng.integers(0, 256, (sh + T, sw + 2 * T)).astype(np.float64)
    base = (base + np.roll(base, 1, 0) + np.roll(base, 1, 1)) / 3
    frames = [base[t:t + sh, 2 * t:2 * t + sw] + rng.integers(-2, 3, (sh, sw)) for t in range(T)]
    return np.clip(np.stack(frames), 0, 255).astype(np.uint8) if T else np.zeros((0, sh, sw), np.uint8)


def random_boxes(T, K, sh, sw, seed):
    rng = np.random.default_rng(500 + seed)
    x0, y0 = rng.uniform(-0.2 * sw, 0.8 * sw, (T, K)), rng.uniform(-0.2 * sh, 0.8 * sh, (T, K))
    return np.stack([x0, y0, x0 + rng.uniform(1, 0.7 * sw, (T, K)), y0 + rng.uniform(1, 0.7 * sh, (T, K))], -1).astype(F32)


def every(T, n, first=0):
    return ((np.arange(T) - first) % n == 0).astype(np.uint8)


def spec(fmt, luma, boxes, anchor, shot=None, radius=8, reach=3, accept=(24, 1), pad=3, gap=37, alias=False, absent=(), seed=0, colour=False):
    """``pad`` bytes behind every row and ``gap`` bytes in front of every plane: with 3 and 37, rows and frames at odd addresses."""
    boxes = np.ascontiguousarray(boxes, dtype=F32)
    boxes = boxes[:, None] if boxes.ndim == 2 else boxes
    return dict(fmt=fmt, luma=luma, boxes=boxes, anchor=np.asarray(anchor, dtype=np.uint8), shot=None if shot is None else np.asarray(shot, dtype=np.int32), radius=radius,
                reach=reach, accept=accept, pad=pad, gap=gap, alias=alias, absent=tuple(absent), seed=seed, colour=colour)


def out_layout(n, absent):
    offs, o = {}, 0
    for name, size in PARTS:
        if name in absent:
            continue
        o = (o + GAP + 15) // 16 * 16
        offs[name] = (o, size * n)
        o += size * n
    return offs, o + GAP


def run_follow(specs, launches=1):
    """ONE launch (or the same one again) of all specs; asserts every job's whole output buffer against the reference and returns
    the references."""
    from tubedetr_amd.render import follow_job, tube_follow

    dev = torch.device(DEV)
    jobs, keep, checks, refs = [], [], [], []
    for s in specs:
        assert not (s["alias"] and launches > 1)
        rng = np.random.default_rng(100 + s["seed"])
        T, K = s["boxes"].shape[:2]
        sh, sw = s["luma"].shape[1:]
        planes = planes_of(s["luma"] if T else np.zeros((1, sh, sw), np.uint8), s["fmt"], s["seed"], s["colour"])
        want = follow_ref(luma_of_planes(planes, s["fmt"])[:T], s["boxes"], s["anchor"], s["shot"], s["radius"], s["reach"], s["accept"])
        refs.append(want)
        rows = [r[:T] for r in as_rows(planes, s["fmt"])]  # (a clip without frames still has planes with addresses)
        lay = layout(rows, s["gap"], s["pad"])
        src_np = place(rng.integers(0, 256, max(lay["total"], 1), dtype=np.uint8), rows, lay)
        src = torch.from_numpy(src_np).to(dev)
        offs, total = out_layout(T * K, s["absent"])
        expect = np.full(total, 0xFF, dtype=np.uint8)
        for name, (a, size) in offs.items():
            expect[a:a + size] = np.ascontiguousarray(want[name]).view(np.uint8).reshape(-1)
        first = np.full(total, 0xFF, dtype=np.uint8)
        if s["alias"]:
            a, size = offs["out"]
            first[a:a + size] = s["boxes"].view(np.uint8).reshape(-1)
        out = torch.from_numpy(first).to(dev)
        at = lambda name: out.data_ptr() + offs[name][0] if name in offs else None  # noqa: E731
        boxes = torch.from_numpy(s["boxes"].reshape(-1) if T else np.zeros(4, F32)).to(dev)
        anchor = torch.from_numpy(s["anchor"] if T else np.zeros(1, np.uint8)).to(dev)
        shot = torch.from_numpy(s["shot"] if T else np.zeros(1, np.int32)).to(dev) if s["shot"] is not None else None
        jobs.append(follow_job(None, T, sh, sw, at("out") if s["alias"] else boxes.data_ptr(), anchor.data_ptr(), at("out"), K, s["fmt"], shot.data_ptr() if shot is not None else None,
                               s["radius"], s["reach"], s["accept"], at("offset"), at("cost"), at("status"), src_planes=[src.data_ptr() + o for o in lay["offs"]],
                               src_pitches=lay["pitches"], src_frame_stride=lay["stride"]))
        keep.append((src, boxes, anchor, shot))
        checks.append((out, expect, offs, src, src_np, boxes))
    for _ in range(launches):
        tables = tube_follow(jobs, dev)
        torch.cuda.synchronize()
        del tables
        for i, (out, expect, offs, src, src_np, boxes) in enumerate(checks):
            s = specs[i]
            got = out.cpu().numpy()
            for name, (a, size) in offs.items():
                bad = int((got[a:a + size] != expect[a:a + size]).sum())
                assert bad == 0, (f"job {i} {s['fmt']} {s['luma'].shape[1]} x {s['luma'].shape[2]} K {s['boxes'].shape[1]} radius {s['radius']} reach {s['reach']}: "
                                  f"{bad} of {size} bytes of {name} differ from the reference")
            assert np.array_equal(got, expect), f"job {i}: a byte outside the outputs was written"
            assert np.array_equal(src.cpu().numpy(), src_np), f"job {i}: the source was written"
            if s["boxes"].shape[0]:
                assert np.array_equal(boxes.cpu().numpy().view(np.uint32), s["boxes"].reshape(-1).view(np.uint32)), f"job {i}: the input boxes were written"
    return refs


def three_tubes(lerp):
    """K = 3: the tube and two displaced copies of it."""
    return np.stack([lerp, lerp + F32([3, -2, 3, -2]), lerp + F32([-5.5, 4.25, -5.5, 4.25])], 1)


# ---- the scene ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt,colour", [("yuv420p", False), ("nv12", False), ("rgb24", False), ("rgb24", True)])
def test_the_scene_in_every_format_with_one_tube_and_three(fmt, colour):
    luma, true, anchor, lerp = the_scene()
    refs = run_follow([spec(fmt, luma, lerp, anchor, colour=colour, seed=1), spec(fmt, luma, three_tubes(lerp), anchor, colour=colour, seed=2)])
    if not colour:  # what the CPU test shows for the reference holds for the device, bit for bit
        assert (corner_error(refs[0]["out"][:, 0], true) <= 1).all() and (corner_error(lerp, true)[anchor == 0] >= 2).all()
        assert (refs[0]["status"][anchor == 0] == 1).all()
    assert (refs[1]["status"][anchor == 0] != 0).all() and (refs[1]["status"][anchor != 0] == 0).all()


@pytest.mark.parametrize("radius,reach", [(0, 1), (1, 3), (8, 64), (16, 1), (16, 3)])
def test_radius_and_reach(radius, reach):
    luma, true, anchor, lerp = the_scene()
    sparse = anchor.copy()
    sparse[6:19] = 0  # frames 1 .. 23 between two anchors: most of them out of a short reach
    refs = run_follow([spec("yuv420p", luma, lerp, anchor, radius=radius, reach=reach, seed=3), spec("rgb24", luma, lerp, sparse, radius=radius, reach=reach, seed=4)])
    assert (refs[1]["status"] != 0).sum() == (2 * min(reach, 23) if reach < 12 else 23)
    if radius == 16 and reach >= 3:  # the far candidates do not disturb the answer
        assert (corner_error(refs[0]["out"][:, 0], true) <= 1).all()


# ---- small frames, odd addresses ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", ["rgb24", "yuv420p", "nv12"])
def test_small_frames_with_rows_at_odd_dword_and_16_byte_addresses(fmt):
    specs = []
    for i, (sh, sw) in enumerate([(37, 53), (7, 9)]):
        luma = moving_picture(13, sh, sw, i)
        for m, (pad, gap, radius, reach) in enumerate([(3, 37, 8, 3), (0, 64, 16, 64), (0, 36, 1, 1), (11, 48, 0, 3)]):
            K = 1 + (m + i) % 3
            specs.append(spec(fmt, luma, random_boxes(13, K, sh, sw, 10 * i + m), every(13, 3 + m % 2, m % 2), radius=radius, reach=reach, accept=(40, 1), pad=pad, gap=gap,
                              seed=10 * i + m, colour=True))
    refs = run_follow(specs)
    assert sum(int((r["status"] == 1).sum()) for r in refs) > 20 and sum(int((r["offset"] != 0).sum()) for r in refs) > 20


def test_boxes_at_the_four_borders_larger_than_the_frame_and_not_finite():
    sh, sw, T = 37, 53, 13
    luma = moving_picture(T, sh, sw, 7)
    anchor = every(T, 4)
    corners = np.array([[-6, 5, 12, 20], [40, 8, 60, 30], [10, -9, 30, 9], [12, 25, 40, 50], [-20, -10, 80, 60], [0, 0, 53, 37], [52, 36, 53, 37], [-3, -3, 1, 1]], dtype=F32)
    boxes = np.stack([corners + F32([2 * t, t, 2 * t, t]) + F32(0.4 * (t % 3)) for t in range(T)])  # K = 8, moving with the picture and a little beside it
    odd = np.stack([corners[:4]] * T)  # K = 4: what is not finite or huge, in anchors and in between
    odd[4, 0] = np.nan            # an anchor frame: tube 0 of frames 2 .. 6 falls back to another anchor, or to none
    odd[8, 1, 2] = np.inf
    odd[5, 1] = [np.nan, 1, 2, 3]  # in between: copied with its bits
    odd[6, 2, 3] = -np.inf
    odd[0, 3] = 1e30              # an anchor box far outside the frame: frames 1 and 2 are copied
    odd[9, 3] = [-1e30, -1e30, 1e30, 1e30]
    odd[10, 0] = [1e30, 1e30, 2e30, 2e30]  # every sample clamped into the far corner
    odd[7, 2] = np.array([0x7FC00001, 0xFFC00000, 0x7F800001, 0x7FFFFFFF], dtype=np.uint32).view(F32)  # NaN payloads survive
    refs = run_follow([spec("yuv420p", luma, boxes, anchor, accept=(60, 1), seed=20), spec("rgb24", luma, odd, anchor, accept=(255, 1), seed=21, colour=True),
                       spec("nv12", luma, odd, anchor, radius=16, reach=64, seed=22)])
    print("matched units per tube", (refs[0]["status"] != 0).sum(0).tolist(), "accepted", int((refs[0]["status"] == 1).sum()))
    assert ((refs[0]["status"] != 0).sum(0)[[0, 2, 4, 5, 7]] == 9).all() and (refs[0]["status"] == 1).sum() >= 30  # (tubes 1, 3 and 6 leave the frame)
    assert refs[1]["status"][5, 1] == 0 and refs[1]["status"][7, 2] == 0 and refs[1]["status"][10, 0] == 1 and refs[1]["status"][9, 3] != 0


def test_no_anchors_all_anchors_and_clips_of_no_one_and_two_frames():
    luma = moving_picture(6, 20, 30, 8)
    specs = [spec("yuv420p", luma, random_boxes(6, 2, 20, 30, 30), np.zeros(6), seed=30), spec("rgb24", luma, random_boxes(6, 2, 20, 30, 31), np.ones(6), seed=31)]
    for T in (0, 1, 2):
        for fmt in ("yuv420p", "rgb24", "nv12"):
            specs.append(spec(fmt, luma[:T], random_boxes(T, 3, 20, 30, 32 + T), [1, 0][:T], seed=32 + T))
            specs.append(spec(fmt, luma[:T], random_boxes(T, 1, 20, 30, 35 + T), [0, 1][:T], shot=[0, 0][:T], seed=35 + T))
    refs = run_follow(specs)
    assert (refs[0]["status"] == 0).all() and (refs[1]["status"] == 0).all()
    assert refs[-1]["status"].tolist() == [[1], [0]] or refs[-1]["status"].tolist() == [[2], [0]]


def test_a_cut_between_a_frame_and_its_nearer_anchor():
    luma, true, anchor, lerp = the_scene()
    shot = (np.arange(25) >= 8).astype(np.int32)  # frame 7 is nearer to anchor 6; frames 8 .. 11 to anchor 12: frames 8 and 9 must not take 6
    cut = luma.copy()
    cut[8:] = 255 - cut[8:]
    refs = run_follow([spec("yuv420p", cut, lerp, anchor, shot=shot, reach=4, seed=40), spec("yuv420p", cut, lerp, anchor, seed=41), spec("rgb24", cut, lerp, anchor, shot=shot, reach=1, seed=42)])
    assert (refs[0]["status"][anchor == 0] == 1).all() and refs[1]["status"][8] == 2 and refs[1]["status"][9] == 2
    assert refs[2]["status"][[8, 9, 10]].ravel().tolist() == [0, 0, 0] and refs[2]["status"][11] == 1


def test_a_flat_picture_answers_no_shift_at_every_radius():
    flat = np.full((5, 40, 56), 93, dtype=np.uint8)
    boxes = random_boxes(5, 2, 40, 56, 50)
    refs = run_follow([spec(fmt, flat, boxes, [1, 0, 0, 0, 1], radius=radius, accept=(0, 1), seed=50 + radius) for radius in (16, 5) for fmt in ("yuv420p", "rgb24")])
    for r in refs:
        assert (r["offset"] == 0).all() and (r["cost"] == 0).all() and r["status"][1:4].ravel().tolist() == [1] * 6


def test_a_grey_frame_is_rejected_and_keeps_its_box():
    luma, true, anchor, lerp = the_scene()
    grey = luma.copy()
    grey[8] = 128
    refs = run_follow([spec("nv12", grey, lerp, anchor, seed=60), spec("rgb24", grey, three_tubes(lerp), anchor, seed=61)])
    assert refs[0]["status"][8] == 2 and refs[0]["cost"][8] > 24 * 256 and np.array_equal(refs[0]["out"][8].view(np.uint32), lerp[8].reshape(1, 4).view(np.uint32))
    assert (refs[1]["status"][8] == 2).all()


def test_out_may_be_boxes_and_every_optional_output_may_be_absent():
    luma, true, anchor, lerp = the_scene()
    specs = [spec("yuv420p", luma, three_tubes(lerp), anchor, alias=True, seed=70), spec("rgb24", luma, lerp, anchor, alias=True, absent=("offset", "cost", "status"), seed=71)]
    specs += [spec("nv12", luma, lerp, anchor, absent=(name,), seed=72 + i) for i, name in enumerate(("offset", "cost", "status"))]
    refs = run_follow(specs)
    assert np.array_equal(refs[0]["out"][anchor != 0].view(np.uint32), three_tubes(lerp)[anchor != 0].view(np.uint32))  # anchor boxes are never changed


def test_five_mixed_jobs_in_one_launch_twice_the_same_bits():
    luma, true, anchor, lerp = the_scene()
    small = moving_picture(13, 7, 9, 80)
    run_follow([spec("rgb24", luma, three_tubes(lerp), anchor, radius=16, seed=80, colour=True), spec("yuv420p", small, random_boxes(13, 8, 7, 9, 81), every(13, 3), radius=3, seed=81),
                spec("nv12", luma[:0], random_boxes(0, 2, 96, 128, 82), [], seed=82), spec("nv12", moving_picture(13, 37, 53, 83), random_boxes(13, 2, 37, 53, 83), every(13, 5, 2), radius=0,
                                                                                          reach=64, accept=(255, 1), seed=83),
                spec("yuv420p", luma, lerp, anchor, shot=np.zeros(25), radius=1, reach=1, accept=(3, 2), pad=0, gap=64, seed=84)], launches=2)


# ---- end to end at 48 x 64 ---------------------------------------------------------------------------------------------------------
E_T, E_SH, E_SW, E_STEP = 25, 48, 64, 6


def _clip(luma, fmt, seed):
    from tubedetr_amd.augment import DecodedClip
    from tubedetr_amd.render import DeviceFrames

    planes = planes_of(luma, fmt, seed, colour=True)
    T = luma.shape[0]
    packed = planes.reshape(-1) if fmt == "rgb24" else np.concatenate([np.concatenate([p[t].ravel() for p in planes]) for t in range(T)])
    return planes, DeviceFrames.from_decoded(DecodedClip(packed.copy(), T, luma.shape[1], luma.shape[2], fmt), torch.device(DEV))


def _pack(planes, fmt):
    if fmt == "rgb24":
        return torch.from_numpy(planes.reshape(-1))
    return torch.from_numpy(np.concatenate([np.concatenate([p[t].ravel() for p in planes]) for t in range(planes[0].shape[0])]))


def _no_sync(fn):
    mode = torch.cuda.get_sync_debug_mode()
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        return fn()
    finally:
        torch.cuda.set_sync_debug_mode(mode)


@pytest.mark.parametrize("fmt", ["yuv420p", "rgb24"])
def test_end_to_end_densify_follow_annotate(fmt):
    from tubedetr_amd.render import FollowedTubes, TubeStyle, anchors, annotate, color_in_space, densify, follow

    dev = torch.device(DEV)
    luma, true, anchor_np, _ = the_scene(E_T, E_SH, E_SW)
    planes, frames = _clip(luma, fmt, 90)
    rows = true[::E_STEP].copy()
    tube = torch.from_numpy(rows).to(dev)
    style = TubeStyle(box_color=(200, 90, 30), thickness=2)

    def stages():
        dense = densify(tube, E_T, first=0, step=E_STEP, mode="lerp")
        anchor = anchors(first=0, step=E_STEP, T=E_T, n_tube=len(rows), device=dev)
        followed = follow(frames, dense, anchor)
        return anchor, followed, annotate(frames, followed.boxes, style=style)

    anchor, followed, out = _no_sync(stages)
    torch.cuda.synchronize()
    assert isinstance(followed, FollowedTubes) and followed.boxes.shape == (E_T, 4) and followed.offset.shape == (E_T, 2) and followed.cost.shape == followed.status.shape == (E_T,)
    assert anchor.dtype == torch.uint8 and np.array_equal(anchor.cpu().numpy(), anchor_np)
    dense_ref = dense_floats(densify_ref(rows, E_T, first=0, step=E_STEP, mode="lerp"))[:, 0]
    want = follow_ref(luma_of_planes(planes, fmt), dense_ref, anchor_np)
    assert np.array_equal(followed.boxes.cpu().numpy().view(np.uint32), want["out"].view(np.uint32))
    assert np.array_equal(followed.offset.cpu().numpy(), want["offset"]) and np.array_equal(followed.cost.cpu().numpy().view(np.uint32), want["cost"])
    assert np.array_equal(followed.status.cpu().numpy(), want["status"]) and (want["status"] == 1).sum() >= 10 and (want["offset"] != 0).any()
    drawn = overlay_ref(planes, fmt, boxes=want["out"], thickness=2, box_color=color_in_space((200, 90, 30), fmt))
    assert torch.equal(out.data.cpu(), _pack(drawn, fmt))
    # in place: the same boxes, in the tensor that was handed over; a bool anchor is taken as it is
    mine = densify(tube, E_T, first=0, step=E_STEP, mode="lerp").boxes
    again = follow([frames], [mine], [anchor.bool()], in_place=True)[0]
    torch.cuda.synchronize()
    assert again.boxes.data_ptr() == mine.data_ptr() and np.array_equal(mine.cpu().numpy().view(np.uint32), want["out"].view(np.uint32))


@pytest.mark.parametrize("fmt", ["yuv420p", "rgb24"])
def test_end_to_end_shot_cuts_densify_follow_redact(fmt):
    from tubedetr_amd.render import anchors, color_in_space, densify, follow, redact, shot_cuts

    dev = torch.device(DEV)
    luma, true, anchor_np, _ = the_scene(E_T, E_SH, E_SW)
    luma = luma.copy()
    luma[13:] = luma[13:] // 4 + 150  # another take from frame 13 on: bright and flat
    planes, frames = _clip(luma, fmt, 91)
    rows = np.stack([true[::E_STEP], true[::E_STEP] + F32([4, 3, 4, 3])], 1)  # K = 2
    tube = torch.from_numpy(rows).to(dev)

    def stages():
        shots = shot_cuts(frames)
        dense = densify(tube, E_T, first=0, step=E_STEP, mode="lerp", shots=shots)
        anchor = anchors(first=0, step=E_STEP, T=E_T, device=dev)
        followed = follow(frames, dense, anchor, shots=shots, radius=16, reach=6, accept=(30, 1))
        return shots, followed, redact(frames, followed.boxes, mode="fill", color=(200, 90, 30))

    shots, followed, out = _no_sync(stages)
    torch.cuda.synchronize()
    hist, sad, n = frame_stats_ref(luma_of_planes(planes, fmt))
    cuts = shot_cuts_ref(hist, sad, n)
    assert np.nonzero(cuts["cut"])[0].tolist() == [13] and np.array_equal(shots.shot.cpu().numpy(), cuts["shot"])
    dense_ref = dense_floats(densify_shots_ref(rows, E_T, first=0, step=E_STEP, mode="lerp", shot=cuts["shot"]))
    want = follow_ref(luma_of_planes(planes, fmt), dense_ref, anchor_np, shot=cuts["shot"], radius=16, reach=6, accept=(30, 1))
    assert followed.boxes.shape == (E_T, 2, 4) and followed.offset.shape == (E_T, 2, 2) and followed.status.shape == (E_T, 2)
    assert np.array_equal(followed.boxes.cpu().numpy().view(np.uint32), want["out"].view(np.uint32))
    assert np.array_equal(followed.offset.cpu().numpy(), want["offset"]) and np.array_equal(followed.cost.cpu().numpy().view(np.uint32), want["cost"])
    assert np.array_equal(followed.status.cpu().numpy(), want["status"])
    blind = follow_ref(luma_of_planes(planes, fmt), dense_ref, anchor_np, radius=16, reach=6, accept=(30, 1))
    assert want["status"][13, 0] != 0 and want["cost"][13, 0] != blind["cost"][13, 0]  # frame 13 is matched against frame 18, in its own shot, not against 12
    assert (want["status"] == 1).sum() >= 10
    hidden = redact_ref(planes, fmt, boxes=want["out"], mode="fill", color=color_in_space((200, 90, 30), fmt))
    assert torch.equal(out.data.cpu(), _pack(hidden, fmt))
