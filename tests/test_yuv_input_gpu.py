"""td_clip_resample_src (yuv420p / nv12 sources of the device-side augmentation) and ClipPipeline.stage_raw with
DecodedClips on the GPU.

The claim is bit equality: a job's output is, byte for byte, what td_clip_resample produces from the rgb24 frames that the
header's integer rule (``yuv_to_rgb8``, tests/test_yuv_input_cpu.py) makes of the source.  Independently of the rgb
kernel, identity-size jobs must return ``yuv_to_rgb8`` exactly and a resized job must agree with the float64 restatement
of the sampling rule within the bound tests/test_augment_gpu.py uses for the rgb path (``_check_single`` there).

Source buffers are allocated at exactly the extent the job describes, so under the electric-fence allocator
(tests/efence) a load outside a plane faults.  Sizes are rows x columns."""
import numpy as np
import pytest
import torch

from test_augment_cpu import resample_f64
from test_augment_gpu import _check_single
from test_yuv_input_cpu import chroma_hw, yuv_to_rgb8

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
FMTS = ["yuv420p", "nv12"]


def make_planes(rng, T, sh, sw, fmt):
    ch, cw = chroma_hw(sh, sw)
    Y = rng.integers(0, 256, (T, sh, sw), dtype=np.uint8)
    if fmt == "yuv420p":
        return (Y, rng.integers(0, 256, (T, ch, cw), dtype=np.uint8), rng.integers(0, 256, (T, ch, cw), dtype=np.uint8))
    return (Y, rng.integers(0, 256, (T, ch, cw, 2), dtype=np.uint8))


def pack(planes, pitches=None, rng=None):
    """The planes as ONE flat buffer, frame after frame, plane after plane, each row at its pitch (default: tight, an
    ffmpeg rawvideo pipe).  Returns (buffer, offsets of frame 0's planes, pitches, frame stride); the buffer ends with
    the last row of the last plane (no slack), bytes between rows are random."""
    T = planes[0].shape[0]
    rows = [p.reshape(T, p.shape[1], -1) for p in planes]  # nv12's UV plane: rows of 2 cw bytes
    pitches = [r.shape[2] for r in rows] if pitches is None else list(pitches)
    offs, o = [], 0
    for r, pt in zip(rows, pitches):
        assert pt >= r.shape[2]
        offs.append(o)
        o += pt * r.shape[1]
    stride = o
    last = rows[-1]
    total = (T - 1) * stride + offs[-1] + (last.shape[1] - 1) * pitches[-1] + last.shape[2]
    buf = (rng.integers(0, 256, total + max(pitches), dtype=np.uint8) if rng is not None else np.zeros(total + max(pitches), dtype=np.uint8))
    for r, pt, off in zip(rows, pitches, offs):
        for t in range(T):
            for y in range(r.shape[1]):
                a = t * stride + off + y * pt
                buf[a : a + r.shape[2]] = r[t, y]
    return buf[:total].copy(), offs, pitches, stride


def _stage(s):
    from tubedetr_amd.augment import ResampleStage

    return ResampleStage(s["rh"], s["rw"], *(s.get("window") or (0, 0, s["rh"], s["rw"])))


def run(specs, pad=(0, 0), entry="src"):
    """ONE launch.  spec: fmt ("yuv420p" | "nv12" | "rgb24"), rh, rw, window | None, flip, planar, and the source: ``planes``
    (+ optional ``pitches``, matrix, full_range) or, for rgb24, ``src`` (T, sh, sw, 3).  entry "src": td_clip_resample_src;
    "rgb": td_clip_resample (rgb24 specs only).  Returns per spec the produced pixels (T, wh, ww, 3) and, for planar jobs,
    the padded frames + mask.  Destinations are pre-filled, so an unwritten byte shows."""
    from tubedetr_amd.augment import clip_resample, clip_resample_src, resample_job, resample_src_job

    dev = torch.device(DEV)
    stages = [_stage(s) for s in specs]
    planar = [i for i, s in enumerate(specs) if s.get("planar")]
    H = max([stages[i].wh for i in planar], default=0) + pad[0]
    W = max([stages[i].ww for i in planar], default=0) + pad[1]
    n = sum((specs[i]["src"] if specs[i]["fmt"] == "rgb24" else specs[i]["planes"][0]).shape[0] for i in planar)
    video = torch.full((max(n, 1), 3, max(H, 1), max(W, 1)), 77, dtype=torch.uint8, device=dev)
    mask = torch.full((max(n, 1), max(H, 1), max(W, 1)), 9, dtype=torch.uint8, device=dev)
    jobs, keep, outs, off = [], [], [], 0
    for s, st in zip(specs, stages):
        kw = {}
        if s["fmt"] == "rgb24":
            T, sh, sw, _ = s["src"].shape
            src = torch.from_numpy(np.ascontiguousarray(s["src"]).reshape(-1)).to(dev)
        else:
            T, sh, sw = s["planes"][0].shape
            buf, offs, pitches, stride = pack(s["planes"], s.get("pitches"), np.random.default_rng(1))
            src = torch.from_numpy(buf).to(dev)
            if s.get("pitches") is not None:
                kw = {"planes": [src.data_ptr() + o for o in offs], "pitches": pitches, "frame_stride": stride}
        keep.append(src)
        if s.get("planar"):
            dst, dkw = video.data_ptr(), {"planar": True, "frame_off": off, "H": H, "W": W, "mask": mask.data_ptr()}
            outs.append(("planar", off, T, st))
            off += T
        else:
            d = torch.full((T, st.wh, st.ww, 3), 55, dtype=torch.uint8, device=dev)
            dst, dkw = d.data_ptr(), {}
            outs.append(("inter", d))
        if entry == "rgb":
            assert s["fmt"] == "rgb24"
            jobs.append(resample_job(src.data_ptr(), T, sh, sw, s.get("flip", False), st, dst, **dkw))
        else:
            jobs.append(resample_src_job(src.data_ptr(), T, sh, sw, s.get("flip", False), st, dst, s["fmt"], s.get("matrix", "bt601"), s.get("full_range", False), **dkw, **kw))
    tables = (clip_resample if entry == "rgb" else clip_resample_src)(jobs, dev)
    torch.cuda.synchronize()
    del tables
    res = []
    v, m = video.cpu().numpy(), mask.cpu().numpy()
    for o in outs:
        if o[0] == "inter":
            res.append({"pixels": o[1].cpu().numpy()})
        else:
            _, off, T, st = o
            fr, mk = v[off : off + T], m[off : off + T]
            res.append({"pixels": fr[:, :, : st.wh, : st.ww].transpose(0, 2, 3, 1), "frames": fr, "mask": mk, "hw": (st.wh, st.ww)})
    return res


def check_padding(r):
    wh, ww = r["hw"]
    want_mask = np.ones(r["mask"].shape[1:], dtype=np.uint8)
    want_mask[:wh, :ww] = 0
    assert (r["mask"] == want_mask[None]).all()
    assert (r["frames"][:, :, wh:, :] == 0).all() and (r["frames"][:, :, :, ww:] == 0).all()


def first_tap(v, n_src, n_dst):
    num = (2 * v + 1) * n_src - n_dst
    return num // (2 * n_dst) if num > 0 else 0


def cmin_of(sw, rw, wx, ww, flip):
    """First source column the window's staging reads (csrc/augment.hip: the first tap of the first column, mirrored under flip)."""
    c_lo, c_hi = first_tap(wx, sw, rw), min(first_tap(wx + ww - 1, sw, rw) + 1, sw - 1)
    return sw - 1 - c_hi if flip else c_lo


# (source rows x columns, T, [(rh, rw, window | None), ...])
CASES = {
    "even-baseline": ((36, 64), 2, [(33, 58, None)]),
    # odd sides: odd pitches, so Y rows and plane starts are not dword-aligned; odd frame stride; two frame chunks
    "odd-sides": ((37, 51), 5, [(45, 62, None)]),
    # a window of a virtual image.  wx = 77 (cmin 6, under flip 34: both even) and wx = 88, whose cmin is odd (asserted)
    "window": ((37, 51), 2, [(300, 533, (101, 77, 40, 90)), (300, 533, (101, 88, 40, 90))]),
    # rgb24's wide-row fallback (more than 1365 source pixels of a row staged)
    "wide-row": ((6, 1500), 1, [(6, 1500, None), (5, 1400, None)]),
    "minify": ((9, 9), 9, [(4, 4, None)]),  # rows skip chroma rows
    "degenerate-2x3": ((2, 3), 1, [(5, 7, None)]),
    "degenerate-1x1": ((1, 1), 1, [(5, 7, None)]),
    # the Y staging's own wide-row fallback (more than 2045 source pixels of a row staged), not in the issue's table
    "wide-y-row": ((3, 2100), 1, [(3, 2100, None), (2, 1900, None)]),
}


@pytest.mark.parametrize("planar", [False, True], ids=["interleaved", "planar"])
@pytest.mark.parametrize("flip", [False, True], ids=["noflip", "flip"])
@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("case", list(CASES))
def test_bit_equal_to_the_rgb24_path(case, fmt, flip, planar):
    (sh, sw), T, targets = CASES[case]
    rng = np.random.default_rng(sum(map(ord, case)) + 2 * flip + planar)
    planes = make_planes(rng, T, sh, sw, fmt)
    rgb = yuv_to_rgb8(planes, fmt)
    if case == "window":
        assert cmin_of(sw, 533, 88, 90, flip) % 2 == 1, "the second window must start its staging at an odd source column"
    for rh, rw, win in targets:
        geo = {"rh": rh, "rw": rw, "window": win, "flip": flip, "planar": planar}
        pad = (3, 5) if planar else (0, 0)
        (got,) = run([dict(geo, fmt=fmt, planes=planes)], pad)
        (want,) = run([dict(geo, fmt="rgb24", src=rgb)], pad, entry="rgb")
        assert got["pixels"].shape == want["pixels"].shape
        assert np.array_equal(got["pixels"], want["pixels"]), f"{case} {fmt} -> {rh}x{rw} {win}: {(got['pixels'] != want['pixels']).sum()} bytes differ"
        if planar:
            assert np.array_equal(got["frames"], want["frames"]) and np.array_equal(got["mask"], want["mask"])
            check_padding(got)


@pytest.mark.parametrize("full_range", [False, True], ids=["limited", "full"])
@pytest.mark.parametrize("matrix", ["bt601", "bt709"])
@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("hw", [(37, 51), (36, 64)])
def test_identity_size_returns_the_converted_frames(hw, fmt, matrix, full_range):
    """rh x rw = sh x sw is an exact copy, so the output IS the conversion: no rgb kernel involved.  Non-tight pitches."""
    sh, sw = hw
    ch, cw = chroma_hw(sh, sw)
    rng = np.random.default_rng(sh + 3 * (matrix == "bt709") + 5 * full_range)
    planes = make_planes(rng, 3, sh, sw, fmt)
    pitches = [sw + 5, cw + 3, cw + 3] if fmt == "yuv420p" else [sw + 5, 2 * cw + 3]
    want = yuv_to_rgb8(planes, fmt, matrix, full_range)
    base = {"fmt": fmt, "planes": planes, "pitches": pitches, "matrix": matrix, "full_range": full_range, "rh": sh, "rw": sw}
    a, b, c = run([base, dict(base, planar=True), dict(base, flip=True)], pad=(2, 3))
    assert np.array_equal(a["pixels"], want) and np.array_equal(b["pixels"], want) and np.array_equal(c["pixels"], want[:, :, ::-1])
    check_padding(b)


@pytest.mark.parametrize("fmt", FMTS)
def test_resized_job_matches_the_float64_restatement(fmt):
    rng = np.random.default_rng(11)
    planes = make_planes(rng, 2, 37, 51, fmt)
    rgb = yuv_to_rgb8(planes, fmt, "bt709", False)
    for flip in (False, True):
        (r,) = run([{"fmt": fmt, "planes": planes, "matrix": "bt709", "rh": 45, "rw": 62, "flip": flip, "planar": True}], pad=(1, 2))
        _check_single(r["pixels"], resample_f64(rgb, 45, 62, None, flip), f"{fmt} 37x51->45x62 flip={flip}")
        check_padding(r)


def test_one_launch_with_mixed_formats():
    rng = np.random.default_rng(12)
    specs = [
        {"fmt": "yuv420p", "planes": make_planes(rng, 5, 37, 51, "yuv420p"), "rh": 45, "rw": 62, "flip": True, "planar": True},
        {"fmt": "nv12", "planes": make_planes(rng, 2, 36, 64, "nv12"), "matrix": "bt709", "full_range": True, "rh": 33, "rw": 58, "window": (2, 3, 30, 50)},
        {"fmt": "rgb24", "src": rng.integers(0, 256, (3, 40, 40, 3), dtype=np.uint8), "rh": 44, "rw": 47, "planar": True},
    ]
    together = run(specs, pad=(2, 1))
    H, W = 45 + 2, 62 + 1
    for s, r in zip(specs, together):
        (alone,) = run([s], pad=(H - _stage(s).wh, W - _stage(s).ww) if s.get("planar") else (0, 0))
        assert np.array_equal(r["pixels"], alone["pixels"])
        if s.get("planar"):
            assert np.array_equal(r["frames"], alone["frames"]) and np.array_equal(r["mask"], alone["mask"])
            check_padding(r)
    # the rgb24 job of td_clip_resample_src is td_clip_resample's
    (old,) = run([specs[2]], pad=(H - 44, W - 47), entry="rgb")
    assert np.array_equal(together[2]["frames"], old["frames"]) and np.array_equal(together[2]["mask"], old["mask"])


def _plan(flip, stages, T, src_hw):
    from tubedetr_amd.augment import ClipPlan, ResampleStage

    st = [ResampleStage(*s) for s in stages]
    hw = (st[-1].wh, st[-1].ww)
    targets = [{"boxes": torch.tensor([[0.5, 0.5, 0.2 + 0.01 * t, 0.3]]), "size": torch.tensor(hw), "orig_size": torch.tensor(src_hw)} for t in range(T)]
    return ClipPlan(flip, st, hw, targets, "a caption", 0, src_hw)


TICKET_TENSORS = ("video", "mask", "valid_hw", "slow_index", "target_boxes", "input_ids", "attention_mask")
TICKET_VALUES = ("durations", "inter_idx", "n_slow", "slow_index_host")


def test_stage_raw_with_decoded_clips_equals_stage_raw_with_host_converted_rgb():
    from tubedetr_amd.augment import DecodedClip
    from tubedetr_amd.data import ClipPipeline

    dev = torch.device(DEV)
    rng = np.random.default_rng(13)
    pa, pb = make_planes(rng, 3, 37, 51, "yuv420p"), make_planes(rng, 4, 36, 64, "nv12")
    rgb_c = rng.integers(0, 256, (5, 40, 40, 3), dtype=np.uint8)
    buf_a, buf_b = pack(pa)[0], pack(pb)[0]
    clips = [DecodedClip(buf_a, 3, 37, 51, "yuv420p"), DecodedClip(torch.from_numpy(buf_b), 4, 36, 64, "nv12", matrix="bt709", full_range=True), rgb_c]
    host_rgb = [yuv_to_rgb8(pa, "yuv420p"), yuv_to_rgb8(pb, "nv12", "bt709", True), rgb_c]
    plans = [
        _plan(True, [(45, 62, 3, 4, 40, 50), (48, 60, 0, 0, 48, 60)], 3, (37, 51)),  # training: resize + crop, second resize; flip
        _plan(False, [(33, 58, 0, 0, 33, 58)], 4, (36, 64)),                          # evaluation: one resize
        _plan(False, [(44, 44, 0, 0, 44, 44)], 5, (40, 40)),
    ]
    ids = torch.randint(3, 50000, (3, 5))
    att = torch.ones(3, 5, dtype=torch.long)
    inter = [[0, 2], [0, 3], [0, 4]]
    pipe = ClipPipeline(dev, 2)
    tk = pipe.stage_raw(clips, plans, ids, att, inter)
    # what was packed into page-locked memory: T * nbytes_per_frame per clip, each clip at the next multiple of 16
    na, nb_ = 3 * clips[0].nbytes_per_frame, 4 * clips[1].nbytes_per_frame
    assert (na, nb_) == (3 * (37 * 51 + 2 * 19 * 26), 4 * (36 * 64 + 2 * 18 * 32)) == (buf_a.size, buf_b.size)
    r16 = lambda v: (v + 15) // 16 * 16  # noqa: E731
    pinned = pipe._raw_slots[0][0]
    assert pinned.numel() == r16(na) + r16(nb_) + r16(rgb_c.size), "the yuv clips are staged at 1.5 bytes per pixel"
    torch.cuda.synchronize()
    assert np.array_equal(pinned[:na].numpy(), buf_a) and np.array_equal(pinned[r16(na) : r16(na) + nb_].numpy(), buf_b)
    ref_pipe = ClipPipeline(dev, 2)
    tk2 = ref_pipe.stage_raw(host_rgb, plans, ids, att, inter)
    assert ref_pipe._raw_slots[0][0].numel() == r16(3 * 37 * 51 * 3) + r16(4 * 36 * 64 * 3) + r16(rgb_c.size)
    batch, batch2 = pipe.collect(tk), ref_pipe.collect(tk2)
    torch.cuda.synchronize()
    assert tk["video"].shape == (12, 3, 48, 60) and tk["valid_hw"] is not None
    for key in TICKET_TENSORS:
        assert tk[key].dtype == tk2[key].dtype and tk[key].shape == tk2[key].shape, key
        assert torch.equal(tk[key].cpu(), tk2[key].cpu()), key
    for key in TICKET_VALUES:
        assert tk[key] == tk2[key], key
    assert set(tk) == set(tk2) == set(TICKET_TENSORS) | set(TICKET_VALUES) | {"event"}
    assert tk["slow_index_host"] == (0, 2, 3, 5, 7, 9, 11)
    assert set(batch) == set(batch2)
    assert torch.equal(batch["frames_mask"].cpu(), batch2["frames_mask"].cpu()) and torch.equal(batch["fast_mask"].cpu(), batch2["fast_mask"].cpu())
    # and not vacuously: clip A's frames are the two-stage resample of its converted frames (uint8 in between)
    video = tk["video"].cpu().numpy()
    assert video[:3, :, :48, :60].std() > 10 and not tk["mask"][:3, :48, :60].any().item()


def test_all_rgb24_stage_raw_is_td_clip_resample_of_the_same_jobs():
    from tubedetr_amd.data import ClipPipeline

    dev = torch.device(DEV)
    rng = np.random.default_rng(14)
    raws = [rng.integers(0, 256, (3, 37, 51, 3), dtype=np.uint8), rng.integers(0, 256, (2, 40, 40, 3), dtype=np.uint8)]
    plans = [_plan(True, [(45, 62, 3, 4, 40, 50), (48, 60, 0, 0, 48, 60)], 3, (37, 51)), _plan(False, [(44, 44, 0, 0, 44, 44)], 2, (40, 40))]
    pipe = ClipPipeline(dev, 2)
    tk = pipe.stage_raw(raws, plans, torch.zeros(2, 5, dtype=torch.long), torch.ones(2, 5, dtype=torch.long), [[0, 2], [0, 1]])
    torch.cuda.synchronize()
    (mid,) = run([{"fmt": "rgb24", "src": raws[0], "rh": 45, "rw": 62, "window": (3, 4, 40, 50), "flip": True}], entry="rgb")
    a, b = run([{"fmt": "rgb24", "src": mid["pixels"], "rh": 48, "rw": 60, "planar": True}, {"fmt": "rgb24", "src": raws[1], "rh": 44, "rw": 44, "planar": True}], entry="rgb")
    assert np.array_equal(tk["video"].cpu().numpy(), np.concatenate([a["frames"], b["frames"]]))
    assert np.array_equal(tk["mask"].cpu().numpy().astype(np.uint8), np.concatenate([a["mask"], b["mask"]]))
