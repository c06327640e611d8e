"""td_tube_crop and render.crop_tubes on the GPU.

The claim is bit equality with entry points that already exist: the window of every frame comes from the numpy restatement of
the rule (tests/tube_crop_ref.py), and the expected bytes from ONE td_clip_resample launch of one-frame planar jobs on the
sub-images (addressed by a source offset, src_pitch = the frame's pitch) of the rgb24 frames - for yuv420p / nv12 the frames the
header's integer rule makes of the source on the host (``yuv_to_rgb8``).  Pixels, mask, valid and windows are compared with
np.array_equal; every output buffer sits between canary bytes, at byte offsets that give the frames every dword alignment.
One test compares with the float64 restatement of the sampling rule instead of with a kernel.

Source buffers are allocated at exactly the extent the job describes, so under the electric-fence allocator (tests/efence) a
load outside a plane faults.  Sizes are rows x columns."""
import numpy as np
import pytest
import torch

from test_augment_cpu import resample_f64
from test_augment_gpu import _check_single
from test_tube_crop_cpu import F64_CASES, f64_frames
from test_yuv_input_cpu import yuv_to_rgb8
from test_yuv_input_gpu import make_planes, pack
from tube_crop_ref import compose, tube_windows

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
FMTS = ["rgb24", "yuv420p", "nv12"]
CANARY, FILL = 0xA5, 0x4D


def frames_of(rng, T, sh, sw, fmt):
    """A source in ``fmt``: for rgb24 the (T, sh, sw, 3) array, else the planes."""
    if fmt == "rgb24":
        return rng.integers(0, 256, (T, sh, sw, 3), dtype=np.uint8)
    return make_planes(rng, T, sh, sw, fmt)


def rgb_of(spec):
    if spec["fmt"] == "rgb24":
        return spec["src"]
    return yuv_to_rgb8(spec["src"], spec["fmt"], spec.get("matrix", "bt601"), spec.get("full_range", False))


def geometry(spec):
    src = spec["src"]
    T, sh, sw = (src.shape[:3] if spec["fmt"] == "rgb24" else src[0].shape)
    return T, sh, sw


class Guarded:
    """A device buffer of n bytes between two runs of canary bytes, starting ``lead`` bytes into its allocation."""

    def __init__(self, n, lead, dev):
        self.n, self.lead = n, lead
        self.buf = torch.full((lead + n + 64,), CANARY, dtype=torch.uint8, device=dev)
        self.buf[lead : lead + n] = FILL

    def ptr(self):
        return self.buf.data_ptr() + self.lead

    def read(self):
        b = self.buf.cpu().numpy()
        assert (b[: self.lead] == CANARY).all() and (b[self.lead + self.n :] == CANARY).all(), "bytes outside an output buffer were written"
        return b[self.lead : self.lead + self.n]


def reference(specs, dev):
    """Per spec (valid, windows, pixels, mask) by the rule's restatement + one td_clip_resample launch for all sub-images."""
    from tubedetr_amd.augment import ResampleStage, clip_resample, resample_job

    jobs, keep, metas = [], [], []
    for s in specs:
        T, sh, sw = geometry(s)
        oh, ow = s["size"]
        valid, windows = tube_windows(s["boxes"], T, sh, sw, oh, ow, s.get("span"), s.get("frame_map"), s.get("margin", (0, 1)), s.get("keep_aspect", True))
        rgb = np.ascontiguousarray(rgb_of(s))
        src = torch.from_numpy(rgb.reshape(-1)).to(dev)
        video = torch.full((T, 3, oh, ow), 77, dtype=torch.uint8, device=dev)
        mask = torch.full((T, oh, ow), 9, dtype=torch.uint8, device=dev)
        keep.append(src)
        for t in range(T):
            wy0, wx0, ch, cw, rh, rw = (int(v) for v in windows[t])
            if rh:
                jobs.append(resample_job(src.data_ptr() + ((t * sh + wy0) * sw + wx0) * 3, 1, ch, cw, False, ResampleStage(rh, rw, 0, 0, rh, rw), video.data_ptr(),
                                         planar=True, frame_off=t, H=oh, W=ow, mask=mask.data_ptr(), src_pitch=3 * sw, src_frame_stride=3 * sw * sh))
        metas.append((valid, windows, video, mask, rgb))
    tables = clip_resample(jobs, dev) if jobs else None
    torch.cuda.synchronize()
    del tables
    out = []
    for valid, windows, video, mask, rgb in metas:
        v, m = video.cpu().numpy(), mask.cpu().numpy()
        oh, ow = m.shape[1:]
        pixels, pad = compose(rgb, windows, oh, ow, lambda t, sub, rh, rw: np.ascontiguousarray(v[t, :, :rh, :rw].transpose(1, 2, 0)))
        assert np.array_equal(pixels[valid], v[valid]) and np.array_equal(pad[valid], m[valid]), "td_clip_resample's own padding is the composer's"
        out.append((valid, windows, pixels, pad))  # an empty frame had no job: zeros and mask 1 (step 9)
    return out


def run(specs, outputs=("mask", "valid", "windows")):
    """ONE td_tube_crop launch.  spec: fmt, src (``frames_of``), boxes (n, 4), size, and optionally span, frame_map, margin,
    keep_aspect, matrix, full_range, pitches (planes with gaps).  Returns per spec (valid, windows, pixels, mask) as numpy
    arrays (None for an output that was left out), canaries checked."""
    from tubedetr_amd.render import crop_job, tube_crop

    dev = torch.device(DEV)
    jobs, keep, outs = [], [], []
    for i, s in enumerate(specs):
        T, sh, sw = geometry(s)
        oh, ow = s["size"]
        planes = [s["src"].reshape(T, sh, 3 * sw)] if s["fmt"] == "rgb24" else list(s["src"])
        buf, offs, pitches, stride = pack(planes, s.get("pitches"), np.random.default_rng(1))
        src = torch.from_numpy(buf).to(dev)
        boxes = torch.from_numpy(np.asarray(s["boxes"], dtype=np.float32).reshape(-1, 4).copy()).to(dev)
        span = torch.tensor(s["span"], dtype=torch.int64, device=dev) if s.get("span") is not None else None
        fmap = torch.tensor(s["frame_map"], dtype=torch.int32, device=dev) if s.get("frame_map") is not None else None
        keep += [src, boxes, span, fmap]
        # leads 61 + i, 63 + i, ...: frames (3 oh ow bytes apart) and rows start at every dword alignment over the specs of a launch
        o = {"pixels": Guarded(T * 3 * oh * ow, 61 + i, dev), "mask": Guarded(T * oh * ow, 63 + i, dev) if "mask" in outputs else None,
             "valid": Guarded(T, 62 + i, dev) if "valid" in outputs else None, "windows": Guarded(T * 24, 64, dev) if "windows" in outputs else None}
        kw = {}
        if s.get("pitches") is not None:
            kw = {"planes": [src.data_ptr() + a for a in offs], "pitches": pitches, "frame_stride": stride}
        jobs.append(crop_job(src.data_ptr(), T, sh, sw, boxes.data_ptr(), boxes.shape[0], o["pixels"].ptr(), (oh, ow), s["fmt"], s.get("matrix", "bt601"),
                             s.get("full_range", False), span.data_ptr() if span is not None else None, fmap.data_ptr() if fmap is not None else None,
                             s.get("margin", (0, 1)), s.get("keep_aspect", True), *(o[k].ptr() if o[k] is not None else None for k in ("mask", "valid", "windows")), **kw))
        outs.append((o, T, oh, ow, src, buf))
    tables = tube_crop(jobs, dev)
    torch.cuda.synchronize()
    del tables
    res = []
    for o, T, oh, ow, src, buf in outs:
        assert np.array_equal(src.cpu().numpy(), buf), "the source was written"
        res.append((o["valid"].read().copy() if o["valid"] else None, o["windows"].read().copy().view(np.int32).reshape(T, 6) if o["windows"] else None,
                    o["pixels"].read().reshape(T, 3, oh, ow).copy(), o["mask"].read().reshape(T, oh, ow).copy() if o["mask"] else None))
    return res


def check(specs, outputs=("mask", "valid", "windows")):
    """Run the launch and the reference; everything equal, byte for byte.  Returns the reference's (valid, windows, pixels, mask) per spec."""
    got, want = run(specs, outputs), reference(specs, torch.device(DEV))
    for i, ((gv, gw, gp, gm), (wv, ww, wp, wm)) in enumerate(zip(got, want)):
        assert gw is None or np.array_equal(gw, ww), (i, gw, ww)
        assert gv is None or np.array_equal(gv, wv.astype(np.uint8)), (i, gv, wv)
        assert gm is None or np.array_equal(gm, wm), i
        assert np.array_equal(gp, wp), (i, np.argwhere(gp != wp)[:5])
    return want


def kinds_of_boxes(sh, sw):
    inf, nan = np.inf, np.nan
    return np.array([
        [1.0, 1.0, sw - 1.0, sh - 1.0],                     # inside, odd (wy0, wx0)
        [2.0, 2.0, float(sw), float(sh)],                   # even (wy0, wx0)
        [1.0, 2.0, sw - 2.0, sh - 1.0],                     # mixed parity
        [-3.4, sh * 0.3, sw * 0.5, sh * 0.9],               # across the left edge
        [sw * 0.3, -2.5, sw * 0.8, sh * 0.5],               # the top edge
        [sw * 0.5, sh * 0.2, sw + 4.2, sh * 0.8],           # the right edge
        [sw * 0.2, sh * 0.5, sw * 0.7, sh + 2.5],           # the bottom edge
        [sw + 1.0, 1.0, sw + 9.0, sh - 1.0],                # wholly outside
        [sw - 3.0, sh - 2.0, sw - 2.0, sh - 1.0],           # 1 x 1
        [0.0, 0.0, float(sw), float(sh)],                   # the whole frame
        [nan, 1.0, 3.0, 3.0],
        [1.0, 1.0, inf, 3.0],
        [1.0, -inf, 3.0, 3.0],
        [2.0, 1.0, 2.3, sh - 1.0],                          # x1 == x0 after rounding
        [-1e30, -1e30, 1e30, 1e30],                         # finite: clamped to +-2^20, the whole frame
    ], dtype=np.float32)


SIZES = [(5, 7), (37, 51), (64, 96)]
OUT_SIZES = [(1, 1), (5, 7), (16, 16), (33, 17)]


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_formats_sizes_and_every_kind_of_box(size, fmt):
    sh, sw = size
    T = 5  # two frame chunks
    boxes = kinds_of_boxes(sh, sw)
    src = frames_of(np.random.default_rng(20), T, sh, sw, fmt)
    specs = []
    for first in range(0, len(boxes), T):  # five tube rows per job: every frame of the clip meets every kind of box over the jobs
        for keep in (False, True):
            for out in OUT_SIZES:
                specs.append(dict(fmt=fmt, src=src, boxes=boxes, frame_map=list(range(first, first + T)), size=out, keep_aspect=keep))
    want = check(specs)
    valid = np.concatenate([w[0] for w in want[:: 2 * len(OUT_SIZES)]])
    assert valid.tolist() == [True] * 7 + [False] + [True] * 2 + [False] * 4 + [True]
    wins = np.concatenate([w[1] for w in want[:: 2 * len(OUT_SIZES)]])[valid]
    assert {(int(a) & 1, int(b) & 1) for a, b in wins[:, :2]} == {(0, 0), (0, 1), (1, 0), (1, 1)}, "chroma parity of the window's origin"
    assert any((w[1][w[0], 4] < s["size"][0]).any() for w, s in zip(want, specs)) and any((w[1][w[0], 5] < s["size"][1]).any() for w, s in zip(want, specs)), "keep_aspect pads both ways"


@pytest.mark.parametrize("fmt", FMTS)
def test_margins(fmt):
    sh, sw, T = 37, 51, 5
    rng = np.random.default_rng(21)
    src = frames_of(rng, T, sh, sw, fmt)
    boxes = np.array([[20, 15, 30, 22], [10.4, 5.5, 30.6, 20.49], [0, 0, 9, 7], [44, 30, 51, 37], [25, 18, 26, 19]], dtype=np.float32)
    specs = [dict(fmt=fmt, src=src, boxes=boxes, size=(16, 16), margin=m, keep_aspect=k) for m in ((0, 1), (1, 4), (1, 1), (4, 1), (3, 1024)) for k in (True, False)]
    want = check(specs)
    assert want[2][1][1].tolist() == [3, 5, 20, 31, 10, 16]  # the case worked by hand in tests/test_tube_crop_cpu.py
    assert want[6][1][0].tolist() == [0, 0, 37, 51, 12, 16]  # 4/1 around a box in the middle: the whole frame, (2 * 37 * 16 + 51) / 102 = 12


@pytest.mark.parametrize("fmt", FMTS)
def test_span_and_frame_map(fmt):
    sh, sw = 37, 53
    rng = np.random.default_rng(22)
    boxes = np.stack([[3 + r, 2 + r, 30 + 2 * r, 20 + 3 * r] for r in range(5)]).astype(np.float32)
    src5 = frames_of(rng, 5, sh, sw, fmt)
    fmap = [0, 0, 0, 1, 1, 1, 2, 2, 2, 3]  # three frames per tube row; row 3 of 3 does not exist
    src10 = frames_of(rng, len(fmap), sh, sw, fmt)
    specs = [dict(fmt=fmt, src=src5, boxes=boxes, span=span, size=(9, 12)) for span in (None, (1, 3), (2, 2), (4, 9), (-3, 0), (3, 1))]
    specs += [dict(fmt=fmt, src=src10, boxes=boxes[:3], frame_map=fmap, span=span, size=(9, 12)) for span in (None, (1, 2))]
    specs.append(dict(fmt=fmt, src=src10, boxes=boxes[:3], frame_map=[2, -1, 0, 1, 2, 0, 1, 2, 0, 7], size=(9, 12)))
    want = check(specs)
    assert [w[0].tolist() for w in want[:6]] == [[True] * 5, [False, True, True, True, False], [False, False, True, False, False], [False] * 4 + [True], [True] + [False] * 4, [False] * 5]
    assert want[6][0].tolist() == [True] * 9 + [False] and want[7][0].tolist() == [False] * 3 + [True] * 6 + [False]
    assert want[8][0].tolist() == [True, False] + [True] * 7 + [False]


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("size", SIZES + [(16, 24)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_identity_returns_the_converted_frame(size, fmt):
    sh, sw = size
    T = 3
    src = frames_of(np.random.default_rng(23), T, sh, sw, fmt)
    spec = dict(fmt=fmt, src=src, boxes=np.array([[0, 0, sw, sh]] * T, dtype=np.float32), size=(sh, sw), keep_aspect=False, matrix="bt709", full_range=True)
    ((valid, windows, pixels, mask),) = run([spec])
    assert valid.all() and not mask.any() and (windows == [0, 0, sh, sw, sh, sw]).all()
    assert np.array_equal(pixels.transpose(0, 2, 3, 1), rgb_of(spec))
    check([spec])


@pytest.mark.parametrize("fmt,sw", [("rgb24", 1400), ("yuv420p", 2100), ("nv12", 2100), ("rgb24", 2100)])
def test_source_rows_past_the_in_register_staging_depth(fmt, sw):
    sh = 6
    src = frames_of(np.random.default_rng(24), 1, sh, sw, fmt)
    full, narrow = [[0, 0, sw, sh]], [[sw - 40.0, 1, sw - 3.0, 5]]
    check([dict(fmt=fmt, src=src, boxes=np.array(b, dtype=np.float32), size=out, keep_aspect=k)
           for b in (full, narrow) for out, k in (((6, 1500), False), ((5, 333), False), ((4, 40), True))])


@pytest.mark.parametrize("fmt", FMTS)
def test_pitched_planes(fmt):
    sh, sw, T = 37, 51, 5
    rng = np.random.default_rng(25)
    src = frames_of(rng, T, sh, sw, fmt)
    pitches = {"rgb24": [3 * sw + 7], "yuv420p": [sw + 5, 26 + 3, 26 + 6], "nv12": [sw + 2, 52 + 9]}[fmt]
    boxes = kinds_of_boxes(sh, sw)[[0, 1, 3, 5, 9]]
    want = check([dict(fmt=fmt, src=src, pitches=pitches, boxes=boxes, size=out, margin=(1, 4)) for out in ((16, 16), (33, 17))])  # run() checks that the gaps are untouched
    tight = check([dict(fmt=fmt, src=src, boxes=boxes, size=out, margin=(1, 4)) for out in ((16, 16), (33, 17))])
    assert all(np.array_equal(a[2], b[2]) for a, b in zip(want, tight))


def test_several_jobs_in_one_launch_and_outputs_left_out():
    rng = np.random.default_rng(26)
    specs = []
    for fmt, (sh, sw), T in zip(FMTS, [(37, 53), (64, 96), (5, 7)], (5, 2, 9)):
        boxes = np.stack([[sw * 0.1 + r % 3, sh * 0.2, sw * 0.8, sh * 0.9 - r % 2] for r in range(T)]).astype(np.float32)
        specs.append(dict(fmt=fmt, src=frames_of(rng, T, sh, sw, fmt), boxes=boxes, span=(1, T - 1), size=(16, 16) if fmt != "nv12" else (5, 7), margin=(1, 4)))
    # two tubes on the same frames (one clip, two sentences)
    specs.append(dict(specs[0], boxes=np.array([[30, 10, 50, 30]] * 5, dtype=np.float32), span=(0, 2), keep_aspect=False))
    together = check(specs)
    for s, t in zip(specs, together):
        (alone,) = check([s])
        assert all(np.array_equal(a, b) for a, b in zip(alone, t))
    assert not np.array_equal(together[0][2], together[3][2])
    for outputs in ((), ("valid",), ("mask", "windows")):  # NULL leaves an output out
        check(specs[:2], outputs)


@pytest.mark.parametrize("name", list(F64_CASES))
def test_crop_matches_the_float64_restatement(name):
    """The check that does not compare kernel with kernel.  Bound and near-tie cap are _check_single's (tests/test_augment_gpu.py);
    that the inputs meet the cap is asserted in tests/test_tube_crop_cpu.py."""
    (sh, sw), box, (oh, ow), window, _ = F64_CASES[name]
    src = f64_frames(name)
    ((valid, windows, pixels, mask),) = run([dict(fmt="rgb24", src=src, boxes=np.array([box] * 2, dtype=np.float32), size=(oh, ow), keep_aspect=False)])
    assert valid.all() and not mask.any() and (windows == window).all()
    wy0, wx0, ch, cw, rh, rw = window
    _check_single(pixels.transpose(0, 2, 3, 1), resample_f64(src[:, wy0 : wy0 + ch, wx0 : wx0 + cw], rh, rw), f"crop {name} {ch}x{cw}->{rh}x{rw}")


def test_end_to_end_model_postprocess_crop_tubes():
    """T = 6, res 64, k = 2 on the synthetic model: forward under no_grad, PostProcess, sted_decode and crop_tubes on a yuv420p
    DecodedClip without a synchronisation; valid equals span membership, pixels equal the composed reference."""
    import tubedetr_amd
    from oracle.tubedetr_oracle import OracleConfig
    from oracle.weights import fill_state, state_spec, synthetic_batch
    from tubedetr_amd.augment import DecodedClip
    from tubedetr_amd.harness import FixedTokenizer, batch_to
    from tubedetr_amd.models import build_model
    from tubedetr_amd.models.postprocessors import PostProcess, sted_decode
    from tubedetr_amd.render import DeviceFrames, TubeCrops, crop_tubes
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
    rng = np.random.default_rng(27)
    Y, U, V = make_planes(rng, T, sh, sw, "yuv420p")
    packed = np.concatenate([np.concatenate([Y[t].ravel(), U[t].ravel(), V[t].ravel()]) for t in range(T)])
    frames = DeviceFrames.from_decoded(DecodedClip(packed, T, sh, sw, "yuv420p", matrix="bt709"), dev)
    wide = torch.tensor([[-5.0, -5.0, sw + 5.0, sh + 5.0]] * T, device=dev)
    torch.cuda.synchronize()
    mode = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")  # crop_tubes must not synchronise
    try:
        one = crop_tubes(frames, boxes, span=span, size=(24, 32), margin=(1, 4))
        two = crop_tubes([frames, frames], [boxes, wide], span=[span, None], size=(24, 32), margin=(1, 4), keep_aspect=False)
    finally:
        torch.cuda.set_sync_debug_mode(mode)
    torch.cuda.synchronize()
    assert isinstance(one, TubeCrops) and isinstance(two, list) and len(two) == 2
    assert one.pixels.shape == (T, 3, 24, 32) and one.pixels.dtype == torch.uint8 and one.mask.shape == (T, 24, 32) and one.mask.dtype == torch.bool
    assert one.valid.shape == (T,) and one.valid.dtype == torch.bool and one.windows.shape == (T, 6) and one.windows.dtype == torch.int32
    s0, s1 = span.cpu().tolist()
    b = boxes.cpu().numpy()
    specs = [dict(fmt="yuv420p", src=(Y, U, V), matrix="bt709", boxes=b, span=(s0, s1), size=(24, 32), margin=(1, 4)),
             dict(fmt="yuv420p", src=(Y, U, V), matrix="bt709", boxes=b, span=(s0, s1), size=(24, 32), margin=(1, 4), keep_aspect=False),
             dict(fmt="yuv420p", src=(Y, U, V), matrix="bt709", boxes=wide.cpu().numpy(), size=(24, 32), margin=(1, 4), keep_aspect=False)]
    want = reference(specs, dev)
    assert tube_windows(b, T, sh, sw, 24, 32, None, None, (1, 4))[0].all(), "the synthetic model's boxes have area: valid is span membership"
    assert one.valid.cpu().tolist() == [s0 <= t <= s1 for t in range(T)] and any(one.valid.cpu().tolist())
    for got, (valid, windows, pixels, mask) in zip([one] + two, want):
        assert np.array_equal(got.valid.cpu().numpy(), valid) and np.array_equal(got.windows.cpu().numpy(), windows)
        assert np.array_equal(got.pixels.cpu().numpy(), pixels) and np.array_equal(got.mask.cpu().numpy(), mask.astype(bool))
    # the composed reference with the float-free resizer of an identity-size crop: the whole frame at its own size is the converted frame
    whole = crop_tubes(frames, wide, size=(sh, sw), keep_aspect=False)
    rgb = yuv_to_rgb8((Y, U, V), "yuv420p", "bt709", False)
    pixels, mask = compose(rgb, whole.windows.cpu().numpy(), sh, sw, lambda t, sub, rh, rw: sub)
    assert np.array_equal(whole.pixels.cpu().numpy(), pixels) and np.array_equal(whole.mask.cpu().numpy(), mask.astype(bool)) and whole.valid.all()
