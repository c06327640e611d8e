"""td_frame_export and tubedetr_amd.render.export on the GPU.  Every comparison is bit equality (torch.equal) with the numpy
restatement of the header's rule (tests/export_ref.py).

A job's destination planes lie in ONE buffer of random bytes, 64 of them in front of every plane of every frame (+ a shift of the
whole layout where a test says so), rows at a pitch of their length + a gap; ``valid`` lies between 64 canary bytes.  The whole
buffers are compared, so a byte written into the row gaps, in front of a plane or behind it shows; the source lies in such a buffer
too and must come back unchanged.  Sizes are rows x columns."""
import numpy as np
import pytest
import torch

import export_ref as ref

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
FMTS = ["rgb24", "yuv420p", "nv12"]
PAIRS = [(s, d) for s in FMTS for d in FMTS]
PAD = (200, 90, 30)
# (sh, sw) -> (oh, ow): one sample; odd, same size; odd, smaller; a ratio that is no integer with odd chroma planes; exactly 2:1;
# a whole plane to one sample; one axis only at a ratio above 15
SHAPES = [((1, 1), (1, 1)), ((5, 7), (5, 7)), ((5, 7), (3, 4)), ((33, 47), (16, 23)), ((64, 80), (32, 40)), ((37, 53), (1, 1)), ((48, 200), (48, 13))]


def plane_rows(fmt, h, w):
    """(rows, row bytes) of every plane of one frame."""
    ch, cw = (h + 1) // 2, (w + 1) // 2
    return [(h, 3 * w)] if fmt == "rgb24" else [(h, w), (ch, cw), (ch, cw)] if fmt == "yuv420p" else [(h, w), (ch, 2 * cw)]


def layout(fmt, h, w, T, gap, shift=0):
    geo = plane_rows(fmt, h, w)
    pitches = [rb + gap for _, rb in geo]
    offs, at = [], shift
    for (rows, _), pitch in zip(geo, pitches):
        offs.append(at + 64)
        at += 64 + rows * pitch
    stride = at - shift
    return dict(geo=geo, pitches=pitches, offs=offs, stride=stride, total=shift + max(T, 1) * stride + 64)


def place(buf, tight, fmt, h, w, T, lay):
    """The tightly packed frames ``tight`` written into their rows of ``buf``."""
    fb = ref.frame_bytes(fmt, h, w)
    for t in range(T):
        at = t * fb
        for (rows, rb), pitch, off in zip(lay["geo"], lay["pitches"], lay["offs"]):
            for r in range(rows):
                o = off + t * lay["stride"] + r * pitch
                buf[o:o + rb] = tight[at:at + rb]
                at += rb
    return buf


def spec(src_fmt, dst_fmt, T, size, out, frame=None, take=None, pad=PAD, matrix="bt601", full_range=False, seed=0, data=None, src_gap=3, dst_gap=5, dst_shift=0):
    sh, sw = size
    oh, ow = out
    dh, dw = frame if frame is not None else out
    if data is None:
        data = np.random.default_rng(seed + 1000 * sh + sw).integers(0, 256, T * ref.frame_bytes(src_fmt, sh, sw), dtype=np.uint8)
    return dict(src_fmt=src_fmt, dst_fmt=dst_fmt, T=T, sh=sh, sw=sw, oh=oh, ow=ow, dh=dh, dw=dw, take=take, pad=pad, matrix=matrix, full_range=full_range, data=data,
                src_gap=src_gap, dst_gap=dst_gap, dst_shift=dst_shift)


def want_of(s):
    """The reference of a spec, computed once and kept in it."""
    if "_want" not in s:
        s["_want"] = ref.export(s["data"], s["src_fmt"], s["T"], s["sh"], s["sw"], s["dst_fmt"], s["oh"], s["ow"], s["dh"], s["dw"], s["pad"], s["take"], s["matrix"], s["full_range"])
    return s["_want"]


def launch(specs):
    """ONE launch of all specs; returns the destination and valid buffers as numpy (whole buffers), after asserting that they are
    the reference placed into the buffers' canaries and that the sources are unchanged."""
    from tubedetr_amd.render import export_job, frame_export

    dev = torch.device(DEV)
    rng = np.random.default_rng(99)
    jobs, keep, checks = [], [], []
    for i, s in enumerate(specs):
        want, want_valid = want_of(s)
        To = s["T"] if s["take"] is None else len(s["take"])
        slay = layout(s["src_fmt"], s["sh"], s["sw"], s["T"], s["src_gap"])
        dlay = layout(s["dst_fmt"], s["dh"], s["dw"], To, s["dst_gap"], s["dst_shift"])
        src = place(rng.integers(0, 256, slay["total"], dtype=np.uint8), s["data"], s["src_fmt"], s["sh"], s["sw"], s["T"], slay)
        dst = rng.integers(0, 256, dlay["total"], dtype=np.uint8)
        val = rng.integers(2, 256, 128 + To, dtype=np.uint8)
        d_src, d_dst, d_val = torch.from_numpy(src).to(dev), torch.from_numpy(dst).to(dev), torch.from_numpy(val).to(dev)
        d_take = torch.tensor(list(s["take"]) + [0], dtype=torch.int32, device=dev) if s["take"] is not None else None  # (+ one entry: an empty list still has an address)
        want_dst = place(dst.copy(), want, s["dst_fmt"], s["dh"], s["dw"], To, dlay)
        want_val = val.copy()
        want_val[64:64 + To] = want_valid
        jobs.append(export_job(0, s["T"], s["sh"], s["sw"], 0, s["src_fmt"], s["dst_fmt"], (s["oh"], s["ow"]), (s["dh"], s["dw"]), s["pad"],
                               d_take.data_ptr() if d_take is not None else None, To, d_val.data_ptr() + 64, s["matrix"], s["full_range"],
                               src_planes=[d_src.data_ptr() + o for o in slay["offs"]], src_pitches=slay["pitches"], src_frame_stride=slay["stride"],
                               dst_planes=[d_dst.data_ptr() + o for o in dlay["offs"]], dst_pitches=dlay["pitches"], dst_frame_stride=dlay["stride"]))
        keep.append(d_take)
        checks.append((d_src, src, d_dst, want_dst, d_val, want_val))
    tables = frame_export(jobs, dev)
    torch.cuda.synchronize()
    del tables
    got = []
    for i, (d_src, src, d_dst, want_dst, d_val, want_val) in enumerate(checks):
        g_dst, g_val = d_dst.cpu(), d_val.cpu()
        s = specs[i]
        what = f"job {i} ({s['src_fmt']} {s['sh']} x {s['sw']} -> {s['dst_fmt']} {s['oh']} x {s['ow']} in {s['dh']} x {s['dw']})"
        assert torch.equal(g_dst, torch.from_numpy(want_dst)), f"{what}: {(g_dst.numpy() != want_dst).sum()} of {want_dst.size} bytes differ from the reference"
        assert torch.equal(g_val, torch.from_numpy(want_val)), f"{what}: valid differs"
        assert torch.equal(d_src.cpu(), torch.from_numpy(src)), f"{what}: the source was written"
        got.append((g_dst.numpy(), g_val.numpy()))
    return got


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0][0]}x{s[0][1]}-{s[1][0]}x{s[1][1]}")
def test_all_nine_format_pairs(shape):
    size, out = shape
    launch([spec(sf, df, 2, size, out) for sf, df in PAIRS])


def test_pitches_misaligned_bases_and_padding_to_even_and_wider_frames():
    specs = []
    for sf, df in PAIRS:
        specs.append(spec(sf, df, 2, (33, 47), (15, 23), frame=(16, 24), dst_shift=1, seed=1))          # odd -> even padding, base 1 mod 16
        specs.append(spec(sf, df, 2, (33, 47), (16, 23), frame=(16, 39), dst_shift=7, dst_gap=0, seed=2))  # dw = ow + 16; rows back to back
        specs.append(spec(sf, df, 1, (20, 300), (20, 300), frame=(21, 301), src_gap=0, dst_gap=11, dst_shift=4, seed=3))  # two column tiles, three bands, padding in the second tile
    launch(specs)


def test_more_than_one_tile_both_ways_at_a_ratio_that_is_no_integer():
    launch([spec(sf, df, 1, (45, 700), (19, 290), frame=(20, 290), seed=4) for sf, df in PAIRS])


def test_take():
    T, size, out = 5, (9, 11), (4, 6)
    takes = [None, [4, 3, 2, 1, 0], [0, 2, 4], [1, 1, 3, 3, 3, 1, 0], [-1, 0, T, 2, -7, T + 100], []]
    specs = [spec(sf, df, T, size, out, frame=(4, 8), take=tk, seed=5) for tk in takes for sf, df in (("rgb24", "yuv420p"), ("nv12", "rgb24"), ("yuv420p", "yuv420p"))]
    got = launch(specs)
    blank = [g for g, s in zip(got, specs) if s["take"] is not None and len(s["take"]) == 6]
    assert [v[64:70].tolist() for _, v in blank] == [[0, 1, 0, 1, 0, 0]] * 3
    # no source frames at all: every entry is out of range, every frame blank
    launch([spec(sf, df, 0, size, out, take=[0, -1, 1], seed=6) for sf, df in (("rgb24", "nv12"), ("yuv420p", "rgb24"))])


@pytest.mark.parametrize("matrix", ["bt601", "bt709"])
@pytest.mark.parametrize("full_range", [False, True])
def test_both_matrices_and_both_ranges(matrix, full_range):
    from tubedetr_amd.render import color_in_space

    specs = [spec("rgb24", "yuv420p", 2, (33, 47), (16, 23), frame=(16, 24), matrix=matrix, full_range=full_range, seed=7),
             spec("nv12", "rgb24", 2, (33, 47), (16, 23), matrix=matrix, full_range=full_range, seed=8)]
    colour = (250, 255, 0)
    solid = np.tile(np.array(colour, np.uint8), 9 * 11)
    specs.append(spec("rgb24", "nv12", 1, (9, 11), (5, 7), frame=(6, 8), pad=color_in_space(colour, "nv12", matrix, full_range), matrix=matrix, full_range=full_range, data=solid))
    got = launch(specs)
    # a solid colour exports to color_in_space(colour): with the pad of the same colour the whole frame is three values
    lay = layout("nv12", 6, 8, 1, 5)
    y, u, v = color_in_space(colour, "nv12", matrix, full_range)
    frame = got[2][0]
    assert all((frame[lay["offs"][0] + r * lay["pitches"][0]:][:8] == y).all() for r in range(6))
    assert all((frame[lay["offs"][1] + r * lay["pitches"][1]:][:8] == np.array([u, v] * 4)).all() for r in range(3))


def test_the_unsigned_32_bit_bound():
    """255 x 2^24 + 2^23 is the largest accumulator a resizing job can have; the expected bytes are written down, not computed."""
    from tubedetr_amd.render import export_job, frame_export

    dev = torch.device(DEV)
    for (sh, sw), (oh, ow) in (((4096, 4096), (1, 1)), ((2160, 3840), (5, 7))):
        src = torch.full((3 * sh * sw,), 255, dtype=torch.uint8, device=dev)
        dst = torch.zeros(64 + 3 * oh * ow + 64, dtype=torch.uint8, device=dev)
        tables = frame_export([export_job(src.data_ptr(), 1, sh, sw, dst.data_ptr() + 64, "rgb24", size=(oh, ow))], dev)
        torch.cuda.synchronize()
        del tables
        want = torch.zeros_like(dst)
        want[64:64 + 3 * oh * ow] = 255
        assert torch.equal(dst, want), (sh, sw, oh, ow)
    launch([spec("rgb24", "rgb24", 1, (4096, 4096), (2, 2), src_gap=0, seed=9)])


def test_five_mixed_jobs_in_one_launch_give_the_same_bits_twice():
    specs = [spec("rgb24", "yuv420p", 3, (33, 47), (16, 23), frame=(16, 24), take=[2, 0, -1, 1], seed=10),
             spec("yuv420p", "nv12", 2, (64, 80), (64, 80), seed=11),
             spec("nv12", "rgb24", 1, (45, 700), (19, 290), matrix="bt709", seed=12),
             spec("rgb24", "rgb24", 4, (5, 7), (3, 4), frame=(4, 4), take=[3, 3], seed=13),
             spec("yuv420p", "yuv420p", 2, (37, 53), (1, 1), frame=(2, 2), full_range=True, seed=14)]
    first = launch(specs)
    second = launch(specs)
    for (a, av), (b, bv) in zip(first, second):
        assert np.array_equal(a, b) and np.array_equal(av, bv)


# ---- end to end ----------------------------------------------------------------------------------------------------------------
def test_annotate_then_export_then_to_decoded_equals_the_reference_on_the_annotated_bytes():
    from tubedetr_amd.augment import DecodedClip
    from tubedetr_amd.render import DeviceFrames, annotate, export

    dev = torch.device(DEV)
    T, h, w = 4, 45, 70
    clip = DecodedClip(torch.from_numpy(np.random.default_rng(20).integers(0, 256, T * 3 * h * w, dtype=np.uint8)), T, h, w, "rgb24")
    frames = DeviceFrames.from_decoded(clip, dev)
    boxes = torch.tensor([[5.0, 4.0, 40.0, 30.0]] * T, device=dev)
    drawn = annotate(frames, boxes)
    out = export(drawn, size=19, pix_fmt="yuv420p")
    host = out.to_decoded()
    torch.cuda.synchronize()
    assert (out.T, out.h, out.w, out.pix_fmt) == (T, 20, 30, "yuv420p") and (host.T, host.h, host.w, host.pix_fmt) == (T, 20, 30, "yuv420p") and host.data.is_pinned()
    annotated = drawn.data.cpu().numpy()
    assert not np.array_equal(annotated, clip.data.numpy())
    want, _ = ref.export(annotated, "rgb24", T, h, w, "yuv420p", 19, 30, 20, 30, (16, 128, 128))
    assert torch.equal(host.data, torch.from_numpy(want))
    # a list of clips in one launch, a Python range for take, no padding
    (a, a_valid), (c, c_valid) = export([drawn, frames], size=(10, 11), take=[range(0, T, 2), [1, T]], multiple=1, want_valid=True)
    b, b_valid = export(frames, take=[1, T], want_valid=True, pad_color=(255, 0, 0))
    torch.cuda.synchronize()
    assert torch.equal(a.data.cpu(), torch.from_numpy(ref.export(annotated, "rgb24", T, h, w, "rgb24", 10, 11, 10, 11, take=[0, 2])[0])) and a_valid.cpu().tolist() == [True, True]
    assert torch.equal(c.data.cpu(), torch.from_numpy(ref.export(clip.data.numpy(), "rgb24", T, h, w, "rgb24", 10, 11, 10, 11, take=[1, T])[0])) and c_valid.cpu().tolist() == [True, False]
    want, _ = ref.export(clip.data.numpy(), "rgb24", T, h, w, "rgb24", h, w, h + 1, w, (255, 0, 0), take=[1, T])
    assert torch.equal(b.data.cpu(), torch.from_numpy(want)) and b_valid.cpu().tolist() == [True, False] and (b.h, b.w) == (h + 1, w)
    empty = export(frames, take=[])
    assert empty.T == 0 and empty.data.numel() == 0


def test_moment_take_cuts_the_clip_to_the_answer():
    from tubedetr_amd.render import DeviceFrames, export, moment_take

    dev = torch.device(DEV)
    T, h, w = 12, 6, 10
    grey = torch.arange(T, dtype=torch.uint8, device=dev).repeat_interleave(3 * h * w)  # frame t is the solid grey t
    frames = DeviceFrames(grey, T, h, w, "rgb24")
    span = torch.tensor([1, 3], dtype=torch.int64, device=dev)  # sampled rows 1..3 at frames 2 + 2 r: decoded frames 4..8
    out, valid = export(frames, size=3, take=moment_take(span, 7, first=2, step=2), want_valid=True, pad_color=(9, 9, 9))
    torch.cuda.synchronize()
    assert (out.T, out.h, out.w) == (7, 4, 6)
    pixels = out.data.cpu().view(7, 4, 6, 3)
    assert valid.cpu().tolist() == [True] * 5 + [False] * 2
    for i in range(7):
        assert (pixels[i, :3, :5] == (4 + i if i < 5 else 9)).all() and (pixels[i, 3:] == 9).all() and (pixels[i, :, 5:] == 9).all()
