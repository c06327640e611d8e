"""td_frame_export without a GPU: the rule's arithmetic in its numpy restatement (tests/export_ref.py: stages A and C, the
composition), the library's refusals through the C ABI (nothing is launched), and the Python layer's job records."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import export_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SPACES = [(m, fr) for m in ("bt601", "bt709") for fr in (False, True)]


# ---- stage A ----------------------------------------------------------------------------------------------------------------
def test_weights_of_one_output_sample_sum_to_n():
    for n in range(1, 41):
        for m in range(1, n + 1):
            w = ref.weights(n, m)
            assert (w.sum(axis=1) == n).all() and (w.sum(axis=0) == m).all() and w.min() >= 0, (n, m)
            # every source sample is touched by at most two output samples: nothing is enlarged
            assert ((w > 0).sum(axis=0) <= 2).all()


def test_equal_sizes_copy_and_two_to_one_is_the_rounded_mean_and_one_sample_is_the_plane_mean():
    rng = np.random.default_rng(1)
    for shape in ((1, 1), (5, 7), (6, 8), (33, 47)):
        p = rng.integers(0, 256, shape, dtype=np.uint8)
        assert np.array_equal(ref.area_resize(p, *shape), p)
        D = shape[0] * shape[1]
        assert ref.area_resize(p, 1, 1)[0, 0] == (int(p.astype(np.int64).sum()) + (D >> 1)) // D
    p = rng.integers(0, 256, (6, 8, 3), dtype=np.uint8)
    mean = (p.astype(np.int64).reshape(3, 2, 4, 2, 3).sum(axis=(1, 3)) + 2) >> 2
    assert np.array_equal(ref.area_resize(p, 3, 4), mean.astype(np.uint8))
    assert (ref.area_resize(np.full((37, 53), 255, np.uint8), 5, 7) == 255).all()  # rounding never leaves the range
    one_axis = ref.area_resize(p[..., 0], 6, 4)  # one axis only: rows are kept
    assert np.array_equal(one_axis, ((p[..., 0].astype(np.int64).reshape(6, 4, 2).sum(axis=2) + 1) >> 1).astype(np.uint8))


# ---- stage C ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("matrix,full_range", SPACES)
def test_a_solid_colour_exports_to_color_in_space(matrix, full_range):
    from tubedetr_amd.render import color_in_space

    for colour in ((0, 0, 0), (255, 255, 255), (250, 255, 0), (255, 0, 0), (0, 0, 255), (17, 200, 99), (1, 2, 3)):
        want = color_in_space(colour, "yuv420p", matrix, full_range)
        for h, w in ((1, 1), (1, 2), (2, 1), (2, 2), (3, 5)):  # blocks of n = 1, 2 and 4 pixels
            rgb = np.empty((h, w, 3), np.uint8)
            rgb[...] = colour
            Y, U, V = ref.rgb_to_yuv(rgb, matrix, full_range)
            assert (Y == want[0]).all() and (U == want[1]).all() and (V == want[2]).all(), (colour, h, w)


@pytest.mark.parametrize("matrix,full_range", SPACES)
def test_chroma_accumulators_fit_int32_and_the_result_is_within_0_5004_of_float64(matrix, full_range):
    (ry, ru, rv), offs, exact = ref.forward_coefficients(matrix, full_range)
    rng = np.random.default_rng(7)
    # the 4096 blocks whose 12 components are 0 or 255
    corners = np.stack([((np.arange(4096)[:, None] >> (3 * np.arange(4)[None, :] + ch)) & 1) * 255 for ch in range(3)], axis=-1)  # [4096][4 pixels][3]
    blocks = np.concatenate([corners, rng.integers(0, 256, (400000, 4, 3), dtype=np.int64)])
    for n in (1, 2, 4):
        sums = blocks[:, :n].sum(axis=1)
        for row, xrow in ((ru, exact[1]), (rv, exact[2])):
            val, acc = ref.chroma_from_sums(sums[:, 0], sums[:, 1], sums[:, 2], n, row, return_acc=True)
            assert acc.min() >= 0 and acc.max() <= 1 << 30
            f = (xrow[0] * sums[:, 0] + xrow[1] * sums[:, 1] + xrow[2] * sums[:, 2]) / n + 128.0
            assert np.abs(val - np.clip(f, 0, 255)).max() < 0.5004
    p = blocks[:, 0]
    acc = ry[0] * p[:, 0] + ry[1] * p[:, 1] + ry[2] * p[:, 2] + (offs[0] << 20) + (1 << 19)
    assert acc.min() >= 0 and acc.max() <= 1 << 30
    f = exact[0][0] * p[:, 0] + exact[0][1] * p[:, 1] + exact[0][2] * p[:, 2] + offs[0]
    assert np.abs(np.clip(acc >> 20, 0, 255) - f).max() < 0.5004


# ---- the composition ---------------------------------------------------------------------------------------------------------
def test_i420_to_nv12_and_back_at_the_same_size_is_byte_identical_and_take_and_padding_follow_the_header():
    rng = np.random.default_rng(3)
    T, h, w = 3, 5, 7
    clip = rng.integers(0, 256, T * ref.frame_bytes("yuv420p", h, w), dtype=np.uint8)
    nv, valid = ref.export(clip, "yuv420p", T, h, w, "nv12", h, w, h, w)
    back, _ = ref.export(nv, "nv12", T, h, w, "yuv420p", h, w, h, w)
    assert np.array_equal(back, clip) and valid.tolist() == [1, 1, 1] and not np.array_equal(nv, clip)
    out, valid = ref.export(clip, "yuv420p", T, h, w, "yuv420p", h, w, 6, 8, pad=(9, 8, 7), take=[2, -1, 0, 3, 2])
    assert valid.tolist() == [1, 0, 1, 0, 1]
    fb = ref.frame_bytes("yuv420p", 6, 8)
    frames = [ref.unpack(out[i * fb:(i + 1) * fb], "yuv420p", 6, 8) for i in range(5)]
    Y2, U2, V2 = ref.unpack(clip[2 * ref.frame_bytes("yuv420p", h, w):], "yuv420p", h, w)
    assert np.array_equal(frames[0][0][:h, :w], Y2) and (frames[0][0][h:] == 9).all() and (frames[0][0][:, w:] == 9).all()
    assert np.array_equal(frames[0][1][:3, :4], U2) and np.array_equal(frames[0][2][:3, :4], V2)  # chroma of 6 x 8 is 3 x 4: no chroma padding here
    assert (frames[1][0] == 9).all() and (frames[1][1] == 8).all() and (frames[1][2] == 7).all()
    assert all(np.array_equal(a, b) for a, b in zip(frames[0], frames[4]))
    # chroma padding: a 3 x 4 picture in a 6 x 8 frame has 2 x 2 chroma samples of the picture in planes of 3 x 4
    out, _ = ref.export(clip, "yuv420p", T, h, w, "nv12", 3, 4, 6, 8, pad=(9, 8, 7))
    Y, U, V = ref.unpack(out[:fb], "nv12", 6, 8)
    assert (U[2:] == 8).all() and (U[:, 2:] == 8).all() and (V[2:] == 7).all() and (V[:, 2:] == 7).all() and (Y[3:] == 9).all()


# ---- the library's refusals: no launch happens ---------------------------------------------------------------------------
def _call(job, nbytes=4096):
    from tubedetr_amd import _hip

    L = _hip.lib()
    table = ctypes.create_string_buffer(4096)
    arr = (_hip.ExportJob * 1)(job)
    rc = L.td_frame_export(arr, 1, ctypes.addressof(table), ctypes.c_void_p(4096), nbytes, None)
    return rc, L.td_last_error()


def _job(**kw):
    from tubedetr_amd.render import export_job

    args = dict(src=1 << 20, T=2, sh=6, sw=8, dst=1 << 24)
    args.update(kw)
    return export_job(**args)


@pytest.mark.parametrize("field,value,names", [
    ("oh", 7, (b"oh", b"enlargement")), ("ow", 9, (b"ow", b"enlargement")), ("oh", 0, (b"oh",)),
    ("dh", 5, (b"dh",)), ("dw", 7, (b"dw",)), ("dh", 16385, (b"dh",)),
    ("To", 3, (b"To", b"take")), ("To", -1, (b"To",)), ("T", -1, (b"T = ",)),
    ("src0", None, (b"src0", b"null")), ("dst0", None, (b"dst0", b"null")),
    ("src_pitch0", 23, (b"src_pitch0",)), ("dst_pitch0", 23, (b"dst_pitch0",)),
    ("src_frame_stride", 6 * 24 - 1, (b"src_frame_stride",)), ("dst_frame_stride", 6 * 24 - 1, (b"dst_frame_stride",)),
    ("sw", 8193, (b"sw",)), ("sh", 16385, (b"sh",)), ("src_fmt", 3, (b"src_fmt",)), ("dst_fmt", -1, (b"dst_fmt",)),
])
def test_library_refuses_a_violated_limit_and_names_the_field(field, value, names):
    job = _job()
    setattr(job, field, value)
    rc, msg = _call(job)
    assert rc != 0 and all(n in msg for n in names), msg


def test_library_refuses_big_resizes_overlaps_and_short_workspaces_and_takes_the_legal_edges():
    from tubedetr_amd import _hip

    L = _hip.lib()
    big = _job(T=0, sh=4097, sw=4096, dst=1 << 40)  # same size: no bound (no frames: checked, not launched)
    rc, msg = _call(big)
    assert rc == 0, msg
    big.oh = 4096
    big.dh = 4096
    rc, msg = _call(big)
    assert rc != 0 and b"sh * sw" in msg and b"2^24" in msg, msg
    for fmts in (("yuv420p", "rgb24"), ("rgb24", "nv12")):
        job = _job(src_fmt=fmts[0], dst_fmt=fmts[1])
        job.matrix = 2
        rc, msg = _call(job)
        assert rc != 0 and b"matrix" in msg
        job.matrix, job.full_range = 0, 2
        rc, msg = _call(job)
        assert rc != 0 and b"full_range" in msg
    rc, msg = _call(_job(dst=(1 << 20) + 1))
    assert rc != 0 and b"overlaps" in msg and b"dst0" in msg and b"src0" in msg
    rc, msg = _call(_job(dst=1 << 20))  # in place is an overlap too
    assert rc != 0 and b"overlaps" in msg
    rc, msg = _call(_job(dst=(1 << 20) - 10, size=(3, 4)))  # the end of the smaller destination reaches into the source
    assert rc != 0 and b"overlaps" in msg
    rc, msg = _call(_job(src_fmt="yuv420p", dst_fmt="nv12", dst_planes=[1 << 24, (1 << 20) + 50], dst_pitches=[8, 8], dst_frame_stride=1 << 12))
    assert rc != 0 and b"overlaps" in msg and b"dst1" in msg
    # To = 0: everything is checked, nothing is launched; T = 0 with a take list is legal (all blank) and reaches the upload
    rc, msg = _call(_job(T=0))
    assert rc == 0, msg
    rc, msg = _call(_job(dst=1 << 20, take=1 << 30, To=0))  # no frames: no bytes that could overlap
    assert rc == 0, msg
    rc, msg = _call(_job(), nbytes=L.td_frame_export_table_bytes(1) - 1)
    assert rc != 0 and b"table" in msg
    assert L.td_frame_export(None, 0, None, None, 0, None) != 0 and b"no jobs" in L.td_last_error()
    assert L.td_frame_export_table_bytes(0) == 0 and L.td_frame_export_table_bytes(3) % 256 == 0 and L.td_frame_export_table_bytes(3) > 0


def test_export_job_mirror_matches_the_header_and_the_abi_is_still_11():
    from tubedetr_amd import _hip, render

    src = open(os.path.join(ROOT, "include", "tubedetr_hip.h")).read()
    flat = " ".join(re.sub(r"/\*.*?\*/", "", src, flags=re.S).split())
    body = re.search(r"typedef struct td_export_job \{(.*?)\} td_export_job;", flat).group(1)
    names = [re.sub(r"\[\d+\]", "", part).split()[-1].lstrip("*") for decl in body.split(";") if decl.strip() for part in decl.split(",")]
    assert names == [n for n, _ in _hip.ExportJob._fields_], "td_export_job and its ctypes mirror list different fields"
    assert _hip.EXPECTED_ABI == 11 and _hip.lib().td_abi_version() == 11
    assert "td_frame_export" in _hip.EXPORTS and "td_frame_export_table_bytes" in _hip.EXPORTS
    assert re.search(r"int td_frame_export\(const td_export_job\* jobs, int n_jobs, void\* table_host, void\* table_dev, size_t table_bytes, td_stream_t stream\);", flat)
    assert flat.index("td_tube_follow(") < flat.index("typedef struct td_export_job")  # an addition: nothing above it changed
    assert render._JOB_TYPES["td_frame_export"] == "ExportJob"
    assert "frame_export.hip" in __import__("tubedetr_amd.build", fromlist=["SOURCES"]).SOURCES


def test_export_job_field_for_field_and_the_python_layers_refusals():
    from tubedetr_amd.render import _export_size, export_job

    j = export_job(4096, 3, 5, 7, 1 << 20, "rgb24", "yuv420p", size=(3, 4), frame_size=(4, 6), pad=(1, 2, 3), take=1 << 22, To=9, valid=1 << 23, matrix="bt709", full_range=True)
    assert (j.src0, j.src1, j.src2, j.src_pitch0, j.src_frame_stride, j.src_fmt) == (4096, None, None, 21, 105, 0)
    assert (j.dst0, j.dst1, j.dst2) == (1 << 20, (1 << 20) + 24, (1 << 20) + 24 + 6) and (j.dst_pitch0, j.dst_pitch1, j.dst_pitch2, j.dst_frame_stride, j.dst_fmt) == (6, 3, 3, 36, 1)
    assert (j.T, j.sh, j.sw, j.To, j.oh, j.ow, j.dh, j.dw, j.matrix, j.full_range) == (3, 5, 7, 9, 3, 4, 4, 6, 1, 1)
    assert (j.take, j.valid, tuple(j.pad)) == (1 << 22, 1 << 23, (1, 2, 3))
    j = export_job(4096, 3, 5, 7, 1 << 20, "nv12")  # the defaults: same format and size, no padding, every frame
    assert (j.dst_fmt, j.oh, j.ow, j.dh, j.dw, j.To, j.take, j.valid) == (2, 5, 7, 5, 7, 3, None, None) and (j.src1 - j.src0, j.src_pitch1, j.dst_frame_stride) == (35, 8, 35 + 24)
    j = export_job(0, 2, 5, 7, 0, "yuv420p", "rgb24", src_planes=[64, 640, 1280], src_pitches=[10, 7, 7], src_frame_stride=2000, dst_planes=[1 << 20], dst_pitches=[32], dst_frame_stride=160)
    assert (j.src0, j.src1, j.src2, j.src_pitch0, j.src_pitch1, j.src_pitch2, j.src_frame_stride) == (64, 640, 1280, 10, 7, 7, 2000) and (j.dst0, j.dst_pitch0, j.dst_frame_stride) == (1 << 20, 32, 160)
    for kw in (dict(size=(6, 7)), dict(size=(5, 8)), dict(size=(0, 1)), dict(frame_size=(4, 7)), dict(To=2), dict(take=64), dict(src_fmt="bgr24"), dict(dst_fmt="yuv444p"),
               dict(matrix="bt2020"), dict(pad=(0, 0, 256)), dict(dst=None), dict(sw=8193), dict(sh=4097, sw=4097, size=(4096, 4097))):
        args = dict(src=4096, T=3, sh=5, sw=7, dst=1 << 20)
        args.update(kw)
        with pytest.raises(ValueError):
            export_job(**args)
    assert _export_size(None, 720, 1280) == (720, 1280) and _export_size(360, 720, 1280) == (360, 640) and _export_size(360, 1280, 720) == (640, 360)
    assert _export_size((3, 4), 5, 7) == (3, 4) and _export_size(1, 5, 4000) == (1, 800) and _export_size(1, 4000, 3) == (1333, 1)
    assert _export_size(3, 9, 5) == (5, 3)  # 9 * 3 / 5 = 5.4
    for bad in ((6, 7), 6, 0, (1, 2, 3), 2.5):
        with pytest.raises(ValueError):
            _export_size(bad, 5, 7)


def test_moment_take_against_a_python_loop():
    from tubedetr_amd.render import moment_take

    for s0, s1, n, first, step in ((2, 4, 6, 0, 1), (2, 4, 2, 0, 1), (0, 0, 3, 5, 4), (1, 3, 12, 2, 5), (3, 3, 0, 0, 1), (4, 2, 5, 0, 1), (0, 9, 10, -3, 1)):
        got = moment_take(torch.tensor([s0, s1], dtype=torch.int64), n, first, step)
        f0, f1 = first + step * s0, first + step * s1
        want = [f0 + i if f0 + i <= f1 else -1 for i in range(n)]
        assert got.dtype == torch.int32 and got.tolist() == want
    for bad in (torch.tensor([1, 2], dtype=torch.int32), torch.tensor([1, 2, 3]), [1, 2]):
        with pytest.raises(ValueError):
            moment_take(bad, 4)
    with pytest.raises(ValueError):
        moment_take(torch.tensor([1, 2]), 4, step=0)
