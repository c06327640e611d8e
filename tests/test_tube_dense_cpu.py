"""td_tube_densify without a GPU: properties of the numpy reference that pin the rule's intent (tests/tube_dense_ref.py), the
library's own refusals (nothing is launched: no device is needed), and the ctypes mirror against the header."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from tube_dense_ref import QNAN_BITS, dense_floats, densify_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROW_FRAME = [3, 4, 9, 16, 21, 22, 27]  # gaps of 1, 5 and 7


def tube(n, K, seed=0):
    rng = np.random.default_rng(seed)
    x0, y0 = rng.uniform(0, 300, (n, K)), rng.uniform(0, 200, (n, K))
    return np.stack([x0, y0, x0 + rng.uniform(2, 300, (n, K)), y0 + rng.uniform(2, 200, (n, K))], -1).astype(np.float32)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@pytest.mark.parametrize("smooth", [0, 2])
def test_hull_contains_lerp_at_every_frame(smooth):
    boxes = tube(len(ROW_FRAME), 3)
    kw = dict(row_frame=ROW_FRAME, t0=0, span=[[0, 6], [1, 4], [2, 2]], smooth=smooth)
    lerp, hull = densify_ref(boxes, 30, mode="lerp", **kw), densify_ref(boxes, 30, mode="hull", **kw)
    L, H = dense_floats(lerp), dense_floats(hull)
    on = lerp["valid"].astype(bool)
    assert on.sum() > 30 and (hull["valid"].astype(bool) | ~on).all()  # wherever LERP has a box, HULL has one
    assert (H[on][:, :2] <= L[on][:, :2]).all() and (H[on][:, 2:] >= L[on][:, 2:]).all()
    assert hull["valid"].sum() > lerp["valid"].sum()  # the one-sided hold at the ends of the spans


def test_lerp_at_an_exact_hit_returns_the_rows_bits_and_smooth_0_is_the_identity():
    boxes = tube(len(ROW_FRAME), 2, seed=1)
    for mode in ("hold", "lerp", "hull"):
        ref = densify_ref(boxes, 30, row_frame=ROW_FRAME, mode=mode, smooth=0)
        for r, f in enumerate(ROW_FRAME):
            assert np.array_equal(ref["dense"][f], bits(boxes[r])) and ref["valid"][f].all()
        assert (ref["dense"][:3] == QNAN_BITS).all() and (ref["dense"][28:] == QNAN_BITS).all() and not ref["valid"][:3].any() and not ref["valid"][28:].any()
    same = densify_ref(boxes, len(boxes), first=0, step=1, mode="lerp", smooth=0)  # the dense rate is the sampled rate
    assert np.array_equal(same["dense"], bits(boxes)) and same["valid"].all()


def test_a_smoothing_radius_beyond_the_tube_gives_every_present_row_the_mean_of_all_present_rows():
    boxes = tube(5, 2, seed=2)
    boxes[3, 1, 2] = np.nan
    ref = densify_ref(boxes, 5, first=0, step=1, mode="lerp", smooth=16)
    got = dense_floats(ref)
    for k, rows in ((0, [0, 1, 2, 3, 4]), (1, [0, 1, 2, 4])):
        s = np.zeros(4, dtype=np.float32)
        for q in rows:
            s = (s + boxes[q, k]).astype(np.float32)
        mean = (s / np.float32(len(rows))).astype(np.float32)
        for r in rows:
            assert np.array_equal(bits(got[r, k]), bits(mean))
    assert (ref["dense"][3, 1] == QNAN_BITS).all() and ref["valid"][3, 1] == 0  # an absent row stays absent


def test_hold_is_the_frame_map():
    boxes = tube(len(ROW_FRAME), 2, seed=3)
    span = np.array([[1, 5], [0, 3]])
    T, t0 = 31, -1
    ref = densify_ref(boxes, T, row_frame=ROW_FRAME, t0=t0, span=span, mode="hold")
    for i in range(T):
        f = t0 + i
        r = max([q for q, fq in enumerate(ROW_FRAME) if fq <= f], default=-1)  # the frame_map a caller would build
        for k in range(2):
            if r >= 0 and f <= ROW_FRAME[-1] and span[k, 0] <= r <= span[k, 1]:
                assert np.array_equal(ref["dense"][i, k], bits(boxes[r, k])) and ref["valid"][i, k] == 1
            else:
                assert (ref["dense"][i, k] == QNAN_BITS).all() and ref["valid"][i, k] == 0


def test_a_nan_row_in_mid_span_is_skipped_by_smoothing_and_opens_two_intervals_under_lerp():
    boxes = tube(5, 1, seed=4)
    boxes[2, 0, 1] = np.nan
    ref = densify_ref(boxes, 21, first=0, step=5, mode="lerp")
    assert ref["valid"][:, 0].tolist() == [1] * 6 + [0] * 9 + [1] * 6  # rows at 0, 5, [10], 15, 20
    hull = densify_ref(boxes, 21, first=0, step=5, mode="hull")
    assert hull["valid"][:, 0].tolist() == [1] * 10 + [0] + [1] * 10  # held from either side; the row itself is absent
    assert np.array_equal(hull["dense"][7, 0], bits(boxes[1, 0])) and np.array_equal(hull["dense"][13, 0], bits(boxes[3, 0]))
    smooth = dense_floats(densify_ref(boxes, 21, first=0, step=5, mode="hold", smooth=1))
    want = ((np.float32(0) + boxes[0, 0]).astype(np.float32) + boxes[1, 0]).astype(np.float32) / np.float32(2)  # row 1: rows 0 and 1, row 2 is skipped
    assert np.array_equal(bits(smooth[5, 0]), bits(want.astype(np.float32)))
    assert np.array_equal(bits(smooth[15, 0]), bits(((boxes[3, 0] + boxes[4, 0]).astype(np.float32) / np.float32(2)).astype(np.float32)))


def test_dense_span_empty_clipped_and_the_hull_extension():
    boxes = tube(len(ROW_FRAME), 4, seed=5)
    span = [[2, 4], [5, 3], [-7, 1], [4, 99]]
    for mode in ("hold", "lerp"):
        got = densify_ref(boxes, 10, row_frame=ROW_FRAME, t0=2, span=span, mode=mode)["span"]
        assert got.tolist() == [[9 - 2, 21 - 2], [0, -1], [3 - 2, 4 - 2], [21 - 2, 27 - 2]]
    got = densify_ref(boxes, 10, row_frame=ROW_FRAME, t0=2, span=span, mode="hull")["span"]
    assert got.tolist() == [[4 + 1 - 2, 22 - 1 - 2], [0, -1], [3 - 2, 9 - 1 - 2], [16 + 1 - 2, 27 - 2]]
    assert densify_ref(boxes, 0, first=10, step=5, mode="hull")["span"].tolist() == [[10, 40]] * 4  # NULL span; T = 0 still has one


def test_heat_rule():
    heat = np.array([[[0, 255]], [[10, 0]], [[200, 100]]], dtype=np.uint8)  # (3, 1, 2)
    boxes = tube(3, 1)
    lerp = densify_ref(boxes, 9, first=1, step=3, heat=heat, mode="lerp")["heat"]
    assert lerp[:, 0, 0].tolist() == [0, 0, 3, 7, 10, 73, 137, 200, 0] and lerp[:, 0, 1].tolist() == [0, 255, 170, 85, 0, 33, 67, 100, 0]
    assert densify_ref(boxes, 9, first=1, step=3, heat=heat, mode="hold")["heat"][:, 0, 0].tolist() == [0, 0, 0, 0, 10, 10, 10, 200, 0]
    assert densify_ref(boxes, 9, first=1, step=3, heat=heat, mode="hull")["heat"][:, 0, 1].tolist() == [0, 255, 255, 255, 0, 100, 100, 100, 0]


# ---- the library's refusals: no launch happens ---------------------------------------------------------------------------
def _call(job, nbytes=4096):
    from tubedetr_amd import _hip

    L = _hip.lib()
    table = ctypes.create_string_buffer(4096)
    arr = (_hip.DenseJob * 1)(job)
    rc = L.td_tube_densify(arr, 1, ctypes.addressof(table), ctypes.c_void_p(4096), nbytes, None)
    return rc, L.td_last_error()


def _job(**kw):
    from tubedetr_amd.render import dense_job

    args = dict(boxes=1 << 20, n_tube=3, T=0, dense=1 << 24)  # T = 0 without dense_span: a job that passes is not launched
    args.update(kw)
    return dense_job(**args)


@pytest.mark.parametrize("field,value,name", [
    ("boxes", None, b"boxes"), ("dense", None, b"dense"), ("n_tube", 0, b"n_tube"), ("K", 0, b"K = "), ("K", 9, b"K = "),
    ("T", -1, b"T = "), ("T", (1 << 20) + 1, b"T = "), ("t0", (1 << 23) + 1, b"t0"), ("t0", -(1 << 23) - 1, b"t0"),
    ("first", (1 << 23) + 1, b"first"), ("first", -(1 << 23) - 1, b"first"), ("step", 0, b"step"), ("step", (1 << 16) + 1, b"step"),
    ("smooth", -1, b"smooth"), ("smooth", 17, b"smooth"), ("mode", 3, b"mode"), ("mode", -1, b"mode"),
    ("heat", 1 << 26, b"dense_heat"), ("dense_heat", 1 << 26, b"heat is null"),
])
def test_library_refuses_a_violated_limit_and_names_the_field(field, value, name):
    job = _job()
    setattr(job, field, value)
    rc, msg = _call(job)
    assert rc != 0 and name in msg, msg


@pytest.mark.parametrize("field,value", [("mh", 0), ("mh", 257), ("mw", 0), ("mw", 257)])
def test_library_refuses_a_map_side_outside_1_to_256(field, value):
    job = _job(heat=1 << 26, dense_heat=1 << 27, heat_hw=(4, 4))
    setattr(job, field, value)
    rc, msg = _call(job)
    assert rc != 0 and field.encode() in msg, msg


def test_library_accepts_what_the_rule_allows_and_checks_its_workspace():
    from tubedetr_amd import _hip

    L = _hip.lib()
    for kw in (dict(), dict(t0=1 << 23, first=-(1 << 23), step=1 << 16, smooth=16, K=8, mode="hull"), dict(heat=1 << 26, dense_heat=1 << 27, heat_hw=(256, 1))):
        rc, msg = _call(_job(**kw))
        assert rc == 0, msg
    job = _job(row_frame=1 << 22)  # with a table, first and step are not read
    job.first, job.step = 1 << 30, 0
    rc, msg = _call(job)
    assert rc == 0, msg
    job = _job()  # without heat, mh and mw are not read
    job.mh, job.mw = 0, 999
    rc, msg = _call(job)
    assert rc == 0, msg
    rc, msg = _call(_job(), nbytes=L.td_tube_densify_table_bytes(1) - 1)
    assert rc != 0 and b"table" in msg
    assert L.td_tube_densify(None, 0, None, None, 0, None) != 0 and b"no jobs" in L.td_last_error()
    assert L.td_tube_densify_table_bytes(0) == 0 and L.td_tube_densify_table_bytes(3) % 256 == 0 and L.td_tube_densify_table_bytes(3) > 0
    assert L.td_tube_densify_table_bytes(16) <= 4096  # a batch of clips fits the smallest pooled table


def test_dense_job_mirror_matches_the_header_and_the_abi_is_still_11():
    from tubedetr_amd import _hip

    src = open(os.path.join(ROOT, "include", "tubedetr_hip.h")).read()
    flat = " ".join(re.sub(r"/\*.*?\*/", "", src, flags=re.S).split())
    body = re.search(r"typedef struct td_dense_job \{(.*?)\} td_dense_job;", flat).group(1)
    names = [part.split()[-1].lstrip("*") for decl in body.split(";") if decl.strip() for part in decl.split(",")]
    assert names == [n for n, _ in _hip.DenseJob._fields_], "td_dense_job and its ctypes mirror list different fields"
    kinds = {"boxes": "P", "span": "P", "row_frame": "P", "heat": "P", "dense": "P", "valid": "P", "dense_span": "P", "dense_heat": "P"}
    for n, t in _hip.DenseJob._fields_:
        assert t is (ctypes.c_void_p if kinds.get(n) == "P" else ctypes.c_int), n
    assert _hip.EXPECTED_ABI == 11 and _hip.lib().td_abi_version() == 11
    assert "td_tube_densify" in _hip.EXPORTS and "td_tube_densify_table_bytes" in _hip.EXPORTS
    assert re.search(r"int td_tube_densify\(const td_dense_job\* jobs, int n_jobs, void\* table_host, void\* table_dev, size_t table_bytes, td_stream_t stream\);", flat)
    assert flat.index("td_linear_ex_route(") < flat.index("typedef struct td_dense_job")  # an addition: nothing above it changed
    for name, code in (("HOLD", _hip.TD_DENSE_HOLD), ("LERP", _hip.TD_DENSE_LERP), ("HULL", _hip.TD_DENSE_HULL)):
        assert re.search(rf"#define TD_DENSE_{name} {code}\b", src)
    assert "WITHIN ABI 11" in src[src.index("Grounded tubes interpolated"):src.index("#define TD_DENSE_HOLD")]
    assert "tube_dense.hip" in __import__("tubedetr_amd.build", fromlist=["SOURCES"]).SOURCES


def test_python_layer_refuses_bad_arguments_before_the_device_is_touched():
    from tubedetr_amd.render import dense_job, densify

    ok = dense_job(4096, 5, 30, 8192, K=2, mode="hull", smooth=3, first=-4, step=6, t0=7)
    assert (ok.boxes, ok.dense, ok.n_tube, ok.K, ok.T, ok.t0, ok.first, ok.step, ok.mode, ok.smooth) == (4096, 8192, 5, 2, 30, 7, -4, 6, 2, 3)
    assert (ok.span, ok.row_frame, ok.heat, ok.valid, ok.dense_span, ok.dense_heat) == (None,) * 6
    for kw in ({"mode": "linear"}, {"smooth": 17}, {"smooth": -1}, {"smooth": 1.5}, {"K": 0}, {"K": 9}, {"T": -1}, {"T": (1 << 20) + 1}, {"t0": (1 << 23) + 1},
               {"first": -(1 << 23) - 1}, {"step": 0}, {"step": (1 << 16) + 1}, {"boxes": None}, {"dense": None}, {"n_tube": 0}, {"heat": 4096},
               {"dense_heat": 4096}, {"heat": 4096, "dense_heat": 8192, "heat_hw": (0, 4)}, {"heat": 4096, "dense_heat": 8192, "heat_hw": (4, 257)}):
        with pytest.raises(ValueError):
            dense_job(**{"boxes": 4096, "n_tube": 2, "T": 4, "dense": 8192, **kw})
    # tensors that live on no device: every scalar is refused from the arguments alone, and so are the tensors themselves
    boxes = torch.zeros(3, 4)
    good = {"T": 4, "mode": "lerp", "smooth": 0, "t0": 0, "first": 0, "step": 1}
    for name, bad in (("mode", "linear"), ("smooth", 17), ("T", -1), ("T", (1 << 20) + 1), ("t0", -(1 << 23) - 1), ("first", (1 << 23) + 1), ("step", 0)):
        with pytest.raises(ValueError, match=name):
            densify(boxes, **{**good, name: bad})
        with pytest.raises(ValueError, match=name):
            densify([boxes, boxes], **{**good, name: [good[name], bad]})  # the second clip's
    with pytest.raises(ValueError, match="boxes"):
        densify(boxes, 4)
    with pytest.raises(ValueError):
        densify([boxes, boxes], [4])  # one T for two clips
    assert densify([], 4) == []
