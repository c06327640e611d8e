"""td_tube_follow without a device: the numpy restatement of the rule (tests/follow_ref.py) on the synthetic scene and on
hand-built cases, and every host refusal of td_tube_follow through ctypes - nothing is launched on those paths, so the addresses
are made up.  The message texts are part of the interface."""
import ctypes

import numpy as np
import pytest

from follow_ref import F32, best_candidate, candidate_costs, corner_error, find_anchor, follow_ref, luma_of_planes, luma_of_rgb, sample_points, scene

SRC, OUT = 1 << 20, 1 << 24
T, SH, SW = 2, 6, 8  # yuv420p: Y 6 rows of 8 bytes, U and V 3 rows of 4; 72 bytes per frame


# ---- the rule -------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def the_scene():
    luma, true, anchor, lerp = scene()
    return luma, true, anchor, lerp, follow_ref(luma, lerp, anchor)


def test_following_brings_every_frame_onto_the_object_where_lerp_is_off(the_scene):
    luma, true, anchor, lerp, got = the_scene
    before, after = corner_error(lerp, true), corner_error(got["out"], true)
    between = anchor == 0
    print("lerp", before.round(2).tolist(), "followed", after.tolist(), "cost per sample", (got["cost"] / 256).round(2).tolist())
    assert (before[between] >= 2).all() and (before[~between] == 0).all()
    assert (after <= 1).all()
    assert (got["status"][between] == 1).all() and (got["status"][~between] == 0).all()
    assert (got["cost"][between] < 3 * 256).all() and (got["cost"][~between] == 0).all() and (got["offset"][~between] == 0).all()
    assert np.array_equal(got["out"][~between].view(np.uint32), lerp[~between].view(np.uint32))


def test_a_grey_frame_is_rejected_and_keeps_its_box(the_scene):
    luma, true, anchor, lerp, _ = the_scene
    grey = luma.copy()
    grey[8] = 128
    got = follow_ref(grey, lerp, anchor)
    assert got["status"][8] == 2 and got["offset"][8].tolist() == [0, 0] and got["cost"][8] > 24 * 256
    assert np.array_equal(got["out"][8].view(np.uint32), lerp[8].view(np.uint32))
    assert (got["status"][[7, 9]] == 1).all()  # every frame is matched against an anchor: its neighbours do not notice


def _flat(T=3, sh=20, sw=30, v=77):
    return np.full((T, sh, sw), v, dtype=np.uint8)


BOX = [5, 4, 21, 16]


def test_on_a_flat_picture_the_tie_order_answers_no_shift():
    boxes = np.array([BOX, [7, 5, 23, 17], BOX], dtype=F32)
    got = follow_ref(_flat(), boxes, [1, 0, 1], radius=16)
    assert got["offset"][1].tolist() == [0, 0] and got["status"][1] == 1 and got["cost"][1] == 0
    assert np.array_equal(got["out"].view(np.uint32), boxes.view(np.uint32))
    c = np.zeros((5, 5), dtype=np.int64)
    assert best_candidate(c, 2) == (0, 0, 0)
    c[2, 2] = 1  # without the centre: (dy, dx) = (-1, 0) before (0, -1), (0, 1) and (1, 0)
    assert best_candidate(c, 2) == (0, -1, 0)
    c[1, 2] = 1
    assert best_candidate(c, 2) == (0, 0, -1)


def test_radius_zero_has_one_candidate():
    rng = np.random.default_rng(1)
    luma = rng.integers(0, 256, (2, 20, 30), dtype=np.uint8)
    boxes = np.array([BOX, [6, 6, 22, 18]], dtype=F32)
    got = follow_ref(luma, boxes, [1, 0], radius=0, accept=(255, 1))
    py, px = sample_points(BOX, 20, 30)
    want = np.abs(luma[1][py[:, None] + 2, px[None, :] + 1].astype(int) - luma[0][py[:, None], px[None, :]].astype(int)).sum()
    assert got["cost"][1] == want and got["offset"][1].tolist() == [0, 0] and got["status"][1] == 1
    assert np.array_equal(got["out"].view(np.uint32), boxes.view(np.uint32))


def test_no_anchor_within_reach_is_copied():
    boxes = np.tile(np.array(BOX, dtype=F32), (9, 1))
    anchor = [1, 0, 0, 0, 0, 0, 0, 0, 1]
    got = follow_ref(_flat(9), boxes, anchor, reach=3)
    assert got["status"].tolist() == [0, 1, 1, 1, 0, 1, 1, 1, 0]  # frame 4 is 4 frames from either anchor
    assert follow_ref(_flat(9), boxes, anchor, reach=4)["status"][4] == 1
    assert (follow_ref(_flat(9), boxes, np.zeros(9), reach=64)["status"] == 0).all()


def test_anchor_choice():
    boxes = np.tile(np.array(BOX, dtype=F32), (9, 1, 1)).reshape(9, 1, 4)
    anchor = np.array([1, 0, 1, 0, 0, 0, 1, 0, 1])
    assert find_anchor(boxes, anchor, 3, 0, 3) == 2    # the nearer one
    assert find_anchor(boxes, anchor, 5, 0, 3) == 6
    assert find_anchor(boxes, anchor, 4, 0, 3) == 2    # equally near: the earlier one
    nan = boxes.copy()
    nan[2, 0, 1] = np.nan
    assert find_anchor(nan, anchor, 3, 0, 3) == 0      # an anchor with a NaN box is skipped for the next: t - 3 before t + 3
    assert find_anchor(nan, anchor, 4, 0, 3) == 6
    nan[0, 0, 0] = np.inf
    assert find_anchor(nan, anchor, 1, 0, 1) is None and find_anchor(nan, anchor, 1, 0, 5) == 6
    shot = np.array([0, 0, 0, 1, 1, 1, 1, 1, 1])
    assert find_anchor(boxes, anchor, 3, 0, 3, shot) == 6  # frame 2 is nearer, in another shot
    assert find_anchor(boxes, anchor, 3, 0, 2, shot) is None
    assert find_anchor(boxes, anchor, 1, 0, 3, shot) == 0
    # the template comes from the chosen frame: frame 2 and frame 6 show different pictures
    luma = _flat(9)
    luma[6:] = 200
    luma[3] = 190
    one, two = follow_ref(luma, boxes, anchor, radius=1), follow_ref(luma, boxes, anchor, shot=shot, radius=1)
    assert one["cost"][3, 0] == 256 * (190 - 77) and one["status"][3, 0] == 2
    assert two["cost"][3, 0] == 256 * 10 and two["status"][3, 0] == 1


def test_anchor_box_outside_the_frame_and_partly_outside():
    rng = np.random.default_rng(2)
    luma = rng.integers(0, 256, (2, 20, 30), dtype=np.uint8)
    for outside in ([30, 2, 40, 10], [-12, 2, 0, 10], [3, 20, 9, 31], [3, -9, 9, 0], [4, 4, 4, 9]):
        boxes = np.array([outside, [5, 4, 21, 16]], dtype=F32)
        got = follow_ref(luma, boxes, [1, 0])
        assert got["status"].tolist() == [0, 0] and got["cost"].tolist() == [0, 0] and np.array_equal(got["out"].view(np.uint32), boxes.view(np.uint32))
    assert sample_points([30, 2, 40, 10], 20, 30) is None
    py, px = sample_points([-10, -6, 6, 26], 20, 30)  # clamped to [0, 6) x [0, 20): the template comes from the part in the frame
    assert px.tolist() == [(2 * j + 1) * 6 // 32 for j in range(16)] and py.tolist() == [(2 * i + 1) * 20 // 32 for i in range(16)]
    assert px.min() == 0 and px.max() == 5 and py.max() == 19
    boxes = np.array([[-10, -6, 6, 26], [-10, -6, 6, 26]], dtype=F32)
    still = np.stack([luma[0], luma[0]])
    got = follow_ref(still, boxes, [1, 0])
    assert got["status"][1] == 1 and got["cost"][1] == 0 and got["offset"][1].tolist() == [0, 0]


def test_a_one_pixel_box_samples_one_pixel_256_times():
    luma = _flat(2)
    luma[0, 7, 9] = 10
    luma[1, 9, 6] = 10   # the pixel moved by (dy, dx) = (2, -3)
    boxes = np.array([[9, 7, 10, 8], [9, 7, 10, 8]], dtype=F32)
    py, px = sample_points([9, 7, 10, 8], 20, 30)
    assert (py == 7).all() and (px == 9).all()
    got = follow_ref(luma, boxes, [1, 0], radius=4)
    assert got["offset"][1].tolist() == [2, -3] and got["cost"][1] == 0 and got["status"][1] == 1
    assert got["out"][1].tolist() == [6, 9, 7, 10]
    assert follow_ref(luma, boxes, [1, 0], radius=2, accept=(66, 1))["cost"][1] == 256 * 67  # out of reach: every candidate sees 77 for 10


def test_a_shift_over_the_edge_reads_the_clamped_pixels():
    rng = np.random.default_rng(3)
    luma = rng.integers(0, 256, (2, 20, 30), dtype=np.uint8)
    boxes = np.array([[2, 2, 14, 12], [-40, -30, -28, -20]], dtype=F32)  # predicted shift (dy, dx) = (-32, -42): every sample lands on pixel (0, 0) ...
    got = follow_ref(luma, boxes, [1, 0], radius=2, accept=(255, 1))
    py, px = sample_points([2, 2, 14, 12], 20, 30)
    tem = luma[0][py[:, None], px[None, :]].astype(int)
    assert got["cost"][1] == np.abs(int(luma[1, 0, 0]) - tem).sum() and got["offset"][1].tolist() == [0, 0]
    c = candidate_costs(luma[1], tem, py, px, 14, 24, 2)  # ... and here some of them beyond the far corner
    yy, xx = np.clip(py + 14 + 2, 0, 19), np.clip(px + 24 - 1, 0, 29)
    assert c[4, 1] == np.abs(luma[1][yy[:, None], xx[None, :]].astype(int) - tem).sum() and (xx == 29).any() and (yy == 19).any()


def test_accept_exactly_met_is_accepted():
    luma = _flat(2)
    luma[1] = 77 + 24
    boxes = np.array([BOX, BOX], dtype=F32)
    assert follow_ref(luma, boxes, [1, 0], accept=24)["status"][1] == 1
    assert follow_ref(luma, boxes, [1, 0], accept=(24, 1))["cost"][1] == 24 * 256
    assert follow_ref(luma, boxes, [1, 0], accept=(47, 2))["status"][1] == 2
    assert follow_ref(luma, boxes, [1, 0], accept=(48, 2))["status"][1] == 1
    assert follow_ref(luma, boxes, [1, 0], accept=0)["status"][1] == 2 and follow_ref(_flat(2), boxes, [1, 0], accept=0)["status"][1] == 1


def test_luma_of_the_three_formats():
    rng = np.random.default_rng(4)
    Y = rng.integers(0, 256, (2, 5, 7), dtype=np.uint8)
    assert np.array_equal(luma_of_planes((Y, None, None), "yuv420p"), Y) and np.array_equal(luma_of_planes((Y, None), "nv12"), Y)
    assert luma_of_rgb(np.array([[255, 255, 255], [0, 0, 0], [255, 0, 0], [0, 255, 0], [0, 0, 255], [1, 2, 3]], dtype=np.uint8)).tolist() == [255, 0, 77, 149, 29, 2]
    rgb = rng.integers(0, 256, (2, 5, 7, 3), dtype=np.uint8)
    assert luma_of_planes(rgb, "rgb24").shape == (2, 5, 7)


# ---- the binding ----------------------------------------------------------------------------------------------------------------
def test_exports_and_abi():
    from tubedetr_amd import _hip
    from tubedetr_amd.render import _JOB_TYPES

    assert "td_tube_follow" in _hip.EXPORTS and "td_tube_follow_table_bytes" in _hip.EXPORTS
    assert _hip.EXPECTED_ABI == 11 and _hip.lib().td_abi_version() == 11
    assert _JOB_TYPES["td_tube_follow"] == "FollowJob"
    assert _hip.lib().td_tube_follow_table_bytes(0) == 0 and _hip.lib().td_tube_follow_table_bytes(1) % 256 == 0 and _hip.lib().td_tube_follow_table_bytes(1) > 0


def test_ctypes_mirror_size_and_field_order():
    from tubedetr_amd import _hip

    assert [f[0] for f in _hip.FollowJob._fields_] == ["src0", "src1", "src2", "src_frame_stride", "src_pitch0", "src_pitch1", "src_pitch2", "fmt", "T", "sh", "sw", "K", "boxes",
                                                       "anchor", "shot", "radius", "reach", "accept_num", "accept_den", "out", "offset", "cost", "status"]
    assert ctypes.sizeof(_hip.FollowJob) == 136
    assert _hip.FollowJob.src_frame_stride.offset == 24 and _hip.FollowJob.fmt.offset == 44 and _hip.FollowJob.boxes.offset == 64
    assert _hip.FollowJob.radius.offset == 88 and _hip.FollowJob.out.offset == 104 and _hip.FollowJob.status.offset == 128


# ---- refusals -------------------------------------------------------------------------------------------------------------------
def _with(job, **fields):
    for k, v in fields.items():
        setattr(job, k, v)
    return job


def _job(fmt="yuv420p", **kw):
    from tubedetr_amd.render import follow_job

    args = dict(src=SRC, T=T, sh=SH, sw=SW, boxes=OUT, anchor=OUT + 4096, out=OUT + 8192, K=2, pix_fmt=fmt, shot=OUT + 12288, offset=OUT + 16384, cost=OUT + 20480,
                status=OUT + 24576)
    args.update(kw)
    return follow_job(**args)


def _call(jobs, n_jobs=None, host=True, dev=4096, nbytes=4096):
    from tubedetr_amd import _hip

    L = _hip.lib()
    table = ctypes.create_string_buffer(4096)
    arr = (_hip.FollowJob * max(len(jobs), 1))(*jobs)
    n = len(jobs) if n_jobs is None else n_jobs
    rc = L.td_tube_follow(arr, n, ctypes.addressof(table) if host else None, ctypes.c_void_p(dev) if dev else None, nbytes, None)
    return rc, L.td_last_error().decode()


REFUSALS = {
    "fmt": (dict(fmt=7), "job 0: unknown fmt 7"),
    "T<0": (dict(T=-1), "job 0: negative frame count T = -1"),
    "sh=0": (dict(sh=0), "job 0: sh x sw = 0 x 8 outside 1..16384"),
    "sw>max": (dict(sw=16385), "job 0: sh x sw = 6 x 16385 outside 1..16384"),
    "K=0": (dict(K=0), "job 0: K = 0 outside 1..8"),
    "K=9": (dict(K=9), "job 0: K = 9 outside 1..8"),
    "radius<0": (dict(radius=-1), "job 0: radius = -1 outside 0..16"),
    "radius>max": (dict(radius=17), "job 0: radius = 17 outside 0..16"),
    "reach=0": (dict(reach=0), "job 0: reach = 0 outside 1..64"),
    "reach>max": (dict(reach=65), "job 0: reach = 65 outside 1..64"),
    "accept_num<0": (dict(accept_num=-1), "job 0: accept_num = -1 outside 0..1048576"),
    "accept_num>max": (dict(accept_num=(1 << 20) + 1), "job 0: accept_num = 1048577 outside 0..1048576"),
    "accept_den=0": (dict(accept_den=0), "job 0: accept_den = 0 outside 1..1048576"),
    "accept_den>max": (dict(accept_den=(1 << 20) + 1), "job 0: accept_den = 1048577 outside 1..1048576"),
    "boxes null": (dict(boxes=None), "job 0: boxes is null"),
    "anchor null": (dict(anchor=None), "job 0: anchor is null"),
    "out null": (dict(out=None), "job 0: out is null"),
    "src0 null": (dict(src0=None), "job 0: src0 is null"),
    "src1 null": (dict(src1=None), "job 0: src1 is null"),
    "src2 null": (dict(src2=None), "job 0: src2 is null"),
    "pitch0": (dict(src_pitch0=7), "job 0: src_pitch0 = 7 is below its row of 8 bytes"),
    "pitch1": (dict(src_pitch1=3), "job 0: src_pitch1 = 3 is below its row of 4 bytes"),
    "pitch2": (dict(src_pitch2=3), "job 0: src_pitch2 = 3 is below its row of 4 bytes"),
    "stride, plane 0": (dict(src_frame_stride=47), "job 0: src_frame_stride 47 is smaller than plane 0 needs (6 rows of pitch 8)"),
    "stride, plane 2": (dict(src_pitch2=100), "job 0: src_frame_stride 72 is smaller than plane 2 needs (3 rows of pitch 100)"),
}
WORKSPACE = {
    "no host table": (dict(host=False), "td_tube_follow: job-table workspace missing or smaller than td_tube_follow_table_bytes(1)"),
    "no device table": (dict(dev=0), "td_tube_follow: job-table workspace missing or smaller than td_tube_follow_table_bytes(1)"),
    "table one byte short": (None, "td_tube_follow: job-table workspace missing or smaller than td_tube_follow_table_bytes(1)"),
    "n_jobs=0": (dict(n_jobs=0), "td_tube_follow: no jobs (or more than 65536)"),
    "more than 65536 jobs": (dict(n_jobs=65537), "td_tube_follow: no jobs (or more than 65536)"),
}


@pytest.mark.parametrize("key", list(REFUSALS))
def test_tube_follow_refusal(key):
    fields, text = REFUSALS[key]
    rc, msg = _call([_with(_job(), **fields)])
    assert rc != 0 and msg == "td_tube_follow: " + text


def test_plane_refusals_of_the_other_formats():
    rc, msg = _call([_with(_job("nv12"), src1=None)])
    assert rc != 0 and msg == "td_tube_follow: job 0: src1 is null"
    rc, msg = _call([_with(_job("nv12"), src_pitch1=7)])
    assert rc != 0 and msg == "td_tube_follow: job 0: src_pitch1 = 7 is below its row of 8 bytes"
    rc, msg = _call([_with(_job("rgb24"), src_pitch0=23)])
    assert rc != 0 and msg == "td_tube_follow: job 0: src_pitch0 = 23 is below its row of 24 bytes"
    rc, msg = _call([_with(_job("rgb24", T=0), src1=None, src2=None)])  # rgb24 has one plane
    assert rc == 0, msg


@pytest.mark.parametrize("key", list(WORKSPACE))
def test_workspace_refusal(key):
    from tubedetr_amd import _hip

    kw, text = WORKSPACE[key]
    if kw is None:
        kw = dict(nbytes=int(_hip.lib().td_tube_follow_table_bytes(1)) - 1)
    rc, msg = _call([_job()], **kw)
    assert rc != 0 and msg == text


def test_a_later_job_is_checked_and_jobs_without_frames_launch_nothing():
    rc, msg = _call([_job(T=0), _with(_job(), radius=17)])
    assert rc != 0 and msg == "td_tube_follow: job 1: radius = 17 outside 0..16"
    for fmt in ("rgb24", "yuv420p", "nv12"):  # checked like any other, then skipped: TD_OK with a null stream and without a device
        for n in (1, 3):
            rc, msg = _call([_job(fmt, T=0, shot=None, offset=None, cost=OUT if i else None, status=None) for i in range(n)])
            assert rc == 0, msg


def test_python_refusals_come_before_the_device():
    from tubedetr_amd import render

    with pytest.raises(ValueError, match="radius = 17"):
        render.follow_job(SRC, 2, 6, 8, OUT, OUT, OUT, radius=17)
    with pytest.raises(ValueError, match="reach = 0"):
        render.follow_job(SRC, 2, 6, 8, OUT, OUT, OUT, reach=0)
    with pytest.raises(ValueError, match="accept denominator = 0"):
        render.follow_job(SRC, 2, 6, 8, OUT, OUT, OUT, accept=(24, 0))
    with pytest.raises(ValueError, match="K = 9"):
        render.follow_job(SRC, 2, 6, 8, OUT, OUT, OUT, K=9)
    with pytest.raises(ValueError, match="device addresses"):
        render.follow_job(SRC, 2, 6, 8, OUT, None, OUT)
    with pytest.raises(ValueError, match="pix_fmt 'gray'"):
        render.follow_job(SRC, 2, 6, 8, OUT, OUT, OUT, pix_fmt="gray")
    j = render.follow_job(SRC, 2, 6, 8, OUT, OUT, OUT, accept=(7, 2))
    assert (j.accept_num, j.accept_den, j.radius, j.reach, j.K, j.shot, j.status) == (7, 2, 8, 3, 1, None, None)
    assert render.follow_job(SRC, 2, 6, 8, OUT, OUT, OUT).accept_num == 24
    # follow: the scalars are refused whatever the frames are, so a host without a device gives the same messages
    for kw, text in ((dict(radius=-1), "radius = -1"), (dict(radius=1.5), "radius = 1.5"), (dict(reach=65), "reach = 65"), (dict(accept=-1), "accept numerator = -1"),
                     (dict(accept=(1, 2, 3)), "accept \\(1, 2, 3\\)"), (dict(accept=(1, 0)), "accept denominator = 0"), (dict(accept=1 << 21), "accept numerator = 2097152")):
        with pytest.raises(ValueError, match=text):
            render.follow(object(), None, None, **kw)
    with pytest.raises(ValueError, match="frames: DeviceFrames"):
        render.follow(object(), None, None)
    with pytest.raises(ValueError, match="radius: 3 entries for 2 clips"):
        render.follow([object(), object()], None, None, radius=[1, 2, 3])
    assert render.follow([], None, None) == []
    for kw, text in ((dict(T=-1), "T = -1"), (dict(T=None), "T = None"), (dict(T=4, step=0), "step = 0"), (dict(T=4, t0=1 << 24), "t0 = 16777216"),
                     (dict(T=4, first=-(1 << 24)), "first = -16777216"), (dict(T=4, row_frame=[0, 1.5]), "row_frame entry = 1.5"), (dict(T=4, n_tube=0), "n_tube = 0")):
        with pytest.raises(ValueError, match=text):
            render.anchors(**kw)
