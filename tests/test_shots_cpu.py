"""Shot cuts without a device: the numpy restatement of the rules (tests/shots_ref.py) on the synthetic clip and on hand-built
sequences, and every host refusal of td_frame_stats, td_shot_cuts and td_tube_densify_shots through ctypes - nothing is launched
on those paths, so the addresses are made up.  The message texts are part of the interface."""
import ctypes

import numpy as np
import pytest

from shots_ref import (SYNTHETIC_CUTS, conditions, cuts_from_distance, densify_shots_ref, frame_stats_ref, luma_of_rgb, sampled_pixels, shot_cuts_ref,
                       synthetic_clip)
from tube_dense_ref import densify_ref

SRC, OUT = 1 << 20, 1 << 24
T, SH, SW = 2, 6, 8  # yuv420p: Y 6 rows of 8 bytes, U and V 3 rows of 4; 72 bytes per frame


# ---- the rule -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("step", [1, 2, 3])
def test_synthetic_clip_has_its_three_cuts_at_every_step(step):
    hist, sad, n = frame_stats_ref(synthetic_clip(), step)
    assert n == sampled_pixels(48, 64, step) and (hist.sum(1) == n).all() and sad[0] == 0
    got = shot_cuts_ref(hist, sad, n)
    assert np.nonzero(got["cut"])[0].tolist() == SYNTHETIC_CUTS == [20, 51, 57]
    assert got["n_shots"] == 4 and got["shot"][19] == 0 and got["shot"][20] == 1 and got["shot"][-1] == 3


def test_repeated_frames_have_no_difference_and_a_flash_cuts_once_at_its_first_frame():
    hist, sad, n = frame_stats_ref(synthetic_clip(), 1)
    assert (sad[21:35] == 0).all() and sad[20] > 0  # frames 20 .. 34 show one still picture
    d = shot_cuts_ref(hist, sad, n)["d"]
    assert d[51] == d[52] > 0  # into the flash and out of it: the earliest of the two equal peaks is the cut


def test_luma_of_rgb_is_the_integer_rule():
    assert luma_of_rgb(np.array([[255, 255, 255], [0, 0, 0], [255, 0, 0], [0, 255, 0], [0, 0, 255], [1, 2, 3]], dtype=np.uint8)).tolist() == [255, 0, 77, 149, 29, 2]


N = 1000
QUIET_D, QUIET_SAD = [0, 10, 10, 10, 10, 900, 10, 10, 10, 10], [0] + [9000] * 9  # frame 5: d / 2N = 0.45, sad / N = 9, a lone peak


def test_a_lone_peak_is_a_cut_and_each_condition_fails_alone():
    assert conditions(QUIET_D, QUIET_SAD, N, 5) == (True, True, True, True)
    assert cuts_from_distance(QUIET_D, QUIET_SAD, N)["cut"].tolist() == [0, 0, 0, 0, 0, 1, 0, 0, 0, 0]
    # 1: the histogram gate: d[5] * 4 = 2000 is not above 2 N
    d = list(QUIET_D)
    d[5] = 500
    assert conditions(d, QUIET_SAD, N, 5) == (False, True, True, True)
    # 2: the difference gate: sad[5] = 8 N is not above 8 N
    sad = list(QUIET_SAD)
    sad[5] = 8000
    assert conditions(QUIET_D, sad, N, 5) == (True, False, True, True)
    # 3: a larger neighbour inside the window, small enough to leave the mean alone
    d = [0, 0, 0, 0, 0, 900, 0, 0, 901, 0]
    assert conditions(d, QUIET_SAD, N, 5) == (True, True, False, True)
    # 4: a peak that does not stand out: 8 * 900 is not above 3 * (8 * 300)
    d = [0, 300, 300, 300, 300, 900, 300, 300, 300, 300]
    assert conditions(d, QUIET_SAD, N, 5) == (True, True, True, False)
    for bad_d, bad_sad in ((d, QUIET_SAD), (QUIET_D, sad)):
        assert cuts_from_distance(bad_d, bad_sad, N)["n_shots"] == 1


def test_of_equal_neighbours_the_earliest_wins():
    d, sad = [0, 0, 0, 900, 900, 0, 0, 900, 0, 0], [0] + [9000] * 9
    assert conditions(d, sad, N, 3)[2] and not conditions(d, sad, N, 4)[2] and not conditions(d, sad, N, 7)[2]
    got = cuts_from_distance(d, sad, N, peak=(0, 1))
    assert got["cut"].tolist() == [0, 0, 0, 1, 0, 0, 0, 0, 0, 0] and got["shot"].tolist() == [0, 0, 0, 1, 1, 1, 1, 1, 1, 1]
    # beyond the window both stand: at most one cut per w + 1 frames
    got = cuts_from_distance(d, sad, N, peak=(0, 1), w=2)
    assert got["cut"].tolist() == [0, 0, 0, 1, 0, 0, 0, 1, 0, 0] and got["n_shots"] == 3


def test_window_zero_and_clips_of_no_frame_and_one_frame():
    d, sad = [0, 900, 900, 900], [0, 9000, 9000, 9000]
    assert conditions(d, sad, N, 2, w=0) == (True, True, True, True)  # Q is empty: 3 and 4 hold
    assert cuts_from_distance(d, sad, N, w=0)["cut"].tolist() == [0, 1, 1, 1]
    assert cuts_from_distance([0, 900], [0, 9000], N)["cut"].tolist() == [0, 1]  # T = 2: Q of frame 1 is empty at any w
    none = shot_cuts_ref(np.zeros((0, 64), np.uint32), np.zeros(0, np.uint32), N)
    assert none["n_shots"] == 0 and none["cut"].shape == (0,) and none["shot"].shape == (0,) and none["d"].shape == (0,)
    one = shot_cuts_ref(np.full((1, 64), 5, np.uint32), np.zeros(1, np.uint32), 320)
    assert one["n_shots"] == 1 and one["cut"].tolist() == [0] and one["shot"].tolist() == [0] and one["d"].tolist() == [0]


@pytest.mark.parametrize("mode", ["hold", "lerp", "hull"])
def test_reference_densify_with_one_shot_is_the_reference_without(mode):
    rng = np.random.default_rng(3)
    boxes = rng.uniform(0, 100, (7, 2, 4)).astype(np.float32)
    boxes[3, 1, 2] = np.nan
    heat = rng.integers(0, 256, (7, 3, 2), dtype=np.uint8)
    kw = dict(boxes=boxes, T=40, first=2, step=5, t0=-3, span=[[0, 6], [1, 5]], heat=heat, mode=mode, smooth=1)
    want = densify_ref(**kw)
    for shot, shot_t0 in ((np.zeros(60, np.int32), -10), (np.full(9, 4, np.int32), 11), (np.zeros(0, np.int32), 0)):
        got = densify_shots_ref(shot=shot, shot_t0=shot_t0, **kw)
        for name in ("dense", "valid", "span", "heat"):
            assert np.array_equal(got[name], want[name]), name


def test_reference_densify_stops_at_a_cut():
    boxes = np.array([[0, 0, 10, 10], [100, 100, 110, 110]], dtype=np.float32)
    shot = np.array([0, 0, 0, 1, 1, 1, 1], dtype=np.int32)  # rows at frames 0 and 6, the cut at frame 3
    for mode in ("hold", "lerp", "hull"):
        got = densify_shots_ref(boxes, 7, first=0, step=6, mode=mode, shot=shot)["dense"].view(np.float32)[:, 0]
        assert [row.tolist() for row in got] == [boxes[0].tolist()] * 3 + [boxes[1].tolist()] * 4, mode


# ---- the binding ----------------------------------------------------------------------------------------------------------------
def test_exports_and_abi():
    from tubedetr_amd import _hip

    for name in ("td_frame_stats", "td_frame_stats_table_bytes", "td_shot_cuts", "td_shot_cuts_table_bytes", "td_tube_densify_shots", "td_tube_densify_shots_table_bytes"):
        assert name in _hip.EXPORTS
    assert _hip.lib().td_tube_densify_shots_table_bytes(5) == _hip.lib().td_tube_densify_table_bytes(5)
    assert _hip.EXPECTED_ABI == 11 and _hip.lib().td_abi_version() == 11
    assert len(_hip._SIGS["td_tube_densify_shots"]) == len(_hip._SIGS["td_tube_densify"]) + 1
    assert ctypes.sizeof(_hip.DenseShots) == 16 and ctypes.sizeof(_hip.StatsJob) == 80 and ctypes.sizeof(_hip.CutsJob) == 88


# ---- refusals -------------------------------------------------------------------------------------------------------------------
def _with(job, **fields):
    for k, v in fields.items():
        setattr(job, k, v)
    return job


def _stats(fmt="yuv420p", **kw):
    from tubedetr_amd.render import stats_job

    args = dict(src=SRC, T=T, sh=SH, sw=SW, pix_fmt=fmt, step=1, hist=OUT, sad=OUT + 4096)
    args.update(kw)
    return stats_job(**args)


def _cuts(**kw):
    from tubedetr_amd.render import cuts_job

    args = dict(hist=SRC, sad=SRC + 4096, T=T, n=48, cut=OUT, shot=OUT + 64, n_shots=OUT + 128, d=OUT + 192)
    args.update(kw)
    return cuts_job(**args)


def _dense(**kw):
    from tubedetr_amd.render import dense_job

    args = dict(boxes=SRC, n_tube=2, T=T, dense=OUT)
    args.update(kw)
    return dense_job(**args)


def _call(entry, jobs, shots=None, n_jobs=None, host=True, dev=4096, nbytes=4096):
    from tubedetr_amd import _hip

    L = _hip.lib()
    table = ctypes.create_string_buffer(4096)
    kind = {"td_frame_stats": _hip.StatsJob, "td_shot_cuts": _hip.CutsJob, "td_tube_densify_shots": _hip.DenseJob}[entry]
    arr = (kind * max(len(jobs), 1))(*jobs)
    n = len(jobs) if n_jobs is None else n_jobs
    tail = (ctypes.addressof(table) if host else None, ctypes.c_void_p(dev) if dev else None, nbytes, None)
    if entry == "td_tube_densify_shots":
        sarr = (_hip.DenseShots * max(len(jobs), 1))(*(shots or [])) if shots is not None else None
        rc = L.td_tube_densify_shots(arr, sarr, n, *tail)
    else:
        rc = getattr(L, entry)(arr, n, *tail)
    return rc, L.td_last_error().decode()


STATS_REFUSALS = {
    "fmt": (dict(fmt=7), "job 0: unknown fmt 7"),
    "T<0": (dict(T=-1), "job 0: negative frame count T = -1"),
    "sh=0": (dict(sh=0), "job 0: sh x sw = 0 x 8 outside 1..16384"),
    "sw>max": (dict(sw=16385), "job 0: sh x sw = 6 x 16385 outside 1..16384"),
    "pixels": (dict(sh=4097, sw=4096, src_pitch0=4096, src_pitch1=2048, src_pitch2=2048, src_frame_stride=1 << 26),
               "job 0: sh * sw = 16781312 pixels is above 16777216 (sad would not fit 32 bits)"),
    "step=0": (dict(step=0), "job 0: step = 0 outside 1..8"),
    "step=9": (dict(step=9), "job 0: step = 9 outside 1..8"),
    "no output": (dict(hist=None, sad=None), "job 0: hist and sad are both null"),
    "src0 null": (dict(src0=None), "job 0: src0 is null"),
    "src1 null": (dict(src1=None), "job 0: src1 is null"),
    "src2 null": (dict(src2=None), "job 0: src2 is null"),
    "pitch0": (dict(src_pitch0=7), "job 0: src_pitch0 = 7 is below its row of 8 bytes"),
    "pitch1": (dict(src_pitch1=3), "job 0: src_pitch1 = 3 is below its row of 4 bytes"),
    "pitch2": (dict(src_pitch2=3), "job 0: src_pitch2 = 3 is below its row of 4 bytes"),
    "stride, plane 0": (dict(src_frame_stride=47), "job 0: src_frame_stride 47 is smaller than plane 0 needs (6 rows of pitch 8)"),
    "stride, plane 2": (dict(src_pitch2=100), "job 0: src_frame_stride 72 is smaller than plane 2 needs (3 rows of pitch 100)"),
}
CUTS_REFUSALS = {
    "hist": (dict(hist=None), "job 0: hist is null"), "sad": (dict(sad=None), "job 0: sad is null"), "cut": (dict(cut=None), "job 0: cut is null"),
    "shot": (dict(shot=None), "job 0: shot is null"), "n_shots": (dict(n_shots=None), "job 0: n_shots is null"),
    "T<0": (dict(T=-1), "job 0: T = -1 outside 0..1048576"), "T>max": (dict(T=(1 << 20) + 1), "job 0: T = 1048577 outside 0..1048576"),
    "N=0": (dict(N=0), "job 0: N = 0 outside 1..16777216"), "N>max": (dict(N=(1 << 24) + 1), "job 0: N = 16777217 outside 1..16777216"),
    "w<0": (dict(w=-1), "job 0: w = -1 outside 0..16"), "w>max": (dict(w=17), "job 0: w = 17 outside 0..16"),
    "hist_num": (dict(hist_num=-1), "job 0: hist_num = -1 outside 0..1048576"), "hist_den": (dict(hist_den=0), "job 0: hist_den = 0 outside 1..1048576"),
    "sad_num": (dict(sad_num=(1 << 20) + 1), "job 0: sad_num = 1048577 outside 0..1048576"), "sad_den": (dict(sad_den=0), "job 0: sad_den = 0 outside 1..1048576"),
    "peak_num": (dict(peak_num=-1), "job 0: peak_num = -1 outside 0..1048576"), "peak_den": (dict(peak_den=(1 << 20) + 1), "job 0: peak_den = 1048577 outside 1..1048576"),
}
DENSE_REFUSALS = {  # td_tube_densify's, under the new name
    "boxes": (dict(boxes=None), "job 0: boxes is null"), "dense": (dict(dense=None), "job 0: dense is null"), "n_tube": (dict(n_tube=0), "job 0: n_tube = 0 is below 1"),
    "K": (dict(K=9), "job 0: K = 9 outside 1..8"), "T": (dict(T=-1), "job 0: T = -1 outside 0..1048576"), "t0": (dict(t0=(1 << 23) + 1), "job 0: t0 = 8388609 outside +-8388608"),
    "first": (dict(first=-(1 << 23) - 1), "job 0: first = -8388609 outside +-8388608"), "step": (dict(step=0), "job 0: step = 0 outside 1..65536"),
    "smooth": (dict(smooth=17), "job 0: smooth = 17 outside 0..16"), "mode": (dict(mode=3), "job 0: unknown mode 3"),
    "heat alone": (dict(heat=SRC), "job 0: heat is given but dense_heat is null"), "dense_heat alone": (dict(dense_heat=SRC), "job 0: dense_heat is given but heat is null"),
    "map": (dict(heat=SRC, dense_heat=OUT, mh=0, mw=3), "job 0: mh x mw = 0 x 3 outside 1..256"),
}
WORKSPACE = {
    "no host table": (dict(host=False), "{who}: job-table workspace missing or smaller than {table}_table_bytes(1)"),
    "no device table": (dict(dev=0), "{who}: job-table workspace missing or smaller than {table}_table_bytes(1)"),
    "table one byte short": (None, "{who}: job-table workspace missing or smaller than {table}_table_bytes(1)"),
    "n_jobs=0": (dict(n_jobs=0), "{who}: no jobs (or more than 65536)"), "more than 65536 jobs": (dict(n_jobs=65537), "{who}: no jobs (or more than 65536)"),
}


@pytest.mark.parametrize("key", list(STATS_REFUSALS))
def test_frame_stats_refusal(key):
    fields, text = STATS_REFUSALS[key]
    rc, msg = _call("td_frame_stats", [_with(_stats(), **fields)])
    assert rc != 0 and msg == "td_frame_stats: " + text


@pytest.mark.parametrize("key", list(CUTS_REFUSALS))
def test_shot_cuts_refusal(key):
    fields, text = CUTS_REFUSALS[key]
    rc, msg = _call("td_shot_cuts", [_with(_cuts(), **fields)])
    assert rc != 0 and msg == "td_shot_cuts: " + text


@pytest.mark.parametrize("key", list(DENSE_REFUSALS))
def test_densify_shots_refusal(key):
    from tubedetr_amd import _hip

    fields, text = DENSE_REFUSALS[key]
    for shots in (None, [_hip.DenseShots(None, 0, 0)], [_hip.DenseShots(SRC, 0, 5)]):
        rc, msg = _call("td_tube_densify_shots", [_with(_dense(), **fields)], shots)
        assert rc != 0 and msg == "td_tube_densify_shots: " + text


def test_densify_shots_refuses_its_own_fields_only_with_a_shot_array():
    from tubedetr_amd import _hip

    for shots, text in (([_hip.DenseShots(SRC, 0, -1)], "job 0: shot_T = -1 outside 0..1048576"), ([_hip.DenseShots(SRC, 0, (1 << 20) + 1)], "job 0: shot_T = 1048577 outside 0..1048576"),
                        ([_hip.DenseShots(SRC, (1 << 23) + 1, 4)], "job 0: shot_t0 = 8388609 outside +-8388608"),
                        ([_hip.DenseShots(SRC, -(1 << 23) - 1, 4)], "job 0: shot_t0 = -8388609 outside +-8388608")):
        rc, msg = _call("td_tube_densify_shots", [_dense()], shots)
        assert rc != 0 and msg == "td_tube_densify_shots: " + text
    # without an array the two numbers mean nothing; the next check (here: of job 1) is reached
    rc, msg = _call("td_tube_densify_shots", [_dense(), _with(_dense(), K=9)], [_hip.DenseShots(None, 1 << 30, -5), _hip.DenseShots(None, 0, 0)])
    assert rc != 0 and msg == "td_tube_densify_shots: job 1: K = 9 outside 1..8"


@pytest.mark.parametrize("entry,table", [("td_frame_stats", "td_frame_stats"), ("td_shot_cuts", "td_shot_cuts"), ("td_tube_densify_shots", "td_tube_densify_shots")])
@pytest.mark.parametrize("key", list(WORKSPACE))
def test_workspace_refusal(entry, table, key):
    from tubedetr_amd import _hip

    kw, text = WORKSPACE[key]
    if kw is None:
        kw = dict(nbytes=int(getattr(_hip.lib(), entry + "_table_bytes")(1)) - 1)
    job = {"td_frame_stats": _stats, "td_shot_cuts": _cuts, "td_tube_densify_shots": _dense}[entry]()
    rc, msg = _call(entry, [job], **kw)
    assert rc != 0 and msg == text.format(who=entry, table=table)


def test_a_later_job_is_checked_and_jobs_without_frames_launch_nothing():
    rc, msg = _call("td_frame_stats", [_stats(T=0), _with(_stats(), step=9)])
    assert rc != 0 and msg == "td_frame_stats: job 1: step = 9 outside 1..8"
    for fmt in ("rgb24", "yuv420p", "nv12"):  # checked like any other, then skipped: TD_OK with a null stream and without a device
        for n in (1, 3):
            rc, msg = _call("td_frame_stats", [_stats(fmt, T=0, hist=OUT if i else None) for i in range(n)])
            assert rc == 0, msg


def test_python_refusals_come_before_the_device():
    from tubedetr_amd import render

    with pytest.raises(ValueError, match="step = 0"):
        render.stats_job(SRC, 2, 6, 8, "yuv420p", 0, OUT, OUT)
    with pytest.raises(ValueError, match="at most 16777216 pixels"):
        render.stats_job(SRC, 2, 4097, 4096, "yuv420p", 1, OUT, OUT)
    with pytest.raises(ValueError, match="at least one of them"):
        render.stats_job(SRC, 2, 6, 8, "yuv420p", 1)
    with pytest.raises(ValueError, match="window = 17"):
        render.cuts_job(SRC, SRC, 2, 48, OUT, OUT, OUT, window=17)
    with pytest.raises(ValueError, match="hist denominator = 0"):
        render.cuts_job(SRC, SRC, 2, 48, OUT, OUT, OUT, hist_thr=(1, 0))
    with pytest.raises(ValueError, match="peak 3"):
        render.shot_cuts([object()], peak=3)
    assert render.sampled_pixels(7, 9, 3) == 9 and render.sampled_pixels(720, 1280, 8) == 90 * 160
