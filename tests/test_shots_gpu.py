"""td_frame_stats, td_shot_cuts and tubedetr_amd.render.shot_cuts on the GPU, against the numpy restatement of the header's rules
(tests/shots_ref.py).  Every comparison is exact equality of bytes: the rules are integers, there is no tolerance.

Canaries: the outputs of a job lie in ONE buffer of 0xFF bytes, at least 64 of them in front of each output and behind the last,
and the whole buffer is compared - so a result that leans on what the outputs held, or a byte written beside them, shows.  The
padding of pitched source rows and between the planes and frames is random bytes that no result may depend on."""
import numpy as np
import pytest
import torch

from shots_ref import SYNTHETIC_CUTS, frame_stats_ref, luma_of_rgb, shot_cuts_ref, synthetic_clip
from test_overlay_gpu import as_rows, layout, make_planes, place

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GAP = 64


def spec(fmt, T, sh, sw, step=1, pad=3, gap=37, outputs="both", seed=0, planes=None):
    """``pad`` bytes behind every row and ``gap`` bytes in front of every plane: with 3 and 37, rows and frames at odd addresses."""
    return dict(fmt=fmt, T=T, sh=sh, sw=sw, step=step, pad=pad, gap=gap, outputs=outputs, seed=seed, planes=planes)


def luma_of(s, planes):
    return luma_of_rgb(planes) if s["fmt"] == "rgb24" else planes[0]


def out_layout(T, outputs):
    parts = ([("hist", 256 * T)] if outputs != "sad" else []) + ([("sad", 4 * T)] if outputs != "hist" else [])
    offs, o = {}, 0
    for name, size in parts:
        o = (o + GAP + 15) // 16 * 16
        offs[name] = (o, size)
        o += size
    return offs, o + GAP


def run_stats(specs, launches=1):
    """ONE launch (or the same one again) of all specs; asserts every job's whole output buffer against the reference and
    returns, per job, (hist, sad, n) of the reference."""
    from tubedetr_amd.render import stats_job, launch_frame_stats

    dev = torch.device(DEV)
    jobs, keep, checks, refs = [], [], [], []
    for s in specs:
        rng = np.random.default_rng(100 + s["seed"])
        planes = s["planes"] if s["planes"] is not None else make_planes(rng, max(s["T"], 1), s["sh"], s["sw"], s["fmt"])
        want = frame_stats_ref(luma_of(s, planes), s["step"]) if s["T"] else (np.zeros((0, 64), np.uint32), np.zeros(0, np.uint32), 0)
        refs.append(want)
        rows = [r[:s["T"]] for r in as_rows(planes, s["fmt"])]  # (a clip without frames still has planes with addresses)
        lay = layout(rows, s["gap"], s["pad"])
        src = torch.from_numpy(place(rng.integers(0, 256, max(lay["total"], 1), dtype=np.uint8), rows, lay)).to(dev)
        offs, total = out_layout(s["T"], s["outputs"])
        expect = np.full(total, 0xFF, dtype=np.uint8)
        for name, (a, size) in offs.items():
            expect[a:a + size] = np.ascontiguousarray(want[0] if name == "hist" else want[1]).view(np.uint8).reshape(-1)
        out = torch.full((total,), 0xFF, dtype=torch.uint8, device=dev)
        at = lambda name: out.data_ptr() + offs[name][0] if name in offs else None  # noqa: E731
        jobs.append(stats_job(None, s["T"], s["sh"], s["sw"], s["fmt"], s["step"], at("hist"), at("sad"), src_planes=[src.data_ptr() + o for o in lay["offs"]],
                              src_pitches=lay["pitches"], src_frame_stride=lay["stride"]))
        keep.append(src)
        checks.append((out, expect, offs))
    for _ in range(launches):
        tables = launch_frame_stats(jobs, dev)
        torch.cuda.synchronize()
        del tables
        for i, (out, expect, offs) in enumerate(checks):
            got = out.cpu().numpy()
            for name, (a, size) in offs.items():
                bad = int((got[a:a + size].view(np.uint32) != expect[a:a + size].view(np.uint32)).sum())
                assert bad == 0, f"job {i} {specs[i]['fmt']} {specs[i]['sh']} x {specs[i]['sw']} step {specs[i]['step']}: {bad} of {size // 4} words of {name} differ from the reference"
            assert np.array_equal(got, expect), f"job {i}: a byte outside the outputs was written"
    return refs


@pytest.mark.parametrize("fmt", ["rgb24", "yuv420p", "nv12"])
def test_frame_stats_sizes_that_take_every_path(fmt):
    run_stats([
        spec(fmt, 3, 7, 9, seed=1),                  # odd sizes: one partial unit per row, rows at odd addresses
        spec(fmt, 2, 3, 4101, seed=2),               # a row longer than one workgroup's lanes
        spec(fmt, 2, 67, 40, seed=3),                # more rows than lanes per unit column, units of 16, 16 and 8 pixels
        spec(fmt, 2, 131, 260, seed=4),              # more units than one band holds, for luma and for rgb24
        spec(fmt, 3, 16, 64, pad=0, gap=64, seed=5), # tight rows at 16-byte addresses: every load is the wide one ...
        spec(fmt, 3, 9, 20, pad=0, gap=36, seed=6),  # ... at 4-byte addresses: four dwords
        spec(fmt, 70, 5, 20, seed=7),                # more frames than one segment: the second one fetches frame 63 again
    ])


@pytest.mark.parametrize("step", [1, 3, 8])
def test_frame_stats_steps_that_divide_neither_side(step):
    refs = run_stats([spec(fmt, 3, sh, sw, step=step, seed=10 + i) for i, (fmt, sh, sw) in enumerate(
        [("rgb24", 29, 43), ("yuv420p", 29, 43), ("nv12", 67, 43), ("yuv420p", 7, 9), ("rgb24", 3, 4101), ("nv12", 131, 260)])])
    assert refs[0][2] == -(-29 // step) * -(-43 // step)


def test_frame_stats_frame_counts_and_one_output_only():
    run_stats([spec("yuv420p", T, 12, 33, seed=20 + T) for T in (0, 1, 2, 9)] + [spec("rgb24", T, 12, 33, seed=30 + T) for T in (0, 1, 2, 9)]
              + [spec("nv12", 4, 30, 50, outputs="hist", seed=40), spec("nv12", 4, 30, 50, outputs="sad", seed=40),
                 spec("rgb24", 4, 30, 50, step=2, outputs="hist", seed=41), spec("rgb24", 4, 30, 50, step=2, outputs="sad", seed=41)])


def test_frame_stats_five_mixed_jobs_in_one_launch_twice_the_same_bits():
    flat = (np.full((3, 40, 70), 200, dtype=np.uint8), np.zeros((3, 20, 35), np.uint8), np.zeros((3, 20, 35), np.uint8))  # every pixel in ONE bin
    refs = run_stats([spec("rgb24", 4, 21, 37, seed=50), spec("yuv420p", 3, 40, 70, planes=flat), spec("nv12", 9, 7, 9, step=3, seed=52),
                      spec("yuv420p", 0, 8, 8, seed=53), spec("rgb24", 2, 64, 48, step=8, seed=54)], launches=2)
    assert refs[1][0][0, 50] == 2800 and refs[1][1].tolist() == [0, 0, 0]


# ---- td_shot_cuts -----------------------------------------------------------------------------------------------------------------
def random_stats(T, n, seed):
    """Statistics with a few real changes: the histogram keeps its shape, drifts, and now and then is drawn anew."""
    rng = np.random.default_rng(seed)
    hist = np.zeros((T, 64), dtype=np.uint32)
    for t in range(T):
        if t == 0 or rng.random() < 0.08:
            w = rng.dirichlet(np.full(64, 0.3))
        elif rng.random() < 0.5:
            w = 0.9 * w + 0.1 * rng.dirichlet(np.full(64, 0.3))
        hist[t] = rng.multinomial(n, w)
    sad = rng.integers(0, 24 * n, T).astype(np.uint32)
    if T:
        sad[0] = 0
    return hist, sad


def run_cuts(cases):
    """ONE launch; case: (hist, sad, n, thresholds of shot_cuts_ref).  Compares d, cut, shot and n_shots, and their surroundings."""
    from tubedetr_amd.render import cuts_job, launch_shot_cuts

    dev = torch.device(DEV)
    jobs, keep, checks = [], [], []
    for hist, sad, n, thr in cases:
        T = hist.shape[0]
        want = shot_cuts_ref(hist, sad, n, **thr)
        parts = [("d", want["d"].astype(np.uint32)), ("cut", want["cut"].astype(np.uint8)), ("shot", want["shot"].astype(np.int32)), ("n_shots", np.array([want["n_shots"]], np.int32))]
        offs, o = {}, 0
        for name, a in parts:
            o = (o + GAP + 15) // 16 * 16
            offs[name] = o
            o += a.nbytes
        expect = np.full(o + GAP, 0xFF, dtype=np.uint8)
        for name, a in parts:
            expect[offs[name]:offs[name] + a.nbytes] = a.view(np.uint8)
        out = torch.full((o + GAP,), 0xFF, dtype=torch.uint8, device=dev)
        h = torch.from_numpy(np.ascontiguousarray(hist).view(np.int32).reshape(-1).copy() if T else np.zeros(1, np.int32)).to(dev)
        s = torch.from_numpy(sad.view(np.int32).copy() if T else np.zeros(1, np.int32)).to(dev)
        jobs.append(cuts_job(h.data_ptr(), s.data_ptr(), T, n, out.data_ptr() + offs["cut"], out.data_ptr() + offs["shot"], out.data_ptr() + offs["n_shots"],
                             out.data_ptr() + offs["d"], hist_thr=thr.get("hist_thr", (1, 4)), sad_thr=thr.get("sad_thr", (8, 1)), peak=thr.get("peak", (3, 1)), window=thr.get("w", 4)))
        keep.append((h, s))
        checks.append((out, expect, want))
    tables = launch_shot_cuts(jobs, dev)
    torch.cuda.synchronize()
    del tables
    for i, (out, expect, want) in enumerate(checks):
        assert np.array_equal(out.cpu().numpy(), expect), f"case {i}: cuts {np.nonzero(want['cut'])[0].tolist()} expected"
    return [c[2] for c in checks]


THRESHOLDS = [dict(), dict(hist_thr=(1, 8), sad_thr=(2, 1), peak=(3, 2), w=2), dict(hist_thr=(0, 1), sad_thr=(0, 1), peak=(0, 1), w=0), dict(hist_thr=(1, 4), sad_thr=(8, 1), peak=(1, 1), w=16),
              dict(hist_thr=(3, 16), sad_thr=(12, 1), peak=(5, 2), w=7)]


def test_shot_cuts_on_the_synthetic_clip_and_on_random_statistics():
    cases = []
    for step in (1, 2, 3):
        hist, sad, n = frame_stats_ref(synthetic_clip(), step)
        cases.append((hist, sad, n, dict()))
    for i, thr in enumerate(THRESHOLDS):
        for T in (1, 2, 300, 257):  # 300 and 257: longer than one workgroup's lanes, the second chunk with 44 frames and with one
            cases.append((*random_stats(T, 3000, 60 + 5 * i + T % 5), 3000, thr))
    cases.append((np.zeros((0, 64), np.uint32), np.zeros(0, np.uint32), 100, dict()))
    got = run_cuts(cases)
    for w in got[:3]:
        assert np.nonzero(w["cut"])[0].tolist() == SYNTHETIC_CUTS
    assert sum(w["n_shots"] > 3 for w in got[3:]) >= 8 and got[-1]["n_shots"] == 0  # the random cases do cut


# ---- end to end ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("step", [1, 2, 3])
def test_shot_cuts_end_to_end_from_the_pixels(step):
    from tubedetr_amd.render import DeviceFrames, FrameStats, frame_stats, shot_cuts

    dev = torch.device(DEV)
    luma = synthetic_clip()
    T, sh, sw = luma.shape
    rng = np.random.default_rng(7)
    yuv = np.concatenate([np.concatenate([luma[t].reshape(-1), rng.integers(0, 256, 2 * (sh // 2) * (sw // 2), dtype=np.uint8)]) for t in range(T)])
    clips = [DeviceFrames(torch.from_numpy(yuv).to(dev), T, sh, sw, "yuv420p"), DeviceFrames(torch.from_numpy(np.repeat(luma[..., None], 3, -1).copy()).to(dev), T, sh, sw, "rgb24"),
             DeviceFrames(torch.from_numpy(yuv[:0].copy()).to(dev), 0, sh, sw, "nv12")]
    hist, sad, n = frame_stats_ref(luma, step)
    want = shot_cuts_ref(hist, sad, n)
    shots = shot_cuts(clips, step=step)
    stats = frame_stats(clips[0], step)
    again = shot_cuts(stats)
    assert isinstance(stats, FrameStats) and stats.n == n
    assert np.array_equal(stats.hist.cpu().numpy().view(np.uint32), hist) and np.array_equal(stats.sad.cpu().numpy().view(np.uint32), sad)
    for s in (shots[0], shots[1], again):
        assert np.nonzero(s.cut.cpu().numpy())[0].tolist() == SYNTHETIC_CUTS
        assert np.array_equal(s.cut.cpu().numpy().astype(np.uint8), want["cut"]) and np.array_equal(s.shot.cpu().numpy(), want["shot"])
        assert np.array_equal(s.d.cpu().numpy().view(np.uint32), want["d"]) and s.count.item() == want["n_shots"] == 4
    assert shots[2].cut.shape == (0,) and shots[2].shot.shape == (0,) and shots[2].count.item() == 0
