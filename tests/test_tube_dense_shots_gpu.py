"""td_tube_densify_shots and tubedetr_amd.render.densify(shots=...) on the GPU, bit for bit against the numpy restatement of
the header's rule (tests/shots_ref.py over tests/tube_dense_ref.py): fp32 outputs as their bit patterns, the rest as bytes.
All outputs of a job lie in ONE buffer of random bytes, with at least 64 of them around each, and the whole buffer is compared.
With no shot array, and with an array that holds one shot, the bytes are td_tube_densify's on the same jobs."""
import numpy as np
import pytest
import torch

from shots_ref import densify_shots_ref
from test_tube_dense_gpu import gaps, tube

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
MODES = ["hold", "lerp", "hull"]
GAP = 64
MAP = (5, 7)


def shots_from_cuts(n, cuts):
    s = np.zeros(n, dtype=np.int32)
    for c in cuts:
        s[c:] += 1
    return s


def run(specs, entry="shots", check=True):
    """ONE launch of all specs (the keyword arguments of densify_shots_ref).  entry "shots": td_tube_densify_shots with every
    spec's array; "null": the same entry point with a NULL shots argument; "plain": td_tube_densify.  Returns every job's buffer."""
    from tubedetr_amd import _hip
    from tubedetr_amd.render import dense_job, tube_densify, tube_densify_shots

    dev = torch.device(DEV)
    rng = np.random.default_rng(5)
    jobs, shots, keep, checks = [], [], [], []
    for s in specs:
        boxes = np.asarray(s["boxes"], dtype=np.float32)
        boxes = boxes[:, None, :] if boxes.ndim == 2 else boxes
        n_tube, K = boxes.shape[:2]
        T, heat = s["T"], s.get("heat")
        mb = int(np.prod(heat.shape[1:])) if heat is not None else 0
        parts = [("dense", 16 * T * K, 0), ("valid", T * K, 0), ("span", 16 * K, 0)] + ([("heat", T * mb, 5)] if heat is not None else [])
        offs, o = {}, 0
        for name, size, skew in parts:
            o = (o + GAP + 15) // 16 * 16 + skew
            offs[name] = (o, size)
            o += size
        canary = rng.integers(0, 256, o + GAP, dtype=np.uint8)
        expect = None
        if check:
            want = densify_shots_ref(**s)
            expect = canary.copy()
            for name, (a, size) in offs.items():
                expect[a:a + size] = np.ascontiguousarray(want[name]).view(np.uint8).reshape(-1)
        buf = torch.from_numpy(canary).to(dev)
        t = {"boxes": torch.from_numpy(boxes).to(dev)}
        if s.get("span") is not None:
            t["span"] = torch.tensor(np.asarray(s["span"]).reshape(K, 2), dtype=torch.int64, device=dev)
        if s.get("row_frame") is not None:
            t["row_frame"] = torch.tensor(s["row_frame"], dtype=torch.int32, device=dev)
        if heat is not None:
            t["heat"] = torch.from_numpy(np.ascontiguousarray(heat)).to(dev)
        if s.get("shot") is not None:
            t["shot"] = torch.from_numpy(np.concatenate([np.asarray(s["shot"], dtype=np.int32), np.full(4, 99, np.int32)])).to(dev)  # (entries behind the array are not its)
        at = lambda name: buf.data_ptr() + offs[name][0]  # noqa: E731
        jobs.append(dense_job(t["boxes"].data_ptr(), n_tube, T, at("dense"), K, span=t["span"].data_ptr() if "span" in t else None,
                              row_frame=t["row_frame"].data_ptr() if "row_frame" in t else None, first=s.get("first", 0), step=s.get("step", 1), t0=s.get("t0", 0),
                              heat=t["heat"].data_ptr() if heat is not None else None, heat_hw=heat.shape[1:] if heat is not None else (0, 0), mode=s.get("mode", "lerp"),
                              smooth=s.get("smooth", 0), valid=at("valid"), dense_span=at("span"), dense_heat=at("heat") if heat is not None else None))
        shots.append(_hip.DenseShots(t["shot"].data_ptr(), s.get("shot_t0", 0), len(s["shot"])) if "shot" in t else _hip.DenseShots(None, 0, 0))
        keep.append(t)
        checks.append((buf, expect, offs))
    tables = tube_densify(jobs, dev) if entry == "plain" else tube_densify_shots(jobs, shots if entry == "shots" else None, dev)
    torch.cuda.synchronize()
    del tables
    out = []
    for i, (buf, expect, offs) in enumerate(checks):
        got = buf.cpu().numpy()
        if check:
            for name, (a, size) in offs.items():
                bad = int((got[a:a + size] != expect[a:a + size]).sum())
                assert bad == 0, f"job {i} ({specs[i].get('mode', 'lerp')}): {bad} of {size} bytes of {name} differ from the reference"
            assert np.array_equal(got, expect), f"job {i}: a byte outside the outputs was written"
        out.append((got, offs))
    return out


def cut_out(res, name):
    got, offs = res
    return got[offs[name][0]:offs[name][0] + offs[name][1]]


def base(K, mode, smooth, with_heat, seed):
    """10 rows at frames 4, 10, 16, ... 58 (no table) or at gaps 1, 5, 7 from 4 (a table); 70 dense frames from frame 0."""
    rng = np.random.default_rng(seed)
    boxes = tube(10, K, seed)
    kw = dict(boxes=boxes if K > 1 else boxes[:, 0], T=70, t0=0, mode=mode, smooth=smooth)
    if with_heat:
        kw["heat"] = rng.integers(0, 256, (10,) + MAP, dtype=np.uint8)
    return kw


@pytest.mark.parametrize("smooth", [0, 2])
@pytest.mark.parametrize("mode", MODES)
def test_cuts_between_rows_on_a_row_outside_the_rows_and_twice_in_one_interval(mode, smooth):
    specs = []
    for K, with_heat, seed in ((1, True, 1), (3, False, 2), (3, True, 3)):
        b = dict(base(K, mode, smooth, with_heat, seed), first=4, step=6)  # rows at 4, 10, ..., 58
        specs += [
            dict(b, shot=shots_from_cuts(70, [13])),                # between rows 1 and 2
            dict(b, shot=shots_from_cuts(70, [16])),                # exactly on row 2: the row belongs to the new shot
            dict(b, shot=shots_from_cuts(70, [2])),                 # before the first row
            dict(b, shot=shots_from_cuts(70, [61])),                # after the last row
            dict(b, shot=shots_from_cuts(70, [24, 26])),            # two cuts between rows 3 and 4: frames 24 and 25 are in neither row's shot
            dict(b, shot=shots_from_cuts(70, [5, 11, 13, 30, 31, 47, 58])),
        ]
    t = dict(base(3, mode, smooth, True, 4), row_frame=gaps(10, 4), span=[[0, 9], [2, 6], [5, 12]])  # rows at 4, 5, 10, 17, 18, 23, 30, 31, 36, 43
    t["boxes"] = t["boxes"].copy()
    t["boxes"][3, 0, 1] = np.nan  # an absent row beside a cut: no one-sided hold comes from it
    t["boxes"][6, 2, :] = np.inf
    specs += [dict(t, shot=shots_from_cuts(70, [14])), dict(t, shot=shots_from_cuts(70, [20, 33])), dict(t, shot=shots_from_cuts(70, [17, 18, 19]))]
    run(specs)


@pytest.mark.parametrize("mode", MODES)
def test_an_array_that_covers_part_of_the_frames_and_chunks_that_equal_the_whole(mode):
    b = dict(base(3, mode, 2, True, 6), row_frame=gaps(10, 4))
    whole_shot = shots_from_cuts(70, [8, 21, 40])
    part = dict(b, shot=whole_shot[15:45], shot_t0=15)  # frames before 15 and from 45 on match every shot
    behind = dict(b, shot=whole_shot[:10] + 7, shot_t0=100)  # an array that covers no frame of the job: td_tube_densify's result
    whole, lo, hi, _, alone = run([dict(b, shot=whole_shot), dict(b, T=33, shot=whole_shot), dict(b, T=37, t0=33, shot=whole_shot), part, behind])
    for name in ("dense", "valid", "heat"):
        assert np.array_equal(np.concatenate([cut_out(lo, name), cut_out(hi, name)]), cut_out(whole, name)), name
    plain = run([b], entry="plain", check=False)[0]
    for name in ("dense", "valid", "span", "heat"):
        assert np.array_equal(cut_out(alone, name), cut_out(plain, name)), name


@pytest.mark.parametrize("mode", MODES)
def test_without_shots_and_with_one_shot_the_bytes_are_td_tube_densify_s(mode):
    specs = []
    for K, smooth, with_heat, seed in ((1, 0, True, 11), (3, 2, True, 12), (3, 0, False, 13)):
        b = dict(base(K, mode, smooth, with_heat, seed), row_frame=gaps(10, 4), t0=-3)
        if K == 3:
            b["boxes"] = b["boxes"].copy()
            b["boxes"][4, 1, 0] = np.nan
            b["span"] = [[0, 9], [1, 7], [3, 3]]
        specs.append(b)
    plain = run(specs, entry="plain", check=False)
    null = run(specs, entry="null", check=False)
    no_array = run(specs, entry="shots", check=False)  # every job's shot pointer is NULL
    one_shot = run([dict(s, shot=np.full(90, 3, np.int32), shot_t0=-10) for s in specs], entry="shots")
    for i in range(len(specs)):
        for other in (null, no_array, one_shot):
            assert np.array_equal(other[i][0], plain[i][0]), f"job {i}"


def test_densify_takes_what_shot_cuts_returns():
    from tubedetr_amd.render import Shots, densify

    dev = torch.device(DEV)
    boxes, shot = tube(10, 3, 21), shots_from_cuts(70, [13, 40])
    kw = dict(first=4, step=6, mode="lerp", smooth=1)
    want = densify_shots_ref(boxes=boxes, T=70, shot=shot, **kw)
    b, s = torch.from_numpy(boxes).to(dev), torch.from_numpy(shot).to(dev)
    as_shots = Shots(s > 99, s, torch.zeros(1, dtype=torch.int32, device=dev), s)
    for given in (s, as_shots):
        got = densify(b, 70, shots=given, **kw)
        assert np.array_equal(got.boxes.cpu().numpy().view(np.uint32), want["dense"]) and np.array_equal(got.valid.cpu().numpy().astype(np.uint8), want["valid"])
    lo, hi = densify([b, b], [30, 40], t0=[0, 30], shots=[s, as_shots], **kw)
    assert np.array_equal(np.concatenate([lo.boxes.cpu().numpy(), hi.boxes.cpu().numpy()]).view(np.uint32), want["dense"])
    plain, none = densify(b, 70, **kw), densify([b], 70, shots=[None], **kw)[0]
    assert np.array_equal(plain.boxes.cpu().numpy().view(np.uint32), none.boxes.cpu().numpy().view(np.uint32))
    with pytest.raises(ValueError, match="shots"):
        densify(b, 70, shots=s.long(), **kw)
