"""Host side of the device-side clip augmentation (tubedetr_amd/augment.py, td_clip_resample): no GPU needed.

* ``plan`` against tests/golden/aug_plans.npz, recorded from the reference's own ``make_video_transforms``
  (tools/gen_golden_aug.py): same seeds -> same output size, boxes, caption, kept boxes per frame.
* the float64 restatement of the sampling rule that the GPU tests compare the kernel with (``resample_f64`` below, built
  from index / weight tables, not from the kernel's code) against ``F.interpolate`` in float64.
* the C ABI: struct mirror, argument validation.

Which rare branches of the random size crop the fixture holds: the whole-image crop WAS found by the generator's search
(tag ``whole-image-crop``) and so was the 100-try fall-back (tag ``cautious-fallback``) - it is not rare at all: in the
reference a try crops the boxes the previous try left behind, so a first draw that drops a box ALWAYS ends in the
fall-back, and "a first crop drops a box, a later one keeps all" cannot happen there (the generator asserts it over
300 seeds).  ``test_a_later_draw_cannot_undo_a_dropped_box`` pins that behaviour of ``plan`` directly with patched draws.
"""
import ctypes
import os
import random
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "aug_plans.npz")


# ---- float64 restatement of the sampling rule (shared with tests/test_augment_gpu.py) ---------------------------------
def taps(n_src: int, n_dst: int, first: int, count: int, flip: bool = False):
    """index pair + float64 weight of output samples first .. first + count - 1 of a resize of n_src samples to n_dst:
    centre c = (v + 0.5) * n_src / n_dst - 0.5 clamped below at 0, i0 = floor(c), i1 = min(i0 + 1, n_src - 1)."""
    v = np.arange(first, first + count, dtype=np.float64)
    c = np.maximum((v + 0.5) * (float(n_src) / float(n_dst)) - 0.5, 0.0)
    # the quotient in exact integers (a float64 floor of c could land on the wrong side of an integer by one ulp)
    num = (2 * np.arange(first, first + count, dtype=np.int64) + 1) * n_src - n_dst
    i0 = np.where(num > 0, num // (2 * n_dst), 0)
    w = np.where(num > 0, (num - i0 * 2 * n_dst) / float(2 * n_dst), 0.0)
    assert np.abs((i0 + w) - c).max() < 1e-9
    i1 = np.minimum(i0 + 1, n_src - 1)
    if flip:
        i0, i1 = n_src - 1 - i0, n_src - 1 - i1
    return i0, i1, w


def resample_f64(src: np.ndarray, rh: int, rw: int, window=None, flip: bool = False) -> np.ndarray:
    """src (..., sh, sw, 3) uint8 -> float64 (..., wh, ww, 3): the UNROUNDED four-tap blend of the window of the virtual
    rh x rw image (uint8 result = floor(value + 0.5))."""
    sh, sw = src.shape[-3], src.shape[-2]
    wy, wx, wh, ww = window if window is not None else (0, 0, rh, rw)
    y0, y1, fy = taps(sh, rh, wy, wh)
    x0, x1, fx = taps(sw, rw, wx, ww, flip)
    s = src.astype(np.float64)
    fy = fy[:, None, None]
    fx = fx[None, :, None]
    top = s[..., y0, :, :][..., :, x0, :] * (1 - fx) + s[..., y0, :, :][..., :, x1, :] * fx
    bot = s[..., y1, :, :][..., :, x0, :] * (1 - fx) + s[..., y1, :, :][..., :, x1, :] * fx
    return top * (1 - fy) + bot * fy


def round_u8(v: np.ndarray) -> np.ndarray:
    return np.floor(v + 0.5).astype(np.uint8)


@pytest.mark.parametrize("shape", [((36, 64), (33, 59)), ((24, 32), (35, 47)), ((64, 36), (59, 33)), ((35, 61), (20, 35)), ((17, 19), (17, 19)), ((9, 7), (40, 50))])
def test_restatement_equals_interpolate_in_float64(shape):
    (sh, sw), (rh, rw) = shape
    rng = np.random.default_rng(sh * 1000 + rw)
    src = rng.integers(0, 256, (2, sh, sw, 3), dtype=np.uint8)
    want = torch.nn.functional.interpolate(torch.from_numpy(src).permute(0, 3, 1, 2).double(), size=(rh, rw), mode="bilinear", align_corners=False)
    got = resample_f64(src, rh, rw)
    assert np.abs(got - want.permute(0, 2, 3, 1).numpy()).max() < 1e-9
    win = (1, 2, max(rh - 3, 1), max(rw - 5, 1))
    got_w = resample_f64(src, rh, rw, win, flip=True)
    want_f = torch.nn.functional.interpolate(torch.from_numpy(src[:, :, ::-1].copy()).permute(0, 3, 1, 2).double(), size=(rh, rw), mode="bilinear",
                                             align_corners=False).permute(0, 2, 3, 1).numpy()
    assert np.abs(got_w - want_f[:, win[0] : win[0] + win[2], win[1] : win[1] + win[3]]).max() < 1e-9
    if (sh, sw) == (rh, rw):
        assert np.array_equal(round_u8(got), src) and np.array_equal(got, src.astype(np.float64))  # identity size: exact copy


# ---- plan against the reference's recorded results ---------------------------------------------------------------------
def _cases():
    z = np.load(GOLDEN)
    return z, len(z["seed"])


def _targets(in_boxes, h, w):
    return [{"boxes": torch.from_numpy(b[None].copy()) if not np.isnan(b[0]) else torch.zeros(0, 4), "orig_size": torch.as_tensor([h, w])} for b in in_boxes]


def test_fixture_covers_the_branches():
    z, n = _cases()
    assert n >= 40
    tags = set(str(t) for t in z["tag"])
    assert {"sweep", "flip+branch1", "flip+branch2", "noflip+branch1", "noflip+branch2", "dropped-some", "dropped-all", "cautious-first-try", "cautious-fallback",
            "whole-image-crop"} <= tags
    assert set(str(s) for s in z["image_set"]) == {"train", "val", "test"} and set(int(r) for r in z["resolution"]) == {224, 352}
    assert set(bool(c) for c in z["cautious"]) == {True, False}
    assert (z["w"] > z["h"]).any() and (z["w"] < z["h"]).any()


@pytest.mark.parametrize("i", range(43))
def test_plan_reproduces_the_reference(i):
    from tubedetr_amd.augment import make_video_transforms

    z, n = _cases()
    assert n == 43, "the parametrisation above names every recorded case"
    seed, w, h = int(z["seed"][i]), int(z["w"][i]), int(z["h"][i])
    random.seed(seed)
    torch.manual_seed(seed)
    tr = make_video_transforms(str(z["image_set"][i]), bool(z["cautious"][i]), int(z["resolution"][i]))
    p = tr.plan(w, h, _targets(z["in_boxes"][i], h, w), str(z["in_caption"][i]))
    assert tuple(p.hw) == tuple(int(v) for v in z["out_hw"][i])
    assert p.caption == str(z["out_caption"][i])
    assert p.flip == bool(z["n_flip"][i]) and p.crop_tries == int(z["n_crop"][i]) and len(p.stages) == int(z["n_resize"][i])
    for t, want in enumerate(z["out_boxes"][i]):
        got = p.targets[t]["boxes"]
        assert len(got) == (0 if np.isnan(want[0]) else 1)
        if len(got):
            assert np.abs(got[0].numpy().astype(np.float64) - want.astype(np.float64)).max() <= 1e-6
        assert p.targets[t]["size"].tolist() == [int(v) for v in z["out_size"][i][t]] and p.targets[t]["orig_size"].tolist() == [h, w]
    # the stages chain: the last one produces the final size, and the first one reads the decoded frames
    assert (p.stages[-1].wh, p.stages[-1].ww) == tuple(p.hw) and tuple(p.src_hw) == (h, w)
    for s in p.stages:
        assert 0 <= s.wy and 0 <= s.wx and s.wy + s.wh <= s.rh and s.wx + s.ww <= s.rw


def test_a_later_draw_cannot_undo_a_dropped_box(monkeypatch):
    """Cautious crop, patched draws: try 1 takes the right half (drops the box at the left), every later try would keep
    everything.  Like the reference, ``plan`` then uses up its 100 tries and falls back to the uncropped clip, boxes intact."""
    from tubedetr_amd import augment

    tr = augment.make_video_transforms("train", True, 352)
    draws = {"randint": 0, "torch": 0}
    monkeypatch.setattr(augment.random, "random", lambda: 0.9)          # second arm of the select
    monkeypatch.setattr(augment.random, "choice", lambda seq: seq[-1])  # 300, then 352

    def randint(a, b):
        draws["randint"] += 1
        return a if draws["randint"] <= 2 else b  # try 1: the smallest crop (192 x 192); later: the whole image

    def trandint(lo, hi, size):
        draws["torch"] += 1
        return torch.tensor([hi - 1])  # bottom-right corner

    monkeypatch.setattr(augment.random, "randint", randint)
    monkeypatch.setattr(augment.torch, "randint", trandint)
    tg = [{"boxes": torch.tensor([[10.0, 10.0, 60.0, 80.0]])}, {"boxes": torch.zeros(0, 4)}]
    p = tr.plan(640, 360, tg, "to the left")
    assert p.crop_tries == 100 and draws["randint"] == 200 and draws["torch"] == 2  # whole-image tries draw no offsets
    assert [len(t["boxes"]) for t in p.targets] == [1, 0] and p.caption == "to the left" and not p.flip
    s0, s1 = p.stages
    assert (s0.rh, s0.rw, s0.wy, s0.wx, s0.wh, s0.ww) == (300, 533, 0, 0, 300, 533)  # uncropped
    assert (s1.rh, s1.rw) == tuple(p.hw) == (330, 586)
    want = torch.tensor([[35.0 / 640, 45.0 / 360, 50.0 / 640, 70.0 / 360]])
    assert (p.targets[0]["boxes"] - want).abs().max().item() < 1e-6


def test_whole_image_crop_draws_no_offsets(monkeypatch):
    from tubedetr_amd import augment

    tr = augment.make_video_transforms("train", False, 352)
    seq = iter([0.9, 0.9])  # no flip, second arm
    monkeypatch.setattr(augment.random, "random", lambda: next(seq))
    monkeypatch.setattr(augment.random, "choice", lambda s: s[0])  # 200, then 224
    monkeypatch.setattr(augment.random, "randint", lambda a, b: b)
    monkeypatch.setattr(augment.torch, "randint", lambda *a, **k: pytest.fail("a whole-image crop draws no offsets"))
    p = tr.plan(640, 360, [{"boxes": torch.tensor([[10.0, 10.0, 60.0, 80.0]])}], "x")
    assert p.crop_tries == 1 and (p.stages[0].wy, p.stages[0].wx, p.stages[0].wh, p.stages[0].ww) == (0, 0, 200, 355)


def test_table_and_errors_of_make_video_transforms():
    from tubedetr_amd.augment import get_size_with_aspect_ratio, make_video_transforms

    for res in (128, 224, 256, 288, 320, 352, 384, 416, 448, 480, 800):
        tr = make_video_transforms("val", False, res)
        assert tr.test_size == [res] and tr.scales[-1] == res
    with pytest.raises(NotImplementedError):
        make_video_transforms("train", False, 300)
    with pytest.raises(ValueError):
        make_video_transforms("trainval", False, 224)
    assert get_size_with_aspect_ratio((640, 360), 352, 587) == (330, 586)
    assert get_size_with_aspect_ratio((1280, 720), 352, 587) == (330, 586)
    assert get_size_with_aspect_ratio((360, 640), 352, 587) == (586, 330)
    assert get_size_with_aspect_ratio((320, 240), 352, 587) == (352, 469)


# ---- C ABI ------------------------------------------------------------------------------------------------------------
def test_resample_job_mirror_has_the_header_fields():
    from tubedetr_amd import _hip

    src = open(os.path.join(ROOT, "include", "tubedetr_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    body = re.search(r"typedef struct td_resample_job \{(.*?)\} td_resample_job;", " ".join(src.split())).group(1)
    names = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            names += [re.sub(r"[^A-Za-z0-9_]", "", part.split()[-1]) for part in decl.split(",")]
    assert names == [f[0] for f in _hip.ResampleJob._fields_]
    assert _hip.lib().td_abi_version() == 11 == _hip.EXPECTED_ABI


def test_clip_resample_rejects_bad_jobs_without_a_launch():
    from tubedetr_amd import _hip
    from tubedetr_amd.augment import ResampleStage, resample_job

    L = _hip.lib()
    nb = L.td_clip_resample_table_bytes(1)
    assert nb > 0 and L.td_clip_resample_table_bytes(0) == 0
    host = (ctypes.c_char * nb)()
    tab = ctypes.addressof(host)

    def call(job):
        arr = (_hip.ResampleJob * 1)(job)
        return L.td_clip_resample(arr, 1, tab, tab, nb, None)

    ok_stage = ResampleStage(33, 58, 0, 0, 33, 58)
    assert call(resample_job(16, 2, 36, 64, False, ResampleStage(33, 58, 30, 0, 4, 58), 16)) != 0 and b"window" in L.td_last_error()
    assert call(resample_job(16, 2, 36, 64, False, ResampleStage(33, 58, 0, 50, 33, 9), 16)) != 0 and b"window" in L.td_last_error()
    assert call(resample_job(None, 2, 36, 64, False, ok_stage, 16)) != 0 and b"null source" in L.td_last_error()
    assert call(resample_job(16, -1, 36, 64, False, ok_stage, 16)) != 0 and b"negative frame count" in L.td_last_error()
    assert call(resample_job(16, 2, 36, 64, False, ok_stage, 16, planar=True, H=33, W=58, mask=None)) != 0 and b"mask" in L.td_last_error()
    assert call(resample_job(16, 2, 36, 64, False, ok_stage, 16, planar=True, H=32, W=58, mask=16)) != 0 and b"planar" in L.td_last_error()
    assert call(resample_job(16, 2, 36, 64, False, ok_stage, 16, src_pitch=100)) != 0 and b"pitch" in L.td_last_error()
    assert L.td_clip_resample(None, 1, tab, tab, nb, None) != 0
    arr = (_hip.ResampleJob * 1)(resample_job(16, 2, 36, 64, False, ok_stage, 16))
    assert L.td_clip_resample(arr, 1, tab, tab, nb - 1, None) != 0 and b"table" in L.td_last_error()
