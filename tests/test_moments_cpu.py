"""Scored K-best moments, the part that needs no GPU: the float64 restatement of td_sted_topk's rule (tests/moments_ref.py)
against the reference-generated golden vectors, the well-posedness of every input that tests/test_moments_gpu.py compares
with float64, and the host-side validation of ``moments_topk``."""
import json
import os

import numpy as np
import pytest
import torch

from moments_cases import CASES, WELL_POSED, limits_case, reference
from moments_ref import moments_ref, suppressed

GOLD = np.load(os.path.join(os.path.dirname(__file__), "golden", "eval_path.npz"))


@pytest.mark.parametrize("name", ["single", "windows"])
def test_reference_with_k1_reproduces_the_golden_post_processor(name):
    from tubedetr_amd.models.postprocessors import window_table

    steds, tm = torch.from_numpy(GOLD[f"sted.{name}.steds"]), torch.from_numpy(GOLD[f"sted.{name}.time_mask"])
    vids, fids = [str(v) for v in GOLD[f"sted.{name}.video_ids"]], json.loads(str(GOLD[f"sted.{name}.frames_id"]))
    if len(set(vids)) == len(vids):
        pairs, _, count, _ = moments_ref(steds, None, None, 1, (1, 2))  # the reference masks only when it ensembles windows
    else:
        pairs, _, count, _ = moments_ref(steds, tm, window_table(vids)[0], 1, (1, 2))
    assert (count == 1).all()
    width = max(len(r) for r in fids) if len(set(vids)) != len(vids) else steds.shape[1]
    fids = [r + [0] * (width - len(r)) for r in fids]  # the frame-id table of PostProcessSTVG: short rows are padded with 0
    got = [[fids[v][int(pairs[v, 0, 0])], fids[v][int(pairs[v, 0, 1])] + 1] for v in range(len(fids))]
    assert np.array_equal(np.array(got, dtype=np.float64), GOLD[f"sted.{name}.result"])


@pytest.mark.parametrize("name", WELL_POSED)
def test_gpu_cases_are_well_posed(name):
    """A condition on the inputs, not a tolerance: at every pick the float64 winner beats the best other admissible pair by more
    than 1e-4 (twice the atol of the score comparison), so an fp32 rounding cannot decide a case."""
    pairs, scores, count, margin = reference(name)
    assert margin > 1e-4, margin
    K = CASES[name][3]
    for v in range(pairs.shape[0]):
        c = int(count[v])
        assert (pairs[v, :c, 0] < pairs[v, :c, 1]).all() and (pairs[v, c:] == -1).all() and (scores[v, c:] == float("-inf")).all()
        assert c <= K and torch.isfinite(scores[v, :c]).all() and (scores[v, :c].diff() <= 0).all()


def test_the_cases_show_what_they_are_meant_to_show():
    p = {n: reference(n)[0] for n in CASES}
    c = {n: reference(n)[2].tolist() for n in CASES}
    assert p["plain"][0, :3].tolist() == [[22, 27], [16, 27], [23, 27]] and c["plain"] == [6, 6, 6]
    assert p["nms"][0].tolist() == [[22, 27], [16, 27], [22, 24], [26, 27], [16, 20]]
    assert not torch.equal(p["nms"], p["plain"][:, :5])  # otherwise the NMS case would test nothing
    assert reference("plain")[3] > 8e-2 and reference("nms")[3] > 1.2e-1 and reference("windows")[3] > 0.2
    # windows: a start in window 1 and an end in window 2; video 1 has three valid positions; nothing lands on padding
    assert p["windows"][0, 1].tolist() == [10, 16] and c["windows"][1] == 2
    steds, valid, ptr, _, _ = CASES["windows"]
    for v in range(3):
        flat = valid[ptr[v]:ptr[v + 1]].reshape(-1)
        assert all(flat[i] for i in p["windows"][v, :c["windows"][v]].reshape(-1).tolist())
    assert p["three_plain"][0, :3].tolist() == [[0, 1], [0, 2], [1, 2]] and c["three_plain"] == [3]
    assert c["three_nms0"] == [1] and c["single_position"] == [0, 0]
    # threshold: (6, 9) overlaps (4, 7) with inter 2, union 6: kept at 1/3, dropped at 33/100
    assert p["threshold_kept"][0].tolist() == [[4, 7], [6, 9]] and p["threshold_dropped"][0].tolist() == [[4, 7], [6, 10]]
    assert not suppressed(6, 9, 4, 7, 1, 3) and suppressed(6, 9, 4, 7, 33, 100)
    assert reference("ties")[0][0].tolist() == [[4, 20], [9, 20], [4, 31], [9, 31]]
    assert reference("ties3")[0][0].tolist() == [[4, 80], [9, 80], [70, 80], [4, 90], [9, 90], [70, 90]]
    # K = 1 is td_sted_decode: never inside a -inf tail
    assert p["k1_tails"][2, 0].tolist() == [0, 1] and p["k1_tails"][1, 0, 1] < 100


def test_limits_case_picks_are_known_and_well_posed():
    """P = 3840 has 7.4 million pairs: the two picks are derived, then confirmed with a vectorised float64 pass instead of the
    brute force."""
    steds, _, ptr, K, (num, den) = limits_case()
    z = steds.double().view(-1, 2)
    assert z.shape[0] == 3840 and K == 2 and z[:, 0].argmax() == 100 and z[:, 1].argmax() == 3000
    score = z[:, 0].log_softmax(0)[:, None] + z[:, 1].log_softmax(0)[None, :]
    s, e = torch.arange(3840)[:, None], torch.arange(3840)[None, :]
    score = score.masked_fill(s >= e, float("-inf"))
    top = score.view(-1).topk(2)
    assert divmod(int(top.indices[0]), 3840) == (100, 3000) and top.values[0] - top.values[1] > 1e-4
    inter = (torch.minimum(e, torch.tensor(3000)) - torch.maximum(s, torch.tensor(100)) + 1).clamp(min=0)
    union = (e - s + 1) + (3000 - 100 + 1) - inter
    score = score.masked_fill(inter * den > num * union, float("-inf"))
    assert score[100, 3700] == float("-inf") and score[100, 3000] == float("-inf")
    top = score.view(-1).topk(2)
    assert divmod(int(top.indices[0]), 3840) == (3200, 3700) and top.values[0] - top.values[1] > 1e-4


def test_window_table():
    from tubedetr_amd.models.postprocessors import window_table

    assert window_table(["a", "a", "a", "b", "c", "c"]) == ([0, 3, 4, 6], 3)
    assert window_table([7]) == ([0, 1], 1) and window_table(["x", "y"]) == ([0, 1, 2], 1)
    with pytest.raises(ValueError, match="video_ids"):
        window_table(["a", "b", "a"])


@pytest.mark.parametrize("kwargs, name", [
    ({"k": 0}, "k"), ({"k": 33}, "k"), ({"nms": (2, 1)}, "nms"), ({"nms": (1, 0)}, "nms"),
    ({"video_ids": ["a", "b", "a"]}, "video_ids"), ({"video_ids": ["a", "b"]}, "video_ids"),
    ({"time_mask": torch.ones(3, 5, dtype=torch.bool)}, "time_mask"), ({}, "steds")])
def test_moments_topk_validates_on_the_host(kwargs, name):
    """Every argument error is a ValueError that names the argument and is raised before a device is touched: the inputs
    are CPU tensors, which are themselves refused (last case)."""
    from tubedetr_amd.models.postprocessors import PostProcessMoments, moments_topk

    with pytest.raises(ValueError, match=name):
        moments_topk(torch.zeros(3, 4, 2), **kwargs)
    if name in ("k", "nms"):
        with pytest.raises(ValueError, match=name):
            PostProcessMoments(**kwargs)


def test_symbol_is_bound_within_abi_11():
    from tubedetr_amd import _hip

    assert "td_sted_topk" in _hip.EXPORTS and len(_hip._SIGS["td_sted_topk"]) == 14 and _hip.EXPECTED_ABI == 11


def test_library_refuses_bad_arguments_before_any_launch():
    """td_sted_topk's host checks, through the C ABI with non-null dummy pointers: nothing is launched (there is no GPU here)."""
    import ctypes

    from tubedetr_amd import _hip
    from tubedetr_amd.build import build_lib

    build_lib(verbose=False)
    L = _hip.lib()
    p = ctypes.c_void_p(16)

    def call(steds=p, n_videos=1, n_windows=1, T=4, max_windows=1, K=1, num=1, den=2, pairs=p, scores=p, count=p):
        rc = L.td_sted_topk(steds, None, None, n_videos, n_windows, T, max_windows, K, num, den, pairs, scores, count, None)
        return rc, L.td_last_error()

    for kw, word in [({"steds": None}, b"null"), ({"pairs": None}, b"null"), ({"scores": None}, b"null"), ({"count": None}, b"null"),
                     ({"n_videos": 0}, b"n_videos"), ({"T": 0}, b"T="), ({"K": 0}, b"K=0"), ({"K": 33}, b"K=33"), ({"den": 0}, b"nms"),
                     ({"num": -1}, b"nms"), ({"num": 3}, b"nms"), ({"n_videos": 2}, b"n_windows"),
                     ({"T": 3841}, b"3840"), ({"T": 1921, "max_windows": 2}, b"3840"), ({"T": 2 ** 30, "max_windows": 8}, b"3840")]:
        rc, msg = call(**kw)
        assert rc != 0 and word in msg, (kw, rc, msg)
