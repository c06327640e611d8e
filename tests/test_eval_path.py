"""Evaluation-side path against golden vectors produced by the reference itself
(tests/golden/eval_path.npz, oracle/gen_golden_eval.py): PostProcessSTVG incl. multi-window ensembling, PostProcess, the
windowed collation bookkeeping, the learning-rate schedules.  CPU tests pin the oracle restatement and the host logic;
the GPU tests run the HIP post-processor."""
import json
import os
import types

import numpy as np
import pytest
import torch

GOLD = np.load(os.path.join(os.path.dirname(__file__), "golden", "eval_path.npz"))


def _sted_case(name):
    return (torch.from_numpy(GOLD[f"sted.{name}.steds"]), torch.from_numpy(GOLD[f"sted.{name}.time_mask"]), [str(v) for v in GOLD[f"sted.{name}.video_ids"]],
            json.loads(str(GOLD[f"sted.{name}.frames_id"])), GOLD[f"sted.{name}.result"])


@pytest.mark.parametrize("name", ["single", "windows"])
def test_oracle_post_process_matches_reference(name):
    from oracle.eval_oracle import post_process_stvg

    steds, tm, vids, fids, want = _sted_case(name)
    assert np.array_equal(np.array(post_process_stvg(steds, fids, vids, tm)), want)


def test_box_post_process_matches_reference():
    from tubedetr_amd.models.postprocessors import PostProcess, build_postprocessors

    res = PostProcess()({"pred_boxes": torch.from_numpy(GOLD["bbox.boxes"])}, torch.from_numpy(GOLD["bbox.sizes"]))
    assert np.allclose(torch.stack([r["boxes"] for r in res]).numpy(), GOLD["bbox.result"], rtol=0, atol=1e-5)
    assert set(build_postprocessors(None, "vidstg")) == {"bbox", "vidstg"} and set(build_postprocessors(None, "x")) == {"bbox"}


def test_window_split_matches_reference_collate():
    from tubedetr_amd.util.misc import split_into_windows

    if "windows.error" in GOLD:
        pytest.skip(str(GOLD["windows.error"]))
    durations = [int(x) for x in GOLD["windows.durations_in"]]
    batch = {"durations": durations, "captions": [f"c{i}" for i in range(len(durations))], "video_ids": [f"v{i}" for i in range(len(durations))],
             "inter_idx": [list(map(int, r)) for r in GOLD["windows.inter_in"]]}
    out = split_into_windows(batch, int(GOLD["windows.div"]))
    assert out["durations"] == [int(x) for x in GOLD["windows.durations"]]
    assert out["inter_idx"] == [list(map(int, r)) for r in GOLD["windows.inter_idx"]]
    assert out["video_ids"] == [str(x) for x in GOLD["windows.video_ids"]] and out["captions"] == [str(x) for x in GOLD["windows.captions"]]
    assert split_into_windows(batch, 0) is batch


def test_learning_rate_schedules_match_reference():
    from tubedetr_amd.optim import adjust_learning_rate

    names = ["step", "multistep", "linear_with_warmup", "all_linear_with_warmup"]
    for row in GOLD["lr.rows"]:
        a = types.SimpleNamespace(fraction_warmup_steps=0.01, schedule=names[int(row[0])], lr_drop=10, epochs=120, lr=5e-5, lr_backbone=1e-5, text_encoder_lr=5e-5)
        opt = types.SimpleNamespace(param_groups=[{"lr": 0.0}, {"lr": 0.0}, {"lr": 0.0}])
        adjust_learning_rate(opt, int(row[1]), int(row[2]), num_training_steps=100000, args=a)
        assert np.allclose([g["lr"] for g in opt.param_groups], row[3:], rtol=1e-12, atol=0), row


# ---- td_sted_decode called directly, against a float64 restatement of oracle/eval_oracle.py:27-33 ----
def _decode_ref(steds):
    """(start, end) per video and, per video, by how much the best pair's score beats the runner-up pair's (float64)."""
    z = steds.double()
    n, T, _ = z.shape
    mask = (torch.ones(T, T, dtype=torch.float64) * float("-inf")).tril(0)  # end <= start impossible
    score = z[:, :, 0].log_softmax(1).unsqueeze(2) + z[:, :, 1].log_softmax(1).unsqueeze(1) + mask
    best, s_idx = score.max(dim=1)
    _, e_idx = best.max(dim=1)
    s_idx = torch.gather(s_idx, 1, e_idx.view(-1, 1)).squeeze(1)
    top = score.reshape(n, -1).topk(min(2, T * T), dim=1).values
    margin = top[:, 0] - top[:, 1] if T > 1 else torch.full((n,), float("inf"), dtype=torch.float64)
    return torch.stack([s_idx, e_idx], 1), margin


def _sted_ordering_case():
    steds = torch.randn(1, 300, 2, generator=torch.Generator().manual_seed(3))
    steds[0, 250, 0] = steds[0, :, 0].max() + 6.0  # the likeliest start lies after the likeliest end
    steds[0, 20, 1] = steds[0, :, 1].max() + 6.0
    return steds


def _sted_tails_case():
    steds = torch.randn(3, 257, 2, generator=torch.Generator().manual_seed(4)) * 4
    steds[1, 100:] = float("-inf")
    steds[2, 2:] = float("-inf")
    return steds


def _sted_random_case():
    return torch.randn(4, 257, 2, generator=torch.Generator().manual_seed(6)) * 4


WELL_POSED = {"ordering": _sted_ordering_case, "tails": _sted_tails_case, "random": _sted_random_case}


@pytest.mark.parametrize("name", sorted(WELL_POSED))
def test_sted_decode_inputs_are_well_posed(name):
    """A condition on the inputs, not a tolerance: the float64 winner beats the runner-up pair by more than 1e-4, so one ulp
    of expf / logf cannot decide a case of test_hip_sted_decode_matches_float64_reference."""
    steds = WELL_POSED[name]()
    want, margin = _decode_ref(steds)
    assert (margin > 1e-4).all(), margin.tolist()
    assert (want[:, 0] < want[:, 1]).all()
    if name == "ordering":
        assert steds[0, :, 0].argmax() == 250 and steds[0, :, 1].argmax() == 20


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(WELL_POSED))
def test_hip_sted_decode_matches_float64_reference(name):
    from tubedetr_amd.models.postprocessors import sted_decode

    steds = WELL_POSED[name]()
    want, margin = _decode_ref(steds)
    assert (margin > 1e-4).all(), margin.tolist()
    got = sted_decode(steds.to("cuda:0")).cpu()
    assert got.dtype == torch.int64 and torch.equal(got, want), (got.tolist(), want.tolist())
    assert (got[:, 0] < got[:, 1]).all()
    if name == "tails":
        assert got[2].tolist() == [0, 1] and got[1, 1] < 100  # never inside the -inf tail


@pytest.mark.gpu
def test_hip_sted_decode_shortest_videos():
    from tubedetr_amd.models.postprocessors import sted_decode

    g = torch.Generator().manual_seed(2)
    one = torch.randn(3, 1, 2, generator=g) * 4
    assert sted_decode(one.to("cuda:0")).cpu().tolist() == [[0, 0]] * 3 == _decode_ref(one)[0].tolist()
    two = torch.randn(4, 2, 2, generator=g) * 4
    two[1] = torch.tensor([[-9.0, 9.0], [9.0, -9.0]])  # (0, 1) is the only pair with end > start, however unlikely
    assert sted_decode(two.to("cuda:0")).cpu().tolist() == [[0, 1]] * 4 == _decode_ref(two)[0].tolist()


@pytest.mark.gpu
def test_hip_sted_decode_first_index_wins_exact_ties():
    from tubedetr_amd.models.postprocessors import sted_decode

    steds = torch.full((1, 40, 2), -3.0)
    steds[0, [4, 9], 0] = 5.0
    steds[0, [20, 31], 1] = 5.0  # equal logits give bit-equal log-probabilities: four pairs tie exactly
    assert _decode_ref(steds)[0].tolist() == [[4, 20]]
    assert sted_decode(steds.to("cuda:0")).cpu().tolist() == [[4, 20]]


@pytest.mark.gpu
def test_hip_sted_decode_lds_limit():
    from tubedetr_amd.models.postprocessors import sted_decode

    steds = torch.randn(1, 3840, 2, generator=torch.Generator().manual_seed(8)) * 0.25  # the longest video the kernel's LDS holds
    steds[0, 100, 0] = 8.0
    steds[0, 3000, 1] = 8.0
    # 100 < 3000 are the two arg-maxima, so the pair is the unconstrained optimum as well: no T x T reference needed
    assert steds[0, :, 0].argmax() == 100 and steds[0, :, 1].argmax() == 3000
    assert sted_decode(steds.to("cuda:0")).cpu().tolist() == [[100, 3000]]
    with pytest.raises(RuntimeError, match="3840"):  # refused on the host, nothing is launched
        sted_decode(torch.zeros(1, 3841, 2, device="cuda:0"))


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["single", "windows"])
def test_hip_post_process_matches_reference(name):
    from tubedetr_amd.models.postprocessors import PostProcessSTVG

    steds, tm, vids, fids, want = _sted_case(name)
    dev = torch.device("cuda:0")
    got = PostProcessSTVG()({"pred_sted": steds.to(dev)}, frames_id=fids, video_ids=vids, time_mask=tm.to(dev))
    assert np.array_equal(np.array(got), want)


@pytest.mark.gpu
def test_hip_post_process_matches_oracle_on_long_videos():
    from oracle.eval_oracle import post_process_stvg
    from tubedetr_amd.models.postprocessors import PostProcessSTVG

    g = torch.Generator().manual_seed(9)
    B, T = 6, 200
    steds = torch.randn(B, T, 2, generator=g) * 4
    tm = torch.ones(B, T, dtype=torch.bool)
    tm[1, 150:] = False
    tm[5, 60:] = False
    vids = ["a", "a", "b", "c", "c", "c"]
    fids = [list(range(400)), list(range(10, 210)), list(range(0, 1200, 2))]
    dev = torch.device("cuda:0")
    got = PostProcessSTVG()({"pred_sted": steds.to(dev)}, frames_id=fids, video_ids=vids, time_mask=tm.to(dev))
    assert got == post_process_stvg(steds, fids, vids, tm)
    uniq = [f"v{i}" for i in range(B)]
    f2 = [list(range(T))] * B
    assert PostProcessSTVG()({"pred_sted": steds.to(dev)}, frames_id=f2, video_ids=uniq, time_mask=tm.to(dev)) == post_process_stvg(steds, f2, uniq, tm)
