"""td_sted_topk, ``moments_topk`` and ``PostProcessMoments`` on the GPU, against tests/moments_ref.py (the float64 brute-force
restatement of the rule in include/tubedetr_hip.h).  Pairs and counts are compared for equality; scores at atol = 5e-5, half
the margin by which tests/test_moments_cpu.py shows every compared case to be well posed (the fp32 error of a log-softmax
over <= 3840 entries of magnitude <= ~30 is a few 1e-6)."""
import pytest
import torch

from moments_cases import CASES, TIES, TIES3, limits_case, reference

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
ATOL = 5e-5


def run(case):
    from tubedetr_amd.models.postprocessors import moments_topk

    steds, valid, ptr, K, nms = case
    ids = None if ptr is None else [v for v in range(len(ptr) - 1) for _ in range(ptr[v + 1] - ptr[v])]
    m = moments_topk(steds.to(DEV), None if valid is None else valid.to(DEV), ids, K, nms)
    assert m.pairs.dtype == torch.int64 and m.scores.dtype == torch.float32 and m.count.dtype == torch.int32
    return m.pairs.cpu(), m.scores.cpu(), m.count.cpu()


def check(name):
    """Run the case and compare all three outputs with the shared reference; -> the device's (pairs, scores, count)."""
    want_p, want_s, want_c, margin = reference(name)
    assert margin > 1e-4
    pairs, scores, count = run(CASES[name])
    assert torch.equal(count.long(), want_c), (count.tolist(), want_c.tolist())
    assert torch.equal(pairs, want_p), (pairs.tolist(), want_p.tolist())
    made = want_s > float("-inf")
    assert (scores[~made] == float("-inf")).all() and (pairs[~made] == -1).all()  # the fill beyond the count
    err = (scores.double()[made] - want_s[made]).abs().max().item() if made.any() else 0.0
    print(f"{name}: largest score error {err:.3e}, smallest margin {margin:.3e}")
    assert err <= ATOL, err
    return pairs, scores, count


@pytest.mark.parametrize("name", ["k1_random", "k1_tails"])
def test_k1_is_sted_decode(name):
    from tubedetr_amd.models.postprocessors import sted_decode

    pairs, _, count = check(name)
    assert torch.equal(pairs[:, 0], sted_decode(CASES[name][0].to(DEV)).cpu()) and (count == 1).all()
    if name == "k1_tails":
        assert pairs[2, 0].tolist() == [0, 1] and pairs[1, 0, 1] < 100  # never inside the -inf tail


def test_plain_top_k_and_nms():
    plain, _, _ = check("plain")
    assert plain[0, :3].tolist() == [[22, 27], [16, 27], [23, 27]]
    nms, _, _ = check("nms")
    assert nms[0].tolist() == [[22, 27], [16, 27], [22, 24], [26, 27], [16, 20]]
    assert not torch.equal(nms, plain[:, :5])


def test_windows_are_concatenated_and_padding_is_never_picked():
    pairs, _, count = check("windows")
    assert pairs[0, 1].tolist() == [10, 16] and count.tolist()[1] == 2  # a start in window 1, an end in window 2; three valid positions
    _, valid, ptr, _, _ = CASES["windows"]
    for v in range(3):
        flat = valid[ptr[v]:ptr[v + 1]].reshape(-1)
        assert all(flat[i] for i in pairs[v, :int(count[v])].reshape(-1).tolist())


def test_exhaustion_and_fill():
    pairs, scores, count = check("three_plain")
    assert count.tolist() == [3] and pairs[0].tolist() == [[0, 1], [0, 2], [1, 2], [-1, -1], [-1, -1]]
    assert (scores[0, 3:] == float("-inf")).all() and torch.isfinite(scores[0, :3]).all()
    pairs, scores, count = check("three_nms0")
    assert count.tolist() == [1] and pairs[0].tolist() == [[0, 1]] + [[-1, -1]] * 4 and (scores[0, 1:] == float("-inf")).all()
    pairs, scores, count = check("single_position")  # T = 1
    assert count.tolist() == [0, 0] and (pairs == -1).all() and (scores == float("-inf")).all()


def test_exact_ties_go_to_the_smallest_end_then_start():
    pairs, scores, count = run(TIES)
    assert count.tolist() == [4] and pairs[0].tolist() == [[4, 20], [9, 20], [4, 31], [9, 31]]
    assert (scores[0] == scores[0, 0]).all()  # bit-equal log-probabilities
    assert torch.equal(pairs, reference("ties")[0])
    pairs, scores, count = run(TIES3)  # three equal starts: a tie inside the recomputation of an end
    assert count.tolist() == [6] and pairs[0].tolist() == [[4, 80], [9, 80], [70, 80], [4, 90], [9, 90], [70, 90]]
    assert (scores[0] == scores[0, 0]).all() and torch.equal(pairs, reference("ties3")[0])


def test_threshold_equality_is_kept():
    kept, _, _ = check("threshold_kept")
    assert kept[0].tolist() == [[4, 7], [6, 9]]  # inter 2, union 6 at nms 1/3
    dropped, _, _ = check("threshold_dropped")
    assert dropped[0].tolist() == [[4, 7], [6, 10]]  # 1/3 > 33/100


def test_limits():
    from tubedetr_amd.models.postprocessors import moments_topk

    pairs, scores, count = run(limits_case())  # P = 3840 as 16 windows of 240
    assert count.tolist() == [2] and pairs[0].tolist() == [[100, 3000], [3200, 3700]]
    assert scores[0, 0] > scores[0, 1] and torch.isfinite(scores).all()
    with pytest.raises(RuntimeError, match="3840"):  # refused on the host, nothing is launched
        moments_topk(torch.zeros(1, 3841, 2, device=DEV))
    with pytest.raises(RuntimeError, match="3840"):
        moments_topk(torch.zeros(17, 226, 2, device=DEV), video_ids=[0] * 17, k=2)  # 17 * 226 = 3842


def test_memory_discipline():
    """Outputs carved out of canary-filled buffers: nothing before or behind them is written; ``moments_topk`` on a non-default
    stream with bf16 logits neither synchronises nor differs from the fp32 call on the rounded logits."""
    from tubedetr_amd import _hip
    from tubedetr_amd.models.postprocessors import moments_topk

    steds, valid, ptr, K, nms = CASES["windows"]
    want_p, want_s, want_c, _ = reference("windows")
    n = len(ptr) - 1
    z, va, table = steds.to(DEV), valid.to(DEV), torch.tensor(ptr, dtype=torch.int32, device=DEV)
    pad = 16
    big_p = torch.full((pad + n * K * 2 + pad,), 0x5A5A5A5A5A5A5A5A, dtype=torch.int64, device=DEV)
    big_s = torch.full((pad + n * K + pad,), 12345.0, dtype=torch.float32, device=DEV)
    big_c = torch.full((pad + n + pad,), 0x5A5A5A5A, dtype=torch.int32, device=DEV)
    out_p, out_s, out_c = big_p[pad:pad + n * K * 2], big_s[pad:pad + n * K], big_c[pad:pad + n]
    _hip.check(_hip.lib().td_sted_topk(_hip.ptr(z), _hip.ptr(va), _hip.ptr(table), n, steds.shape[0], steds.shape[1], 3, K, nms[0], nms[1],
                                       out_p.data_ptr(), out_s.data_ptr(), out_c.data_ptr(), _hip.stream_ptr()), "td_sted_topk")
    torch.cuda.synchronize()
    assert torch.equal(out_p.cpu().view(n, K, 2), want_p) and torch.equal(out_c.cpu().long(), want_c)
    for big, canary in ((big_p, 0x5A5A5A5A5A5A5A5A), (big_s, 12345.0), (big_c, 0x5A5A5A5A)):
        assert (big[:pad] == canary).all() and (big[-pad:] == canary).all()

    z16 = steds.to(DEV, torch.bfloat16)
    ids = ["a", "a", "a", "b", "c", "c"]
    same = moments_topk(z16.float(), va, ids, K, nms)
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    torch.cuda.synchronize()
    mode = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")  # moments_topk must not synchronise
    try:
        with torch.cuda.stream(stream):
            got = moments_topk(z16, va, ids, K, nms)
            again = moments_topk(z16, va, ids, K, nms)  # a second table while the first may still be in flight
    finally:
        torch.cuda.set_sync_debug_mode(mode)
    torch.cuda.synchronize()
    for m in (got, again):
        assert torch.equal(m.pairs, same.pairs) and torch.equal(m.scores, same.scores) and torch.equal(m.count, same.count)


def test_end_to_end_model_to_moments():
    """T = 6, res 64, k = 2 on the synthetic model (as tests/test_overlay_gpu.py builds it): the best moment is PostProcessSTVG's
    span, the scores are log-probabilities in non-increasing order, and the spans feed ``annotate`` unchanged."""
    import tubedetr_amd
    from oracle.tubedetr_oracle import OracleConfig
    from oracle.weights import fill_state, state_spec, synthetic_batch
    from tubedetr_amd.harness import FixedTokenizer, batch_to
    from tubedetr_amd.models import build_model
    from tubedetr_amd.models.postprocessors import PostProcessMoments, PostProcessSTVG
    from tubedetr_amd.util.misc import NestedTensor

    dev = torch.device(DEV)
    T, res, k, L = 6, 64, 2, 5
    batch = synthetic_batch(T=T, res=res, k=k, L=L, seed=3)
    model, _, _ = build_model(tubedetr_amd.default_args(stride=k, compute_dtype=torch.float32))
    model.load_state_dict(fill_state(state_spec(OracleConfig(stride=k)), 11), strict=True)
    model.to(dev).eval()
    model.transformer.tokenizer = FixedTokenizer(batch["input_ids"], batch["attention_mask"])
    bt = batch_to(batch, dev)
    with torch.no_grad():
        samples, fast = NestedTensor(bt["frames"], bt["frames_mask"]), NestedTensor(bt["frames_fast"], bt["fast_mask"])
        cache = model(samples, [T], ["synthetic caption"], encode_and_save=True, samples_fast=fast)
        out = model(samples, [T], ["synthetic caption"], encode_and_save=False, memory_cache=cache)
    assert out["pred_sted"].shape == (1, T, 2)
    frames_id, ids, tm = [[10, 12, 14, 16, 18, 20]], ["v0"], torch.ones(1, T, dtype=torch.bool, device=dev)
    want = PostProcessSTVG()(out, frames_id=frames_id, video_ids=ids, time_mask=tm)
    post = PostProcessMoments(k=3)
    got = post(out, frames_id, ids, tm)
    assert len(got) == 1 and 1 <= len(got[0]) <= 3
    assert got[0][0]["span"] == [int(x) for x in want[0]]
    s = [m["score"] for m in got[0]]
    assert all(x <= 0.0 for x in s) and s == sorted(s, reverse=True)
    d = post.forward_device(out, frames_id, ids, tm)
    c = int(d.count[0])
    assert d.pairs[0, :c].cpu().tolist() == [m["span"] for m in got[0]] and (d.pairs[0, c:] == -1).all()
