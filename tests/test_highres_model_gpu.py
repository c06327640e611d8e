"""The bf16 model at frame sizes whose per-frame token count S lies beyond the one-block lean kernels (S > 256): 544 x 544
frames (17 x 17 visual tokens + 30 text tokens = 319) and 608 x 608 (19 x 19 + 30 = 391).  The encoder's self-attention
now runs on the streaming lean kernels; the same step with TD_MHA_LEAN=0 (read per call) runs it on the probabilities
kernels instead.  Both are bf16 runs of the same model, so they must agree to bf16 rounding, forward and backward, and the
new one must stay at least as close to the exact-fp32 mode of the same step as the old one."""
import pytest
import torch

pytestmark = pytest.mark.gpu

WEIGHT_SEED, CLIP_SEED = 17, 77


def _step(model, criterion, weight_dict, b_dev, params):
    from tubedetr_amd.harness import forward_step

    for p in params:
        p.grad = None
    loss, _, out, _ = forward_step(model, criterion, weight_dict, b_dev)
    loss.backward()
    torch.cuda.synchronize()
    grads = [None if p.grad is None else p.grad.detach().double().flatten().clone() for p in params]
    return loss.item(), out["pred_boxes"].float().clone(), out["pred_sted"].float().clone(), grads


@pytest.mark.parametrize("res,S", [(544, 319), (608, 391)])
def test_bf16_model_on_streaming_encoder_attention_follows_probs_path(res, S, monkeypatch):
    import tubedetr_amd
    from oracle.tubedetr_oracle import OracleConfig
    from oracle.weights import fill_state, state_spec, synthetic_batch
    from tubedetr_amd import ops
    from tubedetr_amd.harness import FixedTokenizer, batch_to
    from tubedetr_amd.models import build_model

    T, k, L = 8, 4, 30
    cfg = OracleConfig(stride=k)
    sd = fill_state(state_spec(cfg), WEIGHT_SEED)
    batch = synthetic_batch(T=T, res=res, k=k, L=L, seed=CLIP_SEED, pad_w=40)  # ragged frame masks: a padded strip of columns
    model, criterion, weight_dict = build_model(tubedetr_amd.default_args(stride=k, compute_dtype=torch.bfloat16))
    model.load_state_dict(sd, strict=True)
    model.to(torch.device("cuda:0")).eval()
    model.transformer.tokenizer = FixedTokenizer(batch["input_ids"], batch["attention_mask"])
    b_dev = batch_to(batch, torch.device("cuda:0"))
    params = [p for p in model.parameters() if p.requires_grad]

    seen = []
    lean_fwd = ops.mha_lean_fwd

    def counting(q, k_, *a, **kw):
        seen.append(k_.shape[1])
        return lean_fwd(q, k_, *a, **kw)

    monkeypatch.setattr(ops, "mha_lean_fwd", counting)
    new = _step(model, criterion, weight_dict, b_dev, params)
    assert S in seen, (S, sorted(set(seen)))  # the encoder took the lean path at S tokens per frame
    monkeypatch.setenv("TD_MHA_LEAN", "0")
    n_before = len(seen)
    old = _step(model, criterion, weight_dict, b_dev, params)
    assert len(seen) == n_before  # ...and the A/B run did not
    model.set_compute_dtype(torch.float32)  # the exact-fp32 mode: the yardstick of both bf16 runs
    ref = _step(model, criterion, weight_dict, b_dev, params)

    def compare(x, y):
        (l_x, b_x, s_x, g_x), (l_y, b_y, s_y, g_y) = x, y
        assert abs(l_x - l_y) < 0.02 * abs(l_y), (l_x, l_y)
        assert (b_x - b_y).abs().max().item() < 0.05
        assert (s_x - s_y).abs().max().item() < 0.1 * max(1.0, s_y.abs().max().item())
        dot = n_x = n_y = 0.0
        for a, b in zip(g_x, g_y):
            assert (a is None) == (b is None)
            if a is None:
                continue
            assert torch.isfinite(a).all()
            dot += (a @ b).item()
            n_x += (a @ a).item()
            n_y += (b @ b).item()
        return dot / (n_x * n_y) ** 0.5, (n_x / n_y) ** 0.5

    # Two slow frames per clip: bf16 rounding noise averages out over few rows, as in test_fullsize_gpu.py's cfg1 (bf16 vs fp32
    # whole-gradient cosine measured 0.981 .. 0.992, bounded at 0.97 / 13 %); the two bf16 runs measured 0.985 against each other.
    cos_ab, nr_ab = compare(new, old)
    cos_new, nr_new = compare(new, ref)
    cos_old, nr_old = compare(old, ref)
    rec = dict(new_vs_old=(cos_ab, nr_ab), new_vs_fp32=(cos_new, nr_new), old_vs_fp32=(cos_old, nr_old))
    print("gradients:", rec)
    assert cos_ab >= 0.97 and abs(nr_ab - 1.0) <= 0.13, rec
    assert cos_new >= 0.97 and abs(nr_new - 1.0) <= 0.13, rec
    assert cos_new >= cos_old - 0.01, rec  # the streaming kernels keep the step at least as close to exact as the probabilities path


def test_model_above_512_tokens_per_frame_fp32_matches_oracle_and_bf16_follows():
    """736 x 736 frames: 23 x 23 visual tokens + 24 text tokens = S = 553, beyond every resident attention kernel (T = 8, k = 4,
    fast branch on, a padded strip for ragged masks).  The fp32 encoder and the decoder's cross-attention (projected path above
    S = 320) run on the chunked probabilities kernels, the bf16 encoder on the streaming lean kernels.  fp32 mode against the CPU
    oracle's forward (logits and attention weights of all six decoder layers within 1e-3, the 24 losses); the bf16 step finite
    and following the fp32 one (whole-gradient cosine and length as for two slow frames in test_fullsize_gpu.py's cfg1)."""
    import tubedetr_amd
    from oracle import tubedetr_oracle as O
    from oracle.tubedetr_oracle import OracleConfig
    from oracle.weights import fill_state, state_spec, synthetic_batch
    from tubedetr_amd.harness import FixedTokenizer, batch_to, forward_step
    from tubedetr_amd.models import build_model

    T, k, L, res = 8, 4, 24, 736
    cfg = OracleConfig(stride=k)
    sd = fill_state(state_spec(cfg), WEIGHT_SEED)
    batch = synthetic_batch(T=T, res=res, k=k, L=L, seed=CLIP_SEED, pad_w=40)
    with torch.no_grad():
        cache = O.encode(sd, cfg, batch["frames"], batch["frames_mask"], batch["durations"], batch["input_ids"], batch["attention_mask"],
                         batch.get("frames_fast"), batch.get("fast_mask"))
        out_ref = O.decode(sd, cfg, cache)
        keep = O.keep_indices(batch["durations"], batch["inter_idx"])
        g = dict(out_ref)
        g["pred_boxes"] = out_ref["pred_boxes"][keep]
        g["aux_outputs"] = [dict(a, pred_boxes=a["pred_boxes"][keep]) for a in out_ref.get("aux_outputs", [])]
        ld_ref = O.criterion(g, batch["target_boxes"], batch["inter_idx"], torch.ones(1, T, dtype=torch.bool), cfg)
    model, criterion, weight_dict = build_model(tubedetr_amd.default_args(stride=k, compute_dtype=torch.float32))
    model.load_state_dict(sd, strict=True)
    model.to(torch.device("cuda:0")).eval()
    model.transformer.tokenizer = FixedTokenizer(batch["input_ids"], batch["attention_mask"])
    b_dev = batch_to(batch, torch.device("cuda:0"))
    with torch.no_grad():
        _, ld, out, _ = forward_step(model, criterion, weight_dict, b_dev)
    torch.cuda.synchronize()
    layers, layers_ref = out["aux_outputs"] + [out], out_ref["aux_outputs"] + [out_ref]
    assert len(layers) == len(layers_ref) == 6
    for key in ("pred_boxes", "pred_sted", "weights", "ca_weights"):
        err = max((a[key].float().cpu() - b[key]).abs().max().item() for a, b in zip(layers, layers_ref))
        assert err < 1e-3, (key, err)
    assert layers[-1]["ca_weights"].shape[-1] == 553, layers[-1]["ca_weights"].shape  # S tokens per frame
    assert sorted(ld) == sorted(ld_ref) and len(ld) == 24
    for k_ in ld_ref:
        assert abs(ld[k_].item() - ld_ref[k_].item()) < 1e-3 * max(1.0, abs(ld_ref[k_].item())), k_
    params = [p for p in model.parameters() if p.requires_grad]
    ref = _step(model, criterion, weight_dict, b_dev, params)
    model.set_compute_dtype(torch.bfloat16)
    got = _step(model, criterion, weight_dict, b_dev, params)
    assert abs(got[0] - ref[0]) < 0.02 * abs(ref[0]), (got[0], ref[0])
    dot = n_x = n_y = 0.0
    for a, b in zip(got[3], ref[3]):
        if a is None:
            continue
        assert torch.isfinite(a).all()
        dot += (a @ b).item()
        n_x += (a @ a).item()
        n_y += (b @ b).item()
    cos, nr = dot / (n_x * n_y) ** 0.5, (n_x / n_y) ** 0.5
    print("bf16 vs fp32 at S = 553:", cos, nr)
    assert cos >= 0.97 and abs(nr - 1.0) <= 0.13, (cos, nr)
