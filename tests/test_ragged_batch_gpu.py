"""Batches of videos with different slow-clip counts on a real MI355X: the device-built index vectors (td_replica_maps), forward / loss /
gradient parity, several captions on ragged clips, host-built against device-built maps, bf16, the uint8 pipeline.

Definition of correct: every video's valid entries are what the model gives for that video ALONE.  The reference is the CPU oracle's
``encode`` + ``decode`` per video (one shared state dict), stitched into the padded layout with zeros in every padded entry (a padded
frame's key mask is what it is in an equal-count batch: every visual token but token 0 masked, the text tokens under the caption's mask), then
``oracle.criterion`` on the stitched outputs after ``keep_indices`` - never the path under test.
Case: OracleConfig(stride=4), weights fill_state(state_spec(cfg), 5), eval mode;
synthetic_batch(T=9, res=64, k=4, L=7, seed=33, durations=[9, 3, 6], text_pad=3): clip counts 3, 1, 2.
Bounds: tests/test_multi_sentence_gpu.py's and tests/test_model_gpu.py's (LOGIT_TOL = 1e-3, their loss, gradient and bf16 rules)."""
import ctypes
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

LOGIT_TOL = 1e-3
K, L_TOK, RES = 4, 7, 64
DURATIONS = [9, 3, 6]
PAIR_CLIPS, PAIR_INDEX = [9, 3], [1, 0, 0, 1]
DEV = "cuda:0"


# ----------------------------------------------------------------------------------------------------------------------------------
# 1. device-built maps
# ----------------------------------------------------------------------------------------------------------------------------------
MAP_NAMES = ("vis_src", "vis_dst", "txt_src", "txt_dst", "all_src", "iota_vis", "clip_vis", "clip_txt",
             "seg_vis_idx", "seg_vis_ptr", "seg_txt_idx", "seg_txt_ptr", "seg_all_idx", "seg_all_ptr")
LAYOUT_NAMES = ("owner", "vid_of_frame", "vid_of_clip", "query_mask", "frame_dest", "clip_of")
GUARD = 8  # sentinel words on either side of every output buffer


def _closed_forms(durations, k, hw, L):
    """Every vector from plain numpy / Python loops over (video, frame, token)."""
    b, t = len(durations), max(durations)
    clips = [math.ceil(d / k) for d in durations]
    first = [sum(clips[:i]) for i in range(b)]
    n, F, S = sum(clips), b * t, hw + L
    owner = np.array([first[i] + min(j // k, clips[i] - 1) for i in range(b) for j in range(t)], dtype=np.int64)
    want = {"owner": owner,
            "vid_of_frame": np.repeat(np.arange(b), t),
            "vid_of_clip": np.repeat(np.arange(b), clips),
            "query_mask": np.array([1 if (j >= durations[i] and j > 0) else 0 for i in range(b) for j in range(t)], dtype=np.uint8),
            "frame_dest": np.array([i * t + j for i in range(b) for j in range(durations[i])], dtype=np.int64),
            "clip_of": np.array([first[i] + j // k for i in range(b) for j in range(durations[i])], dtype=np.int64)}
    f, c = np.arange(F)[:, None], np.arange(n)[:, None]
    p, l_, s = np.arange(hw)[None, :], np.arange(L)[None, :], np.arange(S)[None, :]
    want.update(vis_src=owner[:, None] * S + p, vis_dst=f * S + p, txt_src=owner[:, None] * S + hw + l_, txt_dst=f * S + hw + l_,
                all_src=owner[:, None] * S + s, iota_vis=np.arange(n * hw), clip_vis=c * S + p, clip_txt=c * S + hw + l_)
    for name, m, row0 in (("seg_vis", hw, 0), ("seg_txt", L, hw), ("seg_all", S, 0)):
        idx, ptr = [], [0]
        for ci in range(n):
            frames = np.nonzero(owner == ci)[0]
            for col in range(m):
                idx.extend((frames * S + row0 + col).tolist())
                ptr.append(len(idx))
        want[name + "_idx"], want[name + "_ptr"] = np.array(idx), np.array(ptr)
    return {k_: np.asarray(v).reshape(-1).astype(np.int64) for k_, v in want.items()}, (b, t, n, F, S, clips, first)


@pytest.mark.parametrize("durations,k,hw,L", [([9, 3, 6], 4, 4, 7), ([8, 6], 4, 4, 7), ([1], 4, 4, 7), ([5, 5], 5, 4, 7), ([7, 2, 2, 13], 3, 4, 7),
                                              ([100, 37], 4, 121, 30)], ids=["9-3-6", "8-6", "1", "5-5", "7-2-2-13", "100-37"])
def test_device_built_maps_equal_host_built_maps(durations, k, hw, L):
    """td_replica_maps into sentinel-guarded buffers, as exact integers against numpy closed forms and against the host builder
    ReplicaMaps(owner_host, n, hw, L); ReplicaMaps.from_table yields the same attributes.  [100, 37] at hw = 121, L = 30: 30 200 frame
    rows, 139 workgroups."""
    from tubedetr_amd import _hip
    from tubedetr_amd.functional import ReplicaMaps, batch_layout

    want, (b, t, n, F, S, clips, first) = _closed_forms(durations, k, hw, L)
    lay = batch_layout(durations, k)
    assert (lay.n, lay.F, lay.clips, lay.first_clip) == (n, F, clips, first)
    for name in LAYOUT_NAMES:
        host = lay.query_mask if name == "query_mask" else getattr(lay, name)
        assert np.array_equal(host.reshape(-1).numpy().astype(np.int64), want[name]), name
    dev = torch.device(DEV)
    dtypes = {name: torch.int32 for name in MAP_NAMES}
    dtypes.update({name: torch.long for name in LAYOUT_NAMES}, query_mask=torch.uint8)
    sentinel = {torch.int32: -1234567, torch.long: -987654321012, torch.uint8: 0xA5}
    bufs, out = {}, _hip.ReplicaMapsOut()
    for name, dt in dtypes.items():
        buf = torch.full((want[name].size + 2 * GUARD,), sentinel[dt], dtype=dt, device=dev)
        bufs[name] = buf
        setattr(out, name, buf.data_ptr() + GUARD * buf.element_size())
    table = lay.table().to(dev)
    _hip.check(_hip.lib().td_replica_maps(table.data_ptr(), b, t, k, hw, L, n, ctypes.byref(out), _hip.stream_ptr()), "td_replica_maps")
    torch.cuda.synchronize()
    host_maps = ReplicaMaps(lay.owner, n, hw, L, "cpu")
    built = ReplicaMaps.from_table(lay, hw, L, dev)
    torch.cuda.synchronize()
    for name, dt in dtypes.items():
        got = bufs[name].cpu()
        assert (got[:GUARD] == sentinel[dt]).all() and (got[-GUARD:] == sentinel[dt]).all(), f"{name}: sentinel overwritten"
        inner = got[GUARD:-GUARD].numpy().astype(np.int64)
        assert np.array_equal(inner, want[name]), name
        if name in MAP_NAMES:
            attr = (lambda m: getattr(m, name[:7])[0 if name.endswith("_idx") else 1]) if name.startswith("seg_") else (lambda m: getattr(m, name))
            assert attr(host_maps).dtype == attr(built).dtype == torch.int32
            assert np.array_equal(attr(host_maps).numpy().astype(np.int64), inner), name
        else:
            attr = lambda m: getattr(m, name)
        assert np.array_equal(attr(built).reshape(-1).cpu().numpy().astype(np.int64), inner), name
    assert built.query_mask.dtype == torch.bool and tuple(built.query_mask.shape) == (b, t) and built.owner.dtype == torch.long
    assert (built.F, built.n, built.hw, built.L, built.S) == (host_maps.F, host_maps.n, host_maps.hw, host_maps.L, host_maps.S)


# ----------------------------------------------------------------------------------------------------------------------------------
# cases, reference, models
# ----------------------------------------------------------------------------------------------------------------------------------
def _case():
    from oracle.weights import synthetic_batch

    return synthetic_batch(T=9, res=RES, k=K, L=L_TOK, seed=33, durations=DURATIONS, text_pad=3)


def _videos_of(batch):
    """The batch as single-video batches (each video alone)."""
    out, s0, f0 = [], 0, 0
    for i, d in enumerate(batch["durations"]):
        c = math.ceil(d / K)
        out.append({"frames": batch["frames"][s0 : s0 + c], "frames_mask": batch["frames_mask"][s0 : s0 + c], "frames_fast": batch["frames_fast"][f0 : f0 + d],
                    "fast_mask": batch["fast_mask"][f0 : f0 + d], "input_ids": batch["input_ids"][i : i + 1], "attention_mask": batch["attention_mask"][i : i + 1], "duration": d})
        s0, f0 = s0 + c, f0 + d
    return out


def _pair_case():
    """Clips of 9 and 3 frames, four captions (clip_index 1, 0, 0, 1) and per-pair boxes drawn as tests/test_multi_sentence_gpu.py draws them
    (manual_seed(1032), caption 2 padded by 3 tokens)."""
    from oracle.weights import synthetic_batch

    clips = synthetic_batch(T=9, res=RES, k=K, L=L_TOK, seed=33, durations=PAIR_CLIPS)
    g = torch.Generator().manual_seed(1032)
    P = len(PAIR_INDEX)
    ids = torch.randint(3, 50000, (P, L_TOK), generator=g)
    ids[:, 0], ids[:, -1] = 0, 2
    att = torch.ones(P, L_TOK, dtype=torch.long)
    ids[2, L_TOK - 3 :] = 1
    ids[2, L_TOK - 3 - 1] = 2
    att[2, L_TOK - 3 :] = 0
    pair_durations = [PAIR_CLIPS[c] for c in PAIR_INDEX]
    n_box = sum(pair_durations)
    cxcy = torch.rand(n_box, 2, generator=g) * 0.6 + 0.2
    wh = torch.rand(n_box, 2, generator=g) * 0.3 + 0.1
    per_pair = {"input_ids": ids, "attention_mask": att, "target_boxes": torch.cat([cxcy, wh], 1), "inter_idx": [[0, d - 1] for d in pair_durations]}
    batch = dict(clips, clip_index=list(PAIR_INDEX), **per_pair)
    alone = _videos_of(clips)
    videos = [dict(alone[c], input_ids=ids[p : p + 1], attention_mask=att[p : p + 1]) for p, c in enumerate(PAIR_INDEX)]
    return batch, videos, pair_durations


def _cfg(fast):
    from oracle.tubedetr_oracle import OracleConfig

    return OracleConfig(stride=K, fast=fast)


def _stitched_step(sd, cfg, videos, target_boxes, inter_idx):
    """Oracle encode + decode of every video alone, stitched into the padded layout (zeros in every padded entry; masks as the padded layout
    defines them), then the oracle's criterion on the stitched outputs."""
    import oracle.tubedetr_oracle as O

    durations = [v["duration"] for v in videos]
    b, t = len(durations), max(durations)
    per = []
    for v in videos:
        cache = O.encode(sd, cfg, v["frames"], v["frames_mask"], [v["duration"]], v["input_ids"], v["attention_mask"],
                         v["frames_fast"] if cfg.fast else None, v["fast_mask"] if cfg.fast else None)
        per.append((cache, O.decode(sd, cfg, cache)))
    S, _, d = per[0][0]["img_memory"].shape
    L = per[0][0]["text_memory"].shape[0]
    cache = {"img_memory": torch.zeros(S, b * t, d), "pos_embed": torch.zeros(S, b * t, d), "text_memory": torch.zeros(L, b * t, d), "query_embed": torch.zeros(t, b, d),
             "text_memory_resized": torch.cat([c["text_memory_resized"] for c, _ in per], 1), "text_attention_mask": torch.cat([c["text_attention_mask"] for c, _ in per], 0),
             "mask": torch.ones(b * t, S, dtype=torch.bool), "query_mask": torch.ones(b, t, dtype=torch.bool)}
    cache["mask"][:, 0] = False
    cache["query_mask"][:, 0] = False
    nl = cfg.dec_layers
    layers = [{"pred_boxes": torch.zeros(b * t, 4), "pred_sted": torch.zeros(b, t, 2), "weights": torch.zeros(b, t, t), "ca_weights": torch.zeros(b * t, 1, S)} for _ in range(nl)]
    for i, ((c, o), dur) in enumerate(zip(per, durations)):
        rows = slice(i * t, i * t + dur)
        for key in ("img_memory", "pos_embed", "text_memory"):
            cache[key][:, rows] = c[key]
        cache["query_embed"][:dur, i] = c["query_embed"][:, 0]
        cache["mask"][rows] = c["mask"]
        cache["mask"][i * t + dur : (i + 1) * t, S - L :] = c["text_attention_mask"][0]  # a padded frame: no visual key but token 0, its video's text mask
        cache["query_mask"][i, :dur] = False
        for l, lo in enumerate(o["aux_outputs"] + [o]):
            layers[l]["pred_boxes"][rows] = lo["pred_boxes"]
            layers[l]["pred_sted"][i, :dur] = lo["pred_sted"][0]
            layers[l]["weights"][i, :dur, :dur] = lo["weights"][0]
            layers[l]["ca_weights"][rows] = lo["ca_weights"]
    out = dict(layers[-1], aux_outputs=layers[:-1])
    keep = O.keep_indices(durations, inter_idx)
    kept = dict(out, pred_boxes=out["pred_boxes"][keep], aux_outputs=[dict(a, pred_boxes=a["pred_boxes"][keep]) for a in out["aux_outputs"]])
    time_mask = torch.zeros(b, t, dtype=torch.bool)
    for i, dur in enumerate(durations):
        time_mask[i, :dur] = True
    ld = O.criterion(kept, target_boxes, inter_idx, time_mask, cfg)
    wd = O.weight_dict(cfg)
    loss = sum(ld[k_] * wd[k_] for k_ in ld if k_ in wd)
    return loss, ld, layers, cache


_REF, _MODELS = {}, {}


def _reference(which):
    """which: ("batch", fast) - the [9, 3, 6] case - or ("pairs", True).  Computed once; gradients for ("batch", True)."""
    if which not in _REF:
        from oracle.weights import fill_state, state_spec

        kind, fast = which
        cfg = _cfg(fast)
        want_grad = which == ("batch", True)
        sd = fill_state(state_spec(cfg), 5, requires_grad=want_grad)
        if kind == "batch":
            batch = _case()
            videos, durations = _videos_of(batch), batch["durations"]
        else:
            batch, videos, durations = _pair_case()
        with torch.set_grad_enabled(want_grad):
            loss, ld, layers, cache = _stitched_step(sd, cfg, videos, batch["target_boxes"], batch["inter_idx"])
        if want_grad:
            loss.backward()
        det = lambda x: x.detach() if torch.is_tensor(x) else x
        _REF[which] = {"loss": loss.detach(), "ld": {k_: v.detach() for k_, v in ld.items()}, "cache": {k_: det(v) for k_, v in cache.items()},
                       "layers": [{k_: det(v) for k_, v in lo.items()} for lo in layers], "durations": durations,
                       "grads": {k_: v.grad for k_, v in sd.items() if v.requires_grad}}
    return _REF[which]


def _model(fast, batch, dtype=torch.float32, fast_mode=""):
    """(model, criterion, weight_dict) with the case's weights, on the GPU, in eval mode, its tokenizer returning ``batch``'s captions."""
    import tubedetr_amd
    from oracle.weights import fill_state, state_spec
    from tubedetr_amd.harness import FixedTokenizer
    from tubedetr_amd.models import build_model

    key = (fast, fast_mode)
    if key not in _MODELS:
        cfg = _cfg(fast)
        torch.manual_seed(0)
        model, criterion, weight_dict = build_model(tubedetr_amd.default_args(stride=cfg.stride, fast=cfg.fast, no_tsa=cfg.no_tsa, compute_dtype=torch.float32,
                                                                              **({"fast_mode": fast_mode} if fast_mode else {})))
        if not fast_mode:  # (an ablation variant has other parameters; it is only asked to refuse)
            model.load_state_dict(fill_state(state_spec(cfg), 5), strict=True)
        model.to(torch.device(DEV))
        _MODELS[key] = (model, criterion, weight_dict)
    model, criterion, weight_dict = _MODELS[key]
    model.transformer.tokenizer = FixedTokenizer(batch["input_ids"], batch["attention_mask"])
    model.set_compute_dtype(dtype).eval()
    for p in model.parameters():
        p.grad = None
    return model, criterion, weight_dict


def _cpu(x):
    return x.detach().float().cpu().numpy()


def _check_forward(loss, ld, out, cache, ref):
    durations = ref["durations"]
    b, t = len(durations), max(durations)
    valid = np.array([j < d for d in durations for j in range(t)])
    # cache: valid-frame columns; per-clip entries and masks in full
    for key in ("img_memory", "pos_embed", "text_memory"):
        assert tuple(cache[key].shape) == tuple(ref["cache"][key].shape), key
        err = np.abs(_cpu(cache[key])[:, valid] - _cpu(ref["cache"][key])[:, valid]).max()
        print(f"cache.{key}: max err {err:.3e}")
        assert err < LOGIT_TOL, (key, err)
    got, want = _cpu(cache["query_embed"]), _cpu(ref["cache"]["query_embed"])
    assert got.shape == want.shape == (t, b, got.shape[2])
    vq = valid.reshape(b, t).T
    err = np.abs(got[vq] - want[vq]).max()
    print(f"cache.query_embed: max err {err:.3e}")
    assert err < LOGIT_TOL
    assert tuple(cache["text_memory_resized"].shape) == tuple(ref["cache"]["text_memory_resized"].shape)
    err = np.abs(_cpu(cache["text_memory_resized"]) - _cpu(ref["cache"]["text_memory_resized"])).max()
    print(f"cache.text_memory_resized: max err {err:.3e}")
    assert err < LOGIT_TOL
    for key in ("mask", "query_mask", "text_attention_mask"):
        assert np.array_equal(cache[key].cpu().numpy().astype(bool), ref["cache"][key].numpy()), key
    n = sum(math.ceil(d / K) for d in durations)
    assert cache["tokenized"]["input_ids"].shape[0] == n and len(cache["tokenized"]._encodings) == n
    layers = out["aux_outputs"] + [out]
    assert len(layers) == len(ref["layers"]) == 6
    vt = valid.reshape(b, t)
    for key in ("pred_boxes", "pred_sted", "weights", "ca_weights"):
        got, want = np.stack([_cpu(o[key]) for o in layers]), np.stack([_cpu(o[key]) for o in ref["layers"]])
        assert got.shape == want.shape, key
        if key in ("pred_boxes", "ca_weights"):  # (layers, b * t, ...)
            sel = np.broadcast_to(valid.reshape((1, b * t) + (1,) * (got.ndim - 2)), got.shape)
        elif key == "pred_sted":
            sel = np.broadcast_to(vt[None, :, :, None], got.shape)
        else:  # weights (layers, b, t, t): valid rows, valid key columns; padded key columns of valid rows are exactly 0
            sel = np.broadcast_to((vt[:, :, None] & vt[:, None, :])[None], got.shape)
            pad_cols = np.broadcast_to((vt[:, :, None] & ~vt[:, None, :])[None], got.shape)
            assert (got[pad_cols] == 0).all(), "attention weight on a time-padded key"
        err = np.abs(got[sel] - want[sel]).max()
        print(f"out.{key}: max err {err:.3e}")
        assert err < LOGIT_TOL, (key, err)
    names = sorted(ld)
    assert names == sorted(ref["ld"]) and len(names) == 24
    print("losses:", [f"{ld[k_].item():.6f}/{ref['ld'][k_].item():.6f}" for k_ in names])
    np.testing.assert_allclose([ld[k_].item() for k_ in names], [ref["ld"][k_].item() for k_ in names], rtol=1e-3, atol=1e-4)
    print(f"total: {loss.item():.6f} / {ref['loss'].item():.6f}")
    assert abs(loss.item() - ref["loss"].item()) <= 1e-3 * abs(ref["loss"].item())


# ----------------------------------------------------------------------------------------------------------------------------------
# 2. - 4. parity
# ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fast", [True, False], ids=["default", "no_fast"])
def test_ragged_batch_matches_single_video_oracle_fp32(fast):
    from tubedetr_amd.harness import batch_to, forward_step

    batch = _case()
    model, criterion, weight_dict = _model(fast, batch)
    with torch.no_grad():
        loss, ld, out, cache = forward_step(model, criterion, weight_dict, batch_to(batch, torch.device(DEV)))
    _check_forward(loss, ld, out, cache, _reference(("batch", fast)))


def test_ragged_batch_backward_matches_oracle_fp32():
    """loss.backward() against the oracle's autograd through the stitched loss (one state dict shared by the single-video passes); every
    trainable parameter, test_pairs_backward_matches_oracle_fp32's acceptance.  Time-padded frames contribute an exactly zero gradient in
    both: the reference has no such frames at all."""
    from tubedetr_amd.harness import batch_to, forward_step

    ref = _reference(("batch", True))
    batch = _case()
    model, criterion, weight_dict = _model(True, batch)
    loss, _, _, _ = forward_step(model, criterion, weight_dict, batch_to(batch, torch.device(DEV)))
    loss.backward()
    torch.cuda.synchronize()
    params = dict(model.named_parameters())
    unused = [k_ for k_, p in params.items() if p.requires_grad and p.grad is None]
    assert unused and all("pooler" in k_ for k_ in unused), unused
    assert sorted(k_ for k_, g in ref["grads"].items() if g is None) == sorted(unused)
    checked = 0
    for k_, g_ref in ref["grads"].items():
        if g_ref is None:
            continue
        g = params[k_].grad
        assert g is not None, k_
        n = g_ref.double().norm().item()
        gn = g.double().norm().item()
        assert abs(gn - n) <= 5e-3 * n + 1e-4, (k_, gn, n)
        np.testing.assert_allclose(g.flatten()[:8].float().cpu().numpy(), g_ref.flatten()[:8].numpy(), rtol=2e-2, atol=2e-3 * max(n, 1e-2), err_msg=k_)
        checked += 1
    assert checked == len(params) - len(unused) - sum(1 for p in params.values() if not p.requires_grad)


def test_several_captions_on_ragged_clips_match_oracle_fp32():
    """Clips of 9 and 3 frames (3 and 1 slow clips), clip_index = [1, 0, 0, 1]: the pair batch [3, 9, 9, 3] is ragged itself.  Reference: the
    oracle on every (clip, caption) pair alone, stitched."""
    from tubedetr_amd.harness import batch_to, forward_step

    batch, _, pair_durations = _pair_case()
    assert pair_durations == [3, 9, 9, 3]
    model, criterion, weight_dict = _model(True, batch)
    with torch.no_grad():
        loss, ld, out, cache = forward_step(model, criterion, weight_dict, batch_to(batch, torch.device(DEV)))
    _check_forward(loss, ld, out, cache, _reference(("pairs", True)))


# ----------------------------------------------------------------------------------------------------------------------------------
# 5. host builders against the device builder
# ----------------------------------------------------------------------------------------------------------------------------------
def _step_bits(model, criterion, weight_dict, batch):
    from tubedetr_amd.harness import forward_step

    for p in model.parameters():
        p.grad = None
    loss, _, out, cache = forward_step(model, criterion, weight_dict, batch)
    loss.backward()
    torch.cuda.synchronize()
    bits = {"loss": loss.detach().clone(), **{k_: out[k_].detach().clone() for k_ in ("pred_boxes", "pred_sted", "weights", "ca_weights")},
            **{"cache." + k_: cache[k_].detach().clone() for k_ in ("img_memory", "pos_embed", "mask", "query_mask", "text_memory_resized")}}
    bits.update({"grad." + k_: p.grad.detach().clone() for k_, p in model.named_parameters() if p.grad is not None})
    return bits


@pytest.mark.parametrize("durations,seed", [([8, 6], 32), ([9, 3, 6], 33)], ids=["8-6", "9-3-6"])
def test_host_and_device_builders_give_the_same_bits(durations, seed):
    """Deterministic mode: outputs, cache and every gradient are bit-equal whichever builder made the index vectors (they are the same
    integers, so the same launches follow); two runs with the default builder are bit-equal too."""
    import tubedetr_amd
    from oracle.weights import synthetic_batch
    from tubedetr_amd import functional as Fk
    from tubedetr_amd.harness import batch_to

    raw = synthetic_batch(T=max(durations), res=RES, k=K, L=L_TOK, seed=seed, durations=durations, text_pad=3)
    model, criterion, weight_dict = _model(True, raw)
    batch = batch_to(raw, torch.device(DEV))
    before = Fk.host_maps()
    tubedetr_amd.set_deterministic(True)
    try:
        Fk.set_host_maps(False)
        runs = [_step_bits(model, criterion, weight_dict, batch), _step_bits(model, criterion, weight_dict, batch)]
        Fk.set_host_maps(True)
        runs.append(_step_bits(model, criterion, weight_dict, batch))
    finally:
        tubedetr_amd.set_deterministic(False)
        Fk.set_host_maps(before)
    assert runs[0].keys() == runs[1].keys() == runs[2].keys() and len(runs[0]) > 300
    for other, what in ((runs[1], "second run, device builder"), (runs[2], "host builder")):
        bad = [k_ for k_ in runs[0] if not torch.equal(runs[0][k_], other[k_])]
        assert not bad, (what, bad[:8])


# ----------------------------------------------------------------------------------------------------------------------------------
# 6. - 8.
# ----------------------------------------------------------------------------------------------------------------------------------
def test_ragged_batch_bf16_close_to_fp32_and_trains():
    """bf16 against the fp32 run of the same call, bounds of test_model_bf16_close_to_fp32_and_trains (0.05 boxes, 0.1 start-end logits);
    then a train-mode step: every trainable parameter but the pooler's gets a finite, non-zero gradient."""
    from tubedetr_amd.harness import batch_to, forward_step

    raw = _case()
    batch = batch_to(raw, torch.device(DEV))
    outs = {}
    for dt in (torch.float32, torch.bfloat16):
        model, criterion, weight_dict = _model(True, raw, dt)
        with torch.no_grad():
            _, _, out, _ = forward_step(model, criterion, weight_dict, batch)
        outs[dt] = {k_: out[k_].float().clone() for k_ in ("pred_boxes", "pred_sted")}
    err_b = (outs[torch.float32]["pred_boxes"] - outs[torch.bfloat16]["pred_boxes"]).abs().max().item()
    err_s = (outs[torch.float32]["pred_sted"] - outs[torch.bfloat16]["pred_sted"]).abs().max().item()
    print(f"bf16 vs fp32: boxes {err_b:.3e}, sted {err_s:.3e}")
    assert err_b < 0.05 and err_s < 0.1
    try:
        model.train()
        torch.manual_seed(3)
        loss, _, _, _ = forward_step(model, criterion, weight_dict, batch)
        assert torch.isfinite(loss)
        loss.backward()
        torch.cuda.synchronize()
        for k_, p in model.named_parameters():
            if p.requires_grad and "pooler" not in k_:
                assert p.grad is not None and torch.isfinite(p.grad).all(), k_
                assert p.grad.abs().sum() > 0, k_
    finally:
        model.set_compute_dtype(torch.float32).eval()


def test_ragged_videos_through_the_uint8_pipeline():
    """uint8 videos of 9, 3 and 6 frames through ClipPipeline.stage (the slow clip is an index list over the fast frames: the de-duplicated
    trunk pass), then harness.forward_step: a finite loss, EQUAL to the loss of the direct model calls on the same staged tensors followed by
    the same (fused) criterion.  Deterministic mode, so that the same launches give the same bits."""
    import tubedetr_amd
    from tubedetr_amd.data import ClipPipeline
    from tubedetr_amd.harness import forward_step
    from tubedetr_amd.util.misc import NestedTensor

    dev = torch.device(DEV)
    g = torch.Generator().manual_seed(7)
    videos = [torch.randint(0, 256, (d, 3, RES, RES), generator=g, dtype=torch.uint8) for d in DURATIONS]
    raw = _case()
    model, criterion, weight_dict = _model(True, raw)
    pipe = ClipPipeline(dev, K)
    batch = pipe.collect(pipe.stage(videos, raw["input_ids"], raw["attention_mask"], raw["target_boxes"], raw["inter_idx"]))
    assert batch["durations"] == DURATIONS and batch["frames"].shape[0] == 6 and batch["frames_fast"].shape[0] == 18
    tubedetr_amd.set_deterministic(True)
    try:
        with torch.no_grad():
            loss_h, ld_h, out_h, _ = forward_step(model, criterion, weight_dict, batch)
            ld_h = {k_: v.clone() for k_, v in ld_h.items()}
            captions = ["caption"] * 3
            cache = model(NestedTensor(batch["frames"], batch["frames_mask"]), DURATIONS, captions, encode_and_save=True,
                          samples_fast=NestedTensor(batch["frames_fast"], batch["fast_mask"]))
            out = model(None, DURATIONS, captions, encode_and_save=False, memory_cache=cache)
            stacked, model._last_stacked = model._last_stacked, None
            t = max(DURATIONS)
            keep = torch.tensor([i * t + j for i, (a, b_) in enumerate(batch["inter_idx"]) for j in range(a, b_ + 1)], device=dev)
            time_mask = torch.tensor([[j < d for j in range(t)] for d in DURATIONS], device=dev)
            ld_d = criterion.forward_fused(stacked, keep, batch["target_boxes"], batch["inter_idx"], time_mask, aux=True)
            loss_d = (criterion.last_loss_matrix * criterion.weight_matrix(weight_dict, stacked["pred_boxes"].shape[0], dev)).sum()
            torch.cuda.synchronize()
    finally:
        tubedetr_amd.set_deterministic(False)
    assert torch.isfinite(loss_h) and sorted(ld_h) == sorted(ld_d) and len(ld_h) == 24
    print(f"harness {loss_h.item():.8f}, direct {loss_d.item():.8f}")
    assert loss_h.item() == loss_d.item()
    for k_ in ld_h:
        assert ld_h[k_].item() == ld_d[k_].item(), k_
    for k_ in ("pred_boxes", "pred_sted"):
        assert torch.equal(out_h[k_], out[k_]), k_
    assert tuple(out_h["pred_boxes"].shape) == (3 * 9, 4) and tuple(out_h["pred_sted"].shape) == (3, 9, 2)


def test_fast_mode_variant_refuses_ragged_clip_counts():
    from tubedetr_amd.harness import batch_to, forward_step

    raw = _case()
    model, criterion, weight_dict = _model(True, raw, fast_mode="gating")
    with torch.no_grad(), pytest.raises(NotImplementedError, match="--fast_mode gating"):
        forward_step(model, criterion, weight_dict, batch_to(raw, torch.device(DEV)))
