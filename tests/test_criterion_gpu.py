"""Fused SetCriterion kernel (csrc/criterion.hip: keep-gather + 24 losses + their derivatives in one launch) against the
CPU oracle's criterion (models/tubedetr.py:270-372,397-460 restated) run in float64, and torch autograd through it: loss
values and the gradients with respect to boxes, start/end logits and attention weights.  Beside the three basic shapes:
T > 256 and more than 256 annotated frames (second pass of every strided loop), unannotated and fully annotated videos,
T = 1, layer counts other than 6, loss subsets (null sted / weights), aux=False, num_boxes as a device scalar, no
annotated frame at all, GIoU on ties / touching / disjoint / contained boxes, an unsorted keep, and two batches that
share every cache key of forward_fused but not their time mask.  Every (layer, loss) gets its own upstream coefficient,
so a wrong layer index in the backward kernel cannot cancel out."""
import contextlib
import types

import pytest
import torch

from criterion_cases import GIOU_EDGE_TABLE, giou_edge_boxes, giou_edge_reference

pytestmark = pytest.mark.gpu

ALL_LOSSES = ("boxes", "sted", "guided_attn")
COLUMNS = ("loss_bbox", "loss_giou", "loss_sted", "loss_guided_attn")


@contextlib.contextmanager
def _default_dtype(dt):
    old = torch.get_default_dtype()
    torch.set_default_dtype(dt)  # the oracle builds its Gaussian targets in the default dtype
    try:
        yield
    finally:
        torch.set_default_dtype(old)


def _close_loss(got, ref):
    return abs(got - ref) <= 2e-5 * max(1.0, abs(ref))


def _close_grad(a, r):
    err = (a.detach().double().cpu() - r).abs().max().item() if r.numel() else 0.0
    return err <= 2e-4 * (r.abs().max().item() if r.numel() else 0.0) + 1e-7, err


def run_case(durations, inter, losses=ALL_LOSSES, aux=True, num_boxes=None, nl=6, *, crit=None, perm=None, boxes=None, tgt=None):
    """One forward_fused + backward on the device against oracle.criterion + autograd on float64 copies of the same inputs.
    ``num_boxes``: None, or (value of the device scalar external_num_boxes, world_size the oracle divides by).  ``perm``:
    order in which keep / tgt rows are handed to the kernel.  ``boxes`` [nl, b*T, 4] / ``tgt`` [n, 4] replace the random ones.
    Returns the fused losses (floats), the gradients (CPU), keep and the [nl, 4] upstream coefficients it drew."""
    from oracle.tubedetr_oracle import OracleConfig, criterion as oracle_criterion
    from tubedetr_amd.models.tubedetr import SetCriterion

    b, T = len(durations), max(durations)
    g = torch.Generator().manual_seed(11)
    mk = lambda *s: torch.cat([torch.rand(*s, 2, generator=g) * 0.5 + 0.25, torch.rand(*s, 2, generator=g) * 0.3 + 0.1], -1)
    rnd_boxes = mk(nl, b * T)                                     # every frame, every layer (cxcywh)
    sted = torch.randn(nl, b, T, 2, generator=g) * 2
    weights = torch.softmax(torch.randn(nl, b, T, T, generator=g) * 2, -1)
    keep = torch.tensor([i * T + f for i, (s, e) in enumerate(inter) if s >= 0 for f in range(s, e + 1)], dtype=torch.long)
    rnd_tgt = mk(keep.numel())
    coef = torch.rand(nl, 4, generator=g) + 0.5                   # independent upstream gradient for every (layer, loss)
    boxes = rnd_boxes if boxes is None else boxes.float()
    tgt = rnd_tgt if tgt is None else tgt.float()
    tm = torch.zeros(b, T, dtype=torch.bool)
    for i, d in enumerate(durations):
        tm[i, :d] = True
    cfg = OracleConfig(sted="sted" in losses, guided_attn="guided_attn" in losses, aux_loss=aux)
    layer_range = range(nl) if aux else (nl - 1,)
    wd = {c + ("" if l == nl - 1 else f"_{l}"): coef[l, j].item() for l in layer_range for j, c in enumerate(COLUMNS)}

    # reference: the oracle's per-layer criterion + engine.py's weighted sum, autograd for the gradients, all in float64
    b64, s64, w64 = (x.double().requires_grad_() for x in (boxes, sted, weights))
    with _default_dtype(torch.float64):
        layers = [{"pred_boxes": b64[l][keep], "pred_sted": s64[l], "weights": w64[l]} for l in range(nl)]
        out = dict(layers[-1])
        if aux:
            out["aux_outputs"] = layers[:-1]
        ref = oracle_criterion(out, tgt.double(), inter, tm, cfg, world_size=1 if num_boxes is None else num_boxes[1])
        total_ref = sum(ref[k] * wd[k] for k in ref)
        total_ref.backward()
    assert all(torch.isfinite(v) for v in ref.values())

    # fused
    dev = torch.device("cuda:0")
    crit = SetCriterion(list(losses), sigma=cfg.sigma) if crit is None else crit
    crit.external_num_boxes = None if num_boxes is None else torch.tensor(float(num_boxes[0]), dtype=torch.float32, device=dev)
    bx, st_, ws = (x.detach().to(dev).requires_grad_() for x in (boxes, sted, weights))
    order = torch.arange(keep.numel()) if perm is None else perm
    got = crit.forward_fused({"pred_boxes": bx, "pred_sted": st_, "weights": ws}, keep[order].to(dev), tgt[order].to(dev), inter, tm.to(dev), aux=aux)
    assert set(got) == set(ref), (sorted(got), sorted(ref))
    n_cols = 2 + ("sted" in losses) + ("guided_attn" in losses)
    assert len(got) == n_cols * len(layer_range)
    got_f = {k: v.item() for k, v in got.items()}
    for k in ref:
        print(f"{k}: fused {got_f[k]:.9g} oracle {ref[k].item():.9g}")
        assert _close_loss(got_f[k], ref[k].item()), (k, got_f[k], ref[k].item())
    total = (crit.last_loss_matrix * crit.weight_matrix(wd, nl, dev)).sum()
    assert abs(total.item() - total_ref.item()) <= 2e-5 * abs(total_ref.item()), (total.item(), total_ref.item())
    total.backward()
    grads = {}
    for name, a, r in (("boxes", bx.grad, b64.grad), ("sted", st_.grad, s64.grad), ("weights", ws.grad, w64.grad)):
        if r is None:  # an input of a loss that is switched off
            assert a is None, name
            continue
        assert torch.isfinite(r).all()
        ok, err = _close_grad(a, r)
        print(f"grad {name}: max err {err:.3g}, max |ref| {r.abs().max().item() if r.numel() else 0.0:.3g}")
        assert ok, (name, err, r.abs().max().item())
        grads[name] = a.detach().cpu()
    return types.SimpleNamespace(losses=got_f, grads=grads, keep=keep, coef=coef.double())


def _keys(nl, columns, aux=True):
    return {c + ("" if l == nl - 1 else f"_{l}") for l in (range(nl) if aux else (nl - 1,)) for c in columns}


@pytest.mark.parametrize("case", [dict(durations=[12], inter=[[0, 11]]), dict(durations=[9, 6], inter=[[2, 7], [0, 3]]),
                                  dict(durations=[100], inter=[[10, 80]])])
def test_fused_criterion_matches_oracle_and_autograd(case):
    r = run_case(case["durations"], case["inter"])
    assert len(r.losses) == 24 and set(r.grads) == {"boxes", "sted", "weights"}


@pytest.mark.parametrize("durations,inter,nl", [
    ([260], [[3, 255]], 6),                                       # second pass of every loop over T; T*T = 67600
    ([130, 130, 40], [[0, 129], [0, 129], [3, 30]], 6),           # n = 288 > 256, b*T*4 = 1560, padded third video
    ([9, 6, 7], [[2, 7], [-100, -100], [6, 6]], 6),               # unannotated video, one-frame interval at the last frame
    ([5, 2], [[4, 4], [0, 1]], 6),                                # video annotated over its whole length: 0 + eps negative rows
    ([1, 1], [[0, 0], [0, 0]], 6),                                # T = 1
    ([9, 6], [[2, 7], [0, 3]], 1),
    ([9, 6], [[2, 7], [0, 3]], 3),
])
def test_fused_criterion_loop_strides_and_annotation_edges(durations, inter, nl):
    r = run_case(durations, inter, nl=nl)
    assert set(r.losses) == _keys(nl, COLUMNS) and set(r.grads) == {"boxes", "sted", "weights"}
    if max(durations) == 1:  # every row lies inside the annotated interval: nothing for the guided-attention loss to sum
        assert all(r.losses[k] == 0.0 for k in _keys(nl, ["loss_guided_attn"]))
        assert not r.grads["weights"].any()
    if durations == [130, 130, 40]:
        assert r.keep.numel() == 288


@pytest.mark.parametrize("losses", [("boxes", "sted"), ("boxes", "guided_attn"), ("boxes",)])
def test_fused_criterion_loss_subsets_pass_null_inputs(losses):
    r = run_case([9, 6], [[2, 7], [0, 3]], losses=losses)
    columns = ["loss_bbox", "loss_giou"] + ["loss_sted"] * ("sted" in losses) + ["loss_guided_attn"] * ("guided_attn" in losses)
    assert set(r.losses) == _keys(6, columns)
    # run_case has checked that the inputs of the absent losses got no gradient at all
    assert set(r.grads) == {"boxes"} | ({"sted"} if "sted" in losses else set()) | ({"weights"} if "guided_attn" in losses else set())


def test_fused_criterion_without_aux_losses():
    r = run_case([9, 6], [[2, 7], [0, 3]], aux=False)
    assert set(r.losses) == set(COLUMNS)
    for name, g_ in r.grads.items():
        assert not g_[:-1].any(), name     # exactly zero for layers 0 .. nl-2
        assert g_[-1].any(), name


def test_fused_criterion_num_boxes_from_a_device_scalar():
    n = 10
    r = run_case([9, 6], [[2, 7], [0, 3]], num_boxes=(n / 2, 2))
    assert r.keep.numel() == n
    run_case([9, 6], [[2, 7], [0, 3]], num_boxes=(0.25, 4 * n))  # below 1: the kernel clamps to 1 like the reference


def test_fused_criterion_time_mask_follows_the_batch():
    """[9, 6] then [9, 8] with one inter_idx share every cache key of forward_fused; each call must use its own mask."""
    from tubedetr_amd.models.tubedetr import SetCriterion

    crit = SetCriterion(list(ALL_LOSSES), sigma=1.0)
    seen = [run_case(durations, [[2, 7], [0, 3]], crit=crit).losses for durations in ([9, 6], [9, 8], [9, 6])]
    assert seen[0] == seen[2]                                      # same inputs, same launch
    assert seen[0]["loss_sted"] != seen[1]["loss_sted"] and seen[0]["loss_guided_attn"] != seen[1]["loss_guided_attn"]
    assert seen[0]["loss_bbox"] == seen[1]["loss_bbox"]           # the boxes never see the mask


def test_fused_criterion_warm_call_does_not_synchronise():
    """A second batch on warm caches (same keys, another mask): argument checks, the mask view, launch and backward must not
    wait for the device; the result is the one a fresh criterion gives."""
    from tubedetr_amd.models.tubedetr import SetCriterion

    dev, nl, b, T, inter = torch.device("cuda:0"), 6, 2, 9, [[2, 7], [0, 3]]
    g = torch.Generator().manual_seed(12)
    keep = torch.tensor([i * T + f for i, (s, e) in enumerate(inter) for f in range(s, e + 1)]).to(dev)
    tgt = (torch.rand(10, 4, generator=g) * 0.3 + 0.2).to(dev)
    stacked = {"pred_boxes": (torch.rand(nl, b * T, 4, generator=g) * 0.3 + 0.2).to(dev).requires_grad_(),
               "pred_sted": torch.randn(nl, b, T, 2, generator=g).to(dev).requires_grad_(),
               "weights": torch.softmax(torch.randn(nl, b, T, T, generator=g), -1).to(dev).requires_grad_()}
    masks = []
    for durations in ([9, 6], [9, 8]):
        tm = torch.zeros(b, T, dtype=torch.bool)
        for i, d in enumerate(durations):
            tm[i, :d] = True
        masks.append(tm.to(dev))
    wd = {c + ("" if l == nl - 1 else f"_{l}"): 1.0 + 0.1 * l + j for l in range(nl) for j, c in enumerate(COLUMNS)}

    def step(crit, tm):
        crit.forward_fused(stacked, keep, tgt, inter, tm)
        L = crit.last_loss_matrix
        (L * crit.weight_matrix(wd, nl, dev)).sum().backward()
        grads = [stacked[k].grad for k in ("pred_boxes", "pred_sted", "weights")]
        for k in stacked:
            stacked[k].grad = None
        return [L.detach()] + grads

    crit = SetCriterion(list(ALL_LOSSES), sigma=1.0)
    step(crit, masks[0])  # fills the caches: positive map, interval table, weight matrix
    torch.cuda.synchronize()
    mode = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        warm = step(crit, masks[1])
    finally:
        torch.cuda.set_sync_debug_mode(mode)
    fresh = step(SetCriterion(list(ALL_LOSSES), sigma=1.0), masks[1])
    for a, f in zip(warm, fresh):
        assert torch.equal(a, f)


def test_fused_criterion_without_any_annotated_frame():
    r = run_case([9, 6], [[-100, -100], [-100, -100]])
    assert r.keep.numel() == 0 and set(r.losses) == _keys(6, COLUMNS)
    assert all(r.losses[k] == 0.0 for k in _keys(6, ["loss_bbox", "loss_giou"]))
    assert not r.grads["boxes"].any()
    # the other terms are unaffected: they matched the oracle in run_case, and they are not trivially zero
    assert r.grads["sted"].any() and r.grads["weights"].any()
    assert all(r.losses[k] > 0.0 for k in _keys(6, ["loss_sted", "loss_guided_attn"]))


def test_fused_criterion_giou_ties_touching_disjoint_contained():
    """Frame i of a fully annotated 8-frame video holds pair i of the edge table, in every layer."""
    nl, n = 6, len(GIOU_EDGE_TABLE)
    pred, tgt = giou_edge_boxes(torch.float32)
    r = run_case([n], [[0, n - 1]], boxes=pred[None].repeat(nl, 1, 1), tgt=tgt)
    loss, d_giou, l1, d_l1 = giou_edge_reference()  # float64 autograd, pair by pair (pinned in tests/test_criterion_cpu.py)
    for l in range(nl):
        sfx = "" if l == nl - 1 else f"_{l}"
        assert _close_loss(r.losses["loss_giou" + sfx], loss.sum().item() / n), (l, r.losses["loss_giou" + sfx], loss.sum().item() / n)
        assert _close_loss(r.losses["loss_bbox" + sfx], l1.sum().item() / n), (l, r.losses["loss_bbox" + sfx], l1.sum().item() / n)
        want = (r.coef[l, 0] * d_l1 + r.coef[l, 1] * d_giou) / n
        ok, err = _close_grad(r.grads["boxes"][l], want)
        print(f"layer {l}: box gradient max err {err:.3g}, max |ref| {want.abs().max().item():.3g}")
        assert ok, (l, err, (r.grads["boxes"][l].double() - want).abs().max(1).values.tolist())


def test_fused_criterion_accepts_an_unsorted_keep():
    durations, inter = [9, 6], [[2, 7], [0, 3]]
    perm = torch.randperm(10, generator=torch.Generator().manual_seed(5))
    assert not torch.equal(perm, torch.arange(10))
    a = run_case(durations, inter)
    p = run_case(durations, inter, perm=perm)  # compared with the oracle's sorted order inside, and with the sorted launch here
    for k in a.losses:
        assert _close_loss(p.losses[k], a.losses[k]), (k, p.losses[k], a.losses[k])
    for name in a.grads:
        ok, err = _close_grad(p.grads[name], a.grads[name].double())
        assert ok, (name, err)

