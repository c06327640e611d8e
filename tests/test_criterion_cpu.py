"""Host side of the fused criterion without a GPU (no kernel is launched): forward_fused hands every call its own time
mask, CriterionFn.forward refuses dtypes and shapes the kernel would misread, and the oracle's GIoU (the reference the
GPU test compares the kernel with) is pinned on box pairs where min / max tie and clamp(min=0) sits exactly at 0."""
import types
from fractions import Fraction

import pytest
import torch

from criterion_cases import GIOU_EDGE_TABLE, giou_edge_boxes, giou_edge_reference
from tubedetr_amd.models import tubedetr as td_model
from tubedetr_amd.models.tubedetr import CriterionFn, SetCriterion


def _time_mask(durations):
    tm = torch.zeros(len(durations), max(durations), dtype=torch.bool)
    for i, d in enumerate(durations):
        tm[i, :d] = True
    return tm


def test_forward_fused_hands_over_each_calls_own_time_mask(monkeypatch):
    """Two batches with the same inter_idx and the same longest video share every cache key of forward_fused; only the
    shorter video's duration differs.  Each call's kernel arguments must carry that call's mask."""
    seen = []

    def recorder(boxes, sted, weights, tgt, keep, tm_u8, pm_u8, inter_dev, num_boxes, sigma):
        assert tm_u8.dtype == torch.uint8 and pm_u8.dtype == torch.uint8 and inter_dev.dtype == torch.int32
        seen.append((tm_u8.clone(), pm_u8.clone(), inter_dev.clone()))
        return torch.zeros(boxes.shape[0], 4)

    monkeypatch.setattr(td_model.CriterionFn, "apply", staticmethod(recorder))
    crit = SetCriterion(["boxes", "sted", "guided_attn"], sigma=1.0)
    inter, nl, b, T = [[2, 7], [0, 3]], 6, 2, 9
    keep = torch.tensor([i * T + f for i, (s, e) in enumerate(inter) for f in range(s, e + 1)])
    stacked = {"pred_boxes": torch.rand(nl, b * T, 4), "pred_sted": torch.randn(nl, b, T, 2), "weights": torch.rand(nl, b, T, T)}
    sequence = ([9, 6], [9, 8], [9, 6])
    for durations in sequence:
        crit.forward_fused(stacked, keep, torch.rand(keep.numel(), 4), inter, _time_mask(durations))
    assert len(seen) == 3
    for durations, (tm_u8, pm_u8, inter_dev) in zip(sequence, seen):
        assert tm_u8.sum(1).tolist() == durations, (durations, tm_u8.sum(1).tolist())
        assert torch.equal(tm_u8, _time_mask(durations).to(torch.uint8))
        # what the key does determine stays right on a cache hit
        assert pm_u8.sum(1).tolist() == [6, 4] and inter_dev.tolist() == inter


def _args(nl=2, b=2, T=5, n=3):
    return dict(boxes=torch.rand(nl, b * T, 4), sted=torch.randn(nl, b, T, 2), weights=torch.rand(nl, b, T, T), tgt=torch.rand(n, 4),
                keep=torch.arange(n), tm_u8=torch.ones(b, T, dtype=torch.uint8), pm_u8=torch.zeros(b, T, dtype=torch.uint8),
                inter_dev=torch.zeros(b, 2, dtype=torch.int32), num_boxes=float(n), sigma=1.0)


@pytest.mark.parametrize("field,change,error", [
    ("keep", lambda x: x.int(), TypeError),
    ("boxes", lambda x: x.double(), TypeError),
    ("boxes", lambda x: x.bfloat16(), TypeError),
    ("sted", lambda x: x.half(), TypeError),
    ("weights", lambda x: x.bfloat16(), TypeError),
    ("tm_u8", lambda x: x.bool(), TypeError),
    ("boxes", lambda x: x[:, :-1], ValueError),                  # boxes.shape[1] != b*T
    ("boxes", lambda x: x[:, :, :3], ValueError),
    ("sted", lambda x: x[:, :, :-1], ValueError),                # T disagrees with time_mask
    ("sted", lambda x: x[:-1], ValueError),                      # layer count disagrees with boxes
    ("weights", lambda x: x[:, :, :, :-1], ValueError),          # not [b, T, T]
    ("weights", lambda x: x[:, :1], ValueError),
    ("tgt", lambda x: x[:-1], ValueError),                       # one target row per keep index
    ("pm_u8", lambda x: x[:, :-1], ValueError),
])
def test_criterion_fn_refuses_what_the_kernel_would_misread(field, change, error):
    a = _args()
    a[field] = change(a[field])
    named = {"tm_u8": "time_mask", "pm_u8": "positive_map"}.get(field, field)
    with pytest.raises(error, match=f"CriterionFn: .*{named}"):
        CriterionFn.apply(*a.values())


def test_criterion_fn_checks_come_before_the_device_assertion(monkeypatch):
    # well-formed CPU arguments pass every check and stop at the GPU-only assertion of _hip.ptr, before any launch
    from tubedetr_amd import _hip

    def launched(*a):
        raise RuntimeError("a launch was reached with CPU tensors")

    monkeypatch.setattr(_hip, "lib", lambda: types.SimpleNamespace(td_criterion_fwd=launched))
    with pytest.raises(AssertionError, match="only run on the GPU"):
        CriterionFn.apply(*_args().values())
    a = _args()
    a["sted"] = a["weights"] = None  # the loss list ["boxes"]: absent inputs are not checked
    with pytest.raises(AssertionError, match="only run on the GPU"):
        CriterionFn.apply(*a.values())


# ---- GIoU edge table ----
def _exact_giou_loss(p, t):
    """1 - GIoU of two cxcywh boxes in exact rational arithmetic (every table entry is dyadic)."""
    (pcx, pcy, pw, ph), (tcx, tcy, tw, th) = ([Fraction(v) for v in p], [Fraction(v) for v in t])
    a = (pcx - pw / 2, pcy - ph / 2, pcx + pw / 2, pcy + ph / 2)
    b = (tcx - tw / 2, tcy - th / 2, tcx + tw / 2, tcy + th / 2)
    inter = max(min(a[2], b[2]) - max(a[0], b[0]), 0) * max(min(a[3], b[3]) - max(a[1], b[1]), 0)
    union = pw * ph + tw * th - inter
    hull = (max(a[2], b[2]) - min(a[0], b[0])) * (max(a[3], b[3]) - min(a[1], b[1]))
    return 1 - (inter / union - (hull - union) / hull)


def _tie_rule_giou_grad(pred, tgt):
    """d(1 - giou)/d pred (cxcywh) by hand, float64, with torch's rules written out: min / max give each argument half
    of the gradient on a tie, clamp(min=0) passes the gradient at exactly 0.  This is the rule set csrc/criterion.hip
    hand-codes; the test below shows that it is what autograd through the oracle does."""
    out = []
    for s, g in zip(pred.tolist(), tgt.tolist()):
        ax1, ay1, ax2, ay2 = s[0] - 0.5 * s[2], s[1] - 0.5 * s[3], s[0] + 0.5 * s[2], s[1] + 0.5 * s[3]
        bx1, by1, bx2, by2 = g[0] - 0.5 * g[2], g[1] - 0.5 * g[3], g[0] + 0.5 * g[2], g[1] + 0.5 * g[3]
        area_a, area_b = (ax2 - ax1) * (ay2 - ay1), (bx2 - bx1) * (by2 - by1)
        iw, ih = min(ax2, bx2) - max(ax1, bx1), min(ay2, by2) - max(ay1, by1)
        iwc, ihc = max(iw, 0.0), max(ih, 0.0)
        inter = iwc * ihc
        uni = area_a + area_b - inter
        ew, eh = max(max(ax2, bx2) - min(ax1, bx1), 0.0), max(max(ay2, by2) - min(ay1, by1), 0.0)
        hull = ew * eh
        up = -1.0  # upstream of giou in 1 - giou
        g_uni = up * (-inter / (uni * uni) + 1.0 / hull)
        g_hull = up * (-uni / (hull * hull))
        g_inter = up / uni - g_uni
        g_iw, g_ih = (g_inter * ihc if iw >= 0 else 0.0), (g_inter * iwc if ih >= 0 else 0.0)
        g_ew, g_eh = g_hull * eh, g_hull * ew
        lt = lambda a, b: 1.0 if a < b else (0.5 if a == b else 0.0)
        gx1 = -g_iw * lt(bx1, ax1) - g_ew * lt(ax1, bx1) - g_uni * (ay2 - ay1)
        gx2 = g_iw * lt(ax2, bx2) + g_ew * lt(bx2, ax2) + g_uni * (ay2 - ay1)
        gy1 = -g_ih * lt(by1, ay1) - g_eh * lt(ay1, by1) - g_uni * (ax2 - ax1)
        gy2 = g_ih * lt(ay2, by2) + g_eh * lt(by2, ay2) + g_uni * (ax2 - ax1)
        out.append([gx1 + gx2, gy1 + gy2, 0.5 * (gx2 - gx1), 0.5 * (gy2 - gy1)])
    return torch.tensor(out, dtype=torch.float64)


def test_oracle_giou_on_ties_touching_disjoint_and_contained_boxes():
    loss, grad, l1, l1_grad = giou_edge_reference()
    assert torch.isfinite(loss).all() and torch.isfinite(grad).all()
    for i, (name, p, t) in enumerate(GIOU_EDGE_TABLE):
        want = _exact_giou_loss(p, t)
        assert abs(loss[i].item() - float(want)) <= 1e-15, (name, loss[i].item(), want)
        assert l1[i].item() == float(sum(abs(Fraction(a) - Fraction(b)) for a, b in zip(p, t))), name
    # facts that need no arithmetic
    assert loss[0].item() == 0.0                                 # identical boxes
    assert loss[4].item() > 1.0 and loss[3].item() > 1.0         # disjoint / touching only in a corner: giou < 0
    pred, tgt = giou_edge_boxes()
    assert torch.equal(l1_grad, torch.sign(pred - tgt))          # |d| has gradient 0 at d == 0
    hand = _tie_rule_giou_grad(pred, tgt)
    err = (hand - grad).abs().max(1).values
    for i, (name, _, _) in enumerate(GIOU_EDGE_TABLE):
        assert err[i].item() <= 1e-13, (name, hand[i].tolist(), grad[i].tolist())
    # the table is only worth pinning if it is exact in float32 too: both precisions must take the same branches
    p32, t32 = giou_edge_boxes(torch.float32)
    assert torch.equal(p32.double(), pred) and torch.equal(t32.double(), tgt)
