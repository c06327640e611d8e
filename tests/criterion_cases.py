"""Shared by tests/test_criterion_cpu.py and tests/test_criterion_gpu.py: the GIoU edge table (box pairs on which min / max
tie or clamp(min=0) sits exactly at 0) and its float64 autograd reference through the oracle's giou_diag.  Every coordinate
is dyadic, so every edge comparison is exact in float32 as well and both sides take the same branch."""
import torch

# name, predicted (cx, cy, w, h), target (cx, cy, w, h)
GIOU_EDGE_TABLE = [
    ("identical", (.5, .5, .25, .25), (.5, .5, .25, .25)),
    ("shared left edge", (.5, .5, .25, .25), (.5625, .5, .375, .125)),
    ("touching in x", (.25, .5, .25, .25), (.5, .5, .25, .5)),
    ("touching corner", (.25, .25, .25, .25), (.5, .5, .25, .25)),
    ("disjoint", (.25, .25, .125, .125), (.75, .75, .25, .125)),
    ("contained", (.5, .5, .5, .5), (.5, .5, .25, .125)),
    ("contained, shared edge", (.5, .5, .5, .5), (.375, .5, .25, .25)),
    ("same centre, crossed", (.5, .5, .5, .125), (.5, .5, .125, .5)),
]


def giou_edge_boxes(dtype=torch.float64):
    pred = torch.tensor([p for _, p, _ in GIOU_EDGE_TABLE], dtype=dtype)
    tgt = torch.tensor([t for _, _, t in GIOU_EDGE_TABLE], dtype=dtype)
    return pred, tgt


def giou_edge_reference():
    """Per pair, in float64 through torch autograd: 1 - giou, d(1 - giou)/d pred, the L1 distance and d L1/d pred."""
    from oracle.tubedetr_oracle import cxcywh_to_xyxy, giou_diag

    pred, tgt = giou_edge_boxes()
    p1 = pred.clone().requires_grad_()
    loss = 1 - giou_diag(cxcywh_to_xyxy(p1), cxcywh_to_xyxy(tgt))
    loss.sum().backward()
    p2 = pred.clone().requires_grad_()
    l1 = (p2 - tgt).abs().sum(1)
    l1.sum().backward()
    return loss.detach(), p1.grad, l1.detach(), p2.grad
