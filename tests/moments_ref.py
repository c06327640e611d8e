"""Brute-force float64 restatement of td_sted_topk's rule, written from the comment in include/tubedetr_hip.h (not from
the kernel): all pairs of a video are enumerated, sorted by (-score, e, s) and suppressed with integer arithmetic."""
import math

import torch


def positions(steds, valid=None, win_ptr=None):
    """Per video the float64 logits [P_v, 2] of its positions: the windows' entries in order, padded ones -inf."""
    z = steds.double().clone()
    if valid is not None:
        z[~valid.bool()] = float("-inf")
    if win_ptr is None:
        win_ptr = list(range(z.shape[0] + 1))
    return [z[win_ptr[v]:win_ptr[v + 1]].reshape(-1, 2) for v in range(len(win_ptr) - 1)]


def suppressed(s, e, a, b, num, den):
    inter = max(0, min(e, b) - max(s, a) + 1)
    union = (e - s + 1) + (b - a + 1) - inter
    return inter * den > num * union


def video_topk(z, K, num, den):
    """z float64 [P, 2] -> (picks [(s, e)], scores [float], margins [float]): margins[k] is by how much pick k beats the best
    pair that was admissible in round k and is not pick k (inf when there is none)."""
    P = z.shape[0]
    if P == 0:
        return [], [], []
    ls, le = z[:, 0].log_softmax(0), z[:, 1].log_softmax(0)
    sc = (ls[:, None] + le[None, :]).tolist()
    cand = sorted((-sc[s][e], e, s) for e in range(P) for s in range(e) if math.isfinite(sc[s][e]))
    picks, scores, margins = [], [], []
    for _ in range(K):
        if picks:  # earlier picks were applied in earlier rounds: only the newest one is tested
            a, b = picks[-1]
            cand = [(m, e, s) for m, e, s in cand if (s, e) != (a, b) and not suppressed(s, e, a, b, num, den)]
        if not cand:
            break
        m, e, s = cand[0]
        picks.append((s, e))
        scores.append(-m)
        margins.append(cand[1][0] - m if len(cand) > 1 else float("inf"))
    return picks, scores, margins


def moments_ref(steds, valid=None, win_ptr=None, K=5, nms=(1, 2)):
    """-> pairs int64 [n, K, 2], scores float64 [n, K], count int64 [n], min_margin float (the rule's outputs)."""
    vids = positions(steds, valid, win_ptr)
    n = len(vids)
    pairs = torch.full((n, K, 2), -1, dtype=torch.int64)
    scores = torch.full((n, K), float("-inf"), dtype=torch.float64)
    count = torch.zeros(n, dtype=torch.int64)
    margin = float("inf")
    for v, z in enumerate(vids):
        p, s, m = video_topk(z, K, nms[0], nms[1])
        count[v] = len(p)
        if p:
            pairs[v, :len(p)] = torch.tensor(p)
            scores[v, :len(p)] = torch.tensor(s, dtype=torch.float64)
            margin = min([margin] + m)
    return pairs, scores, count, margin
