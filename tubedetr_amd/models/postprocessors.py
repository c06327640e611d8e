"""Evaluation-side post-processors behind the reference's ``models.postprocessors`` interface
(models/postprocessors.py:13-118): ``PostProcessSTVG`` (predicted start / end frame per video, with the ensembling of
several forward windows of one long video) and ``PostProcess`` (boxes to absolute xyxy).  Same call signatures and return
values as the reference's, so engine.evaluate (engine.py:292-340) drives them unchanged; the arithmetic runs on the
device: the constrained arg-max over (start, end) pairs is one HIP launch (td_sted_decode) instead of a (B, T, T) score
tensor and three torch reductions."""
from __future__ import annotations

from typing import Dict, List, NamedTuple, Optional, Tuple

import torch
from torch import nn

from .. import _hip
from ..frame_jobs import release_table, take_table


def sted_decode(steds: torch.Tensor) -> torch.Tensor:
    """steds [n, T, 2] logits (-inf = impossible position) -> int64 [n, 2] (start index, end index), end > start."""
    steds = steds.float().contiguous()
    n, T, _ = steds.shape
    out = torch.empty((n, 2), dtype=torch.int64, device=steds.device)
    _hip.check(_hip.lib().td_sted_decode(_hip.ptr(steds), _hip.ptr(out), n, T, _hip.stream_ptr()), "td_sted_decode")
    return out


class PostProcessSTVG(nn.Module):
    @torch.no_grad()
    def forward(self, outputs, frames_id=None, video_ids=None, time_mask=None):
        """outputs["pred_sted"]: [B, T, 2] logits; frames_id: B increasing lists of frame ids; video_ids: B ids (equal ids =
        consecutive windows of one video, ensembled); time_mask [B, T] False on padded positions.  Returns B' lists
        [start_frame, end_frame (exclusive)], one per distinct video, like the reference."""
        steds = outputs["pred_sted"]
        dev = steds.device
        video_ids = list(video_ids)
        if len(set(video_ids)) != len(video_ids):
            # consecutive windows of the same video: concatenate their (masked) logits along time (postprocessors.py:27-53)
            groups: List[List[int]] = [[0]]
            for i in range(1, len(video_ids)):
                if video_ids[i] == video_ids[i - 1]:
                    groups[-1].append(i)
                else:
                    groups.append([i])
            masked = steds.float().masked_fill(~time_mask[:, :, None], float("-inf"))
            T = steds.shape[1]
            max_dur = max(len(g) for g in groups) * T
            eff = torch.full((len(set(video_ids)), max_dur, 2), float("-inf"), device=dev)
            for i_v, g in enumerate(groups):
                eff[i_v, : len(g) * T] = masked[g].reshape(len(g) * T, 2)
            steds = eff
        pred = sted_decode(steds)  # [B', 2] indices
        max_length = steds.shape[1]
        fid = torch.tensor([list(row) + [0] * (max_length - len(row)) for row in frames_id], dtype=torch.long, device=dev)
        pred = torch.gather(fid, 1, pred).float()
        pred[:, 1] += 1  # the end frame is excluded in evaluation
        return pred.cpu().tolist()


class PostProcess(nn.Module):
    """Boxes cxcywh in [0, 1] -> absolute [x0, y0, x1, y1] (postprocessors.py:86-107)."""

    @torch.no_grad()
    def forward(self, outputs, target_sizes):
        b = outputs["pred_boxes"].float()
        cx, cy, w, h = b.unbind(-1)
        boxes = torch.stack((cx - 0.5 * w, cy - 0.5 * h, cx + 0.5 * w, cy + 0.5 * h), -1)
        img_h, img_w = target_sizes.unbind(1)
        boxes = boxes * torch.stack([img_w, img_h, img_w, img_h], dim=1)
        return [{"boxes": x} for x in boxes]


def build_postprocessors(args, dataset_name) -> Dict[str, nn.Module]:
    post: Dict[str, nn.Module] = {"bbox": PostProcess()}
    if dataset_name in ("vidstg", "hcstvg"):
        post[dataset_name] = PostProcessSTVG()
    return post


# ---- scored K-best moments (td_sted_topk; the rule is the comment in include/tubedetr_hip.h) ----
class Moments(NamedTuple):
    pairs: torch.Tensor   # int64 [n_videos, k, 2]; rows >= count hold (-1, -1)
    scores: torch.Tensor  # fp32 [n_videos, k] log-probabilities, non-increasing; rows >= count hold -inf
    count: torch.Tensor   # int32 [n_videos]


# host tables (window table, frame ids) go up through the frame jobs' pool of (pinned, device, event) triples (frame_jobs.py): the event
# is recorded behind the last launch that reads the device side, and a triple is taken again only once it has completed (a query, never a wait).
def _upload(values: torch.Tensor, device):
    """Host tensor -> (device copy, triple); the caller hands the triple to _release behind the device copy's last reader."""
    nb = values.numel() * values.element_size()
    triple = take_table(nb, device)
    host, dev, _ = triple
    host[:nb].copy_(values.contiguous().view(-1).view(torch.uint8))
    dev[:nb].copy_(host[:nb], non_blocking=True)
    return dev[:nb].view(values.dtype).view(values.shape), triple


_release = release_table


def window_table(video_ids) -> Tuple[List[int], int]:
    """Equal consecutive ids are the windows of one video: -> (win_ptr with one more entry than videos, the largest window count)."""
    video_ids = list(video_ids)
    ptr, seen = [0], set()
    for i, vid in enumerate(video_ids):
        if i and vid != video_ids[i - 1]:
            ptr.append(i)
        if (i == 0 or vid != video_ids[i - 1]) and vid in seen:
            raise ValueError(f"video_ids: {vid!r} comes back at window {i} after another video; the windows of a video are consecutive")
        seen.add(vid)
    ptr.append(len(video_ids))
    return ptr, max((b - a for a, b in zip(ptr, ptr[1:])), default=0)


def _check_moment_args(k, nms):
    if not isinstance(k, int) or isinstance(k, bool) or not 1 <= k <= 32:
        raise ValueError(f"k: an integer in 1..32, not {k!r}")
    if not (isinstance(nms, (tuple, list)) and len(nms) == 2 and all(isinstance(x, int) and not isinstance(x, bool) for x in nms)):
        raise ValueError(f"nms: a pair of integers (numerator, denominator), not {nms!r}")
    if nms[1] < 1 or not 0 <= nms[0] <= nms[1] or nms[1] >= 2 ** 31:
        raise ValueError(f"nms: {nms[0]}/{nms[1]} is not a fraction in [0, 1]")


def moments_topk(steds: torch.Tensor, time_mask: Optional[torch.Tensor] = None, video_ids=None, k: int = 5, nms=(1, 2)) -> Moments:
    """The k likeliest (start, end) position pairs per video that are no near-copies of each other, with their log-probabilities.
    steds [n_windows, T, 2] logits of any float dtype on the device; time_mask [n_windows, T], False on padded positions;
    video_ids: a host list, equal consecutive ids = the windows of one video, whose positions are concatenated (None: every
    window is a video); nms = (numerator, denominator): a pair whose temporal IoU with an earlier pick is ABOVE that fraction is
    dropped ((1, 1): plain top-k).  One launch; device tensors come back and nothing here synchronises."""
    _check_moment_args(k, nms)
    if not (torch.is_tensor(steds) and steds.is_floating_point() and steds.dim() == 3 and steds.shape[2] == 2 and steds.shape[0] >= 1 and steds.shape[1] >= 1):
        raise ValueError("steds: a float tensor [n_windows, T, 2]")
    n_windows, T, _ = steds.shape
    if time_mask is not None and not (torch.is_tensor(time_mask) and tuple(time_mask.shape) == (n_windows, T) and time_mask.device == steds.device):
        raise ValueError(f"time_mask: a tensor [{n_windows}, {T}] on {steds.device}")
    ptr, max_windows = None, 1
    if video_ids is not None:
        ptr, max_windows = window_table(video_ids)
        if ptr[-1] != n_windows:
            raise ValueError(f"video_ids: {ptr[-1]} ids for {n_windows} windows")
    n_videos = n_windows if ptr is None else len(ptr) - 1
    if not steds.is_cuda:
        raise ValueError("steds: on the GPU (there is no host path)")
    dev = steds.device
    with torch.cuda.device(dev):
        z = steds.float().contiguous()
        valid = None if time_mask is None else (time_mask if time_mask.dtype == torch.bool else time_mask != 0).contiguous()
        table, triple = (None, None) if ptr is None else _upload(torch.tensor(ptr, dtype=torch.int32), dev)
        pairs = torch.empty((n_videos, k, 2), dtype=torch.int64, device=dev)
        scores = torch.empty((n_videos, k), dtype=torch.float32, device=dev)
        count = torch.empty((n_videos,), dtype=torch.int32, device=dev)
        try:
            _hip.check(_hip.lib().td_sted_topk(_hip.ptr(z), _hip.ptr(valid), _hip.ptr(table), n_videos, n_windows, T, max_windows, k, nms[0], nms[1],
                                               _hip.ptr(pairs), _hip.ptr(scores), _hip.ptr(count), _hip.stream_ptr()), "td_sted_topk")
        finally:
            if triple is not None:
                _release(triple)
    return Moments(pairs, scores, count)


class PostProcessMoments(nn.Module):
    """The k best moments of every video in frame ids, for a server that stays on the device up to ``render.annotate``:
    ``moments_topk`` over the (windowed) start / end logits, then the frame-id gather and the exclusive end of ``PostProcessSTVG``."""

    def __init__(self, k: int = 5, nms=(1, 2)):
        super().__init__()
        _check_moment_args(k, nms)
        self.k, self.nms = k, tuple(nms)

    @torch.no_grad()
    def forward_device(self, outputs, frames_id, video_ids=None, time_mask=None) -> Moments:
        """-> Moments whose pairs are [start_frame, end_frame (exclusive)] ((-1, -1) in the rows >= count); no host copy."""
        steds = outputs["pred_sted"]
        m = moments_topk(steds, time_mask, video_ids, self.k, self.nms)
        n_videos = m.count.shape[0]
        width = steds.shape[1] * (1 if video_ids is None else window_table(video_ids)[1])
        rows = [list(r) for r in frames_id]
        if len(rows) != n_videos or any(len(r) > width for r in rows):
            raise ValueError(f"frames_id: {n_videos} lists of at most {width} frame ids, one per distinct video")
        fid, triple = _upload(torch.tensor([r + [0] * (width - len(r)) for r in rows], dtype=torch.int64).view(n_videos, width), steds.device)
        spans = torch.gather(fid, 1, m.pairs.clamp(min=0, max=width - 1).view(n_videos, 2 * self.k)).view(n_videos, self.k, 2)
        spans[:, :, 1] += 1  # the end frame is exclusive, as in PostProcessSTVG
        spans = torch.where(m.pairs < 0, m.pairs, spans)
        _release(triple)
        return Moments(spans, m.scores, m.count)

    @torch.no_grad()
    def forward(self, outputs, frames_id, video_ids=None, time_mask=None):
        """-> per distinct video a list of ``count`` dicts {"span": [start_frame, end_frame (exclusive)], "score": log-probability},
        best first; one host copy at the very end."""
        m = self.forward_device(outputs, frames_id, video_ids, time_mask)
        n = m.count.shape[0]
        packed = torch.cat([m.pairs.view(n, -1).double(), m.scores.double(), m.count.double()[:, None]], 1).cpu()  # exact: ids < 2^53
        k = self.k
        return [[{"span": [int(row[2 * i]), int(row[2 * i + 1])], "score": float(row[2 * k + i])} for i in range(int(row[3 * k]))] for row in packed.tolist()]
