"""Device-side input path of a training step.

The reference collates normalised fp32 clips on the host (``video_collate_fn`` / ``NestedTensor.from_tensor_list``,
util/misc.py:40-178), builds the slow clip as a second tensor ``video[:, ::stride]`` (datasets/vidstg.py:250-251) and
copies both to the GPU (engine.py:55-57): 186 MB of fp32 pixels per 100-frame clip at res 352, 25 % of them twice.
``ClipPipeline`` sends every pixel ONCE as uint8 (47 MB per clip) from page-locked staging buffers on a copy stream -
double-buffered, so the copy of batch i+1 overlaps the step of batch i - and leaves the rest to the trunk's input kernel
(td_frames_to_nhwc): ImageNet normalisation, NCHW -> NHWC, bf16 cast, and the slow / fast split as an index list over
the one device buffer (``util.misc.FrameSources``).  The produced batch dict is what ``harness.forward_step`` consumes.
"""
from __future__ import annotations

import math
from typing import List, Optional, Sequence

import torch

from .util.misc import FrameSources


class ClipPipeline:
    def __init__(self, device, stride: int, depth: int = 2):
        self.device = torch.device(device)
        self.stride = int(stride)
        self.copy_stream = torch.cuda.Stream(self.device)
        self.depth = depth
        self._slots: list = [None] * depth  # (pinned video, pinned mask, event of the last H2D out of them)
        self._next = 0
        self._raw_slots: list = [None] * depth  # stage_raw: (pinned decoded frames, pinned job tables, event of the last work that read them)
        self._raw_next = 0

    def _staging(self, n_frames: int, H: int, W: int):
        i = self._next % self.depth
        self._next += 1
        slot = self._slots[i]
        need = n_frames * 3 * H * W
        if slot is None or slot[0].numel() < need or slot[1].numel() < n_frames * H * W:
            slot = [torch.empty(need, dtype=torch.uint8, pin_memory=True), torch.empty(n_frames * H * W, dtype=torch.bool, pin_memory=True), None]
            self._slots[i] = slot
        if slot[2] is not None:
            slot[2].synchronize()  # the copy that last read this staging pair has finished
        return slot

    def stage(self, videos: Sequence[torch.Tensor], input_ids: torch.Tensor, attention_mask: torch.Tensor, target_boxes: torch.Tensor,
              inter_idx: List[List[int]]) -> dict:
        """videos: one uint8 (T_i, 3, H_i, W_i) CPU tensor per video (decoder output order).  Pads to the batch's max H, W
        (mask True = padding, like NestedTensor.from_tensor_list), packs into page-locked memory and starts the
        host-to-device copies on the copy stream.  Returns a ticket for ``collect``."""
        durations = [int(v.shape[0]) for v in videos]
        H, W = max(int(v.shape[2]) for v in videos), max(int(v.shape[3]) for v in videos)
        n = sum(durations)
        vid_pin, mask_pin, _ = slot = self._staging(n, H, W)
        vid = vid_pin[: n * 3 * H * W].view(n, 3, H, W)
        msk = mask_pin[: n * H * W].view(n, H, W)
        off = 0
        ragged = any(v.shape[2] != H or v.shape[3] != W for v in videos)
        if ragged:
            vid.zero_()  # raw 0 is NOT 0 after normalisation: the padded area is zeroed by the input kernel through `valid_hw`
            msk.fill_(True)
        else:
            msk.fill_(False)
        valid_hw = []
        for v in videos:
            assert v.dtype == torch.uint8 and v.dim() == 4 and v.shape[1] == 3, "videos are uint8 (T, 3, H, W)"
            t, _, h, w = v.shape
            vid[off : off + t, :, :h, :w].copy_(v)
            if ragged:
                msk[off : off + t, :h, :w] = False
            valid_hw += [[h, w]] * t
            off += t
        k = self.stride
        slow_idx, base = [], 0
        for d in durations:  # slow clip = every k-th frame of each video (datasets/vidstg.py:250-251)
            slow_idx += [base + j for j in range(0, d, k)]
            base += d
        with torch.cuda.stream(self.copy_stream):
            vid_dev = vid.to(self.device, non_blocking=True)
            msk_dev = msk.to(self.device, non_blocking=True)
            idx_dev = torch.tensor(slow_idx, dtype=torch.int32).pin_memory().to(self.device, non_blocking=True)
            # extent of every frame inside the padded H x W (None for a uniform batch): the reference pads the NORMALISED
            # frames with zeros (NestedTensor.from_tensor_list, util/misc.py:158-170), so padded pixels must be 0 after the
            # device-side normalisation, not (0 - mean) / std
            vhw_dev = torch.tensor(valid_hw, dtype=torch.int32).pin_memory().to(self.device, non_blocking=True) if ragged else None
            ids_dev = input_ids.pin_memory().to(self.device, non_blocking=True)
            att_dev = attention_mask.pin_memory().to(self.device, non_blocking=True)
            box_dev = target_boxes.pin_memory().to(self.device, non_blocking=True)
            ev = torch.cuda.Event()
            ev.record(self.copy_stream)
        slot[2] = ev
        return {"event": ev, "video": vid_dev, "mask": msk_dev, "slow_index": idx_dev, "valid_hw": vhw_dev, "durations": durations, "input_ids": ids_dev,
                "attention_mask": att_dev, "target_boxes": box_dev, "inter_idx": [list(x) for x in inter_idx], "n_slow": len(slow_idx), "slow_index_host": tuple(slow_idx)}

    def _raw_staging(self, n_bytes: int, table_bytes: int):
        i = self._raw_next % self.depth
        self._raw_next += 1
        slot = self._raw_slots[i]
        if slot is None or slot[0].numel() < n_bytes or slot[1].numel() < table_bytes:
            slot = [torch.empty(n_bytes, dtype=torch.uint8, pin_memory=True), torch.empty(max(table_bytes, 4096), dtype=torch.uint8, pin_memory=True), None]
            self._raw_slots[i] = slot
        if slot[2] is not None:
            slot[2].synchronize()  # the copy and the launches that last read this staging pair have finished
        return slot

    def stage_raw(self, videos: Sequence, plans: Sequence, input_ids: torch.Tensor, attention_mask: torch.Tensor, inter_idx: List[List[int]]) -> dict:
        """videos: per video its frames AS DECODED at the video's own size: a uint8 (T_i, h_i, w_i, 3) CPU array / tensor
        (rgb24, datasets/vidstg.py:109-115) or a ``tubedetr_amd.augment.DecodedClip`` (the decoder's native yuv420p /
        nv12 buffer: half the bytes, no colour conversion on the host; formats may be mixed); plans: its ``ClipPlan``
        (tubedetr_amd.augment: ``make_video_transforms(...).plan``).
        Packs the decoded frames into page-locked memory, copies them ONCE on the copy stream and enqueues the resample
        launches there (td_clip_resample / td_clip_resample_src: colour conversion, flip, resize, crop, second resize,
        padding and padding mask; the launch that reads a clip converts it, the intermediate between the two training
        resizes is rgb); the ticket is what ``stage`` returns, so ``collect`` gives the same batch dict.
        ``target_boxes`` are the annotated frames' boxes of the plans.  Temporal cropping stays with the caller: slice
        the array (and the targets) before this."""
        from . import _hip
        from .augment import DecodedClip, resample_job, resample_src_job

        vids = []
        for v in videos:
            if not isinstance(v, DecodedClip):
                v = torch.as_tensor(v)
                assert v.dtype == torch.uint8 and v.dim() == 4 and v.shape[3] == 3 and not v.is_cuda, "videos are uint8 (T, h, w, 3) on the host, or DecodedClips"
                v = DecodedClip(v, v.shape[0], v.shape[1], v.shape[2], "rgb24")
            vids.append(v)
        assert len(vids) == len(plans) == len(inter_idx)
        durations = [v.T for v in vids]
        H, W = max(int(p.hw[0]) for p in plans), max(int(p.hw[1]) for p in plans)
        n = sum(durations)
        boxes = []
        for p, v, inter in zip(plans, vids, inter_idx):
            assert len(p.targets) == v.T and tuple(p.src_hw) == (v.h, v.w), "the plan was drawn for another clip"
            if inter and inter[0] >= 0:  # number of boxes = number of frames in the annotated moment (datasets/vidstg.py:140-147)
                n_boxed = len([t for t in p.targets if len(t["boxes"])])
                assert n_boxed == inter[-1] - inter[0] + 1, (n_boxed, inter)
            boxes += [t["boxes"] for t in p.targets if len(t["boxes"])]
        target_boxes = torch.cat(boxes) if boxes else torch.zeros(0, 4)
        offs, total = [], 0
        for v in vids:
            offs.append(total)
            total += (v.nbytes + 15) // 16 * 16
        lib = _hip.lib()
        # a launch whose jobs all read rgb24 is td_clip_resample's, as before there were other formats
        yuv = [[v.pix_fmt != "rgb24" for v, p in zip(vids, plans) if len(p.stages) == 2], [v.pix_fmt != "rgb24" and len(p.stages) == 1 for v, p in zip(vids, plans)]]
        tb = [int((lib.td_clip_resample_src_table_bytes if any(y) else lib.td_clip_resample_table_bytes)(len(y))) for y in yuv]
        raw_pin, tab_pin, _ = slot = self._raw_staging(total, tb[0] + tb[1])
        for v, o in zip(vids, offs):
            raw_pin[o : o + v.nbytes].copy_(v.data)

        def job(use_src, src, d, sh, sw, flip, stage, dst, fmt, **kw):
            if use_src:
                return resample_src_job(src, d, sh, sw, flip, stage, dst, *fmt, **kw)
            return resample_job(src, d, sh, sw, flip, stage, dst, **kw)

        ragged = any(tuple(p.hw) != (H, W) for p in plans)
        valid_hw = []
        for p, d in zip(plans, durations):
            valid_hw += [[int(p.hw[0]), int(p.hw[1])]] * d
        k = self.stride
        slow_idx, base = [], 0
        for d in durations:  # slow clip = every k-th frame of each video (datasets/vidstg.py:250-251)
            slow_idx += [base + j for j in range(0, d, k)]
            base += d
        with torch.cuda.stream(self.copy_stream):
            raw_dev = raw_pin[:total].to(self.device, non_blocking=True)
            vid_dev = torch.empty((n, 3, H, W), dtype=torch.uint8, device=self.device)
            msk_dev = torch.empty((n, H, W), dtype=torch.bool, device=self.device)
            tab_dev = torch.empty(tb[0] + tb[1], dtype=torch.uint8, device=self.device)
            # raw_dev, tab_dev and the intermediates are allocated AND consumed on the copy stream only: the caching allocator
            # hands their memory to later work of that stream alone, so they may go out of scope once the launches are enqueued
            first, final, keep, off = [], [], [], 0
            for v, p, o, d in zip(vids, plans, offs, durations):
                src, sh, sw, flip, fmt = raw_dev.data_ptr() + o, v.h, v.w, p.flip, (v.pix_fmt, v.matrix, v.full_range)
                if len(p.stages) == 2:  # resize + crop into an interleaved uint8 intermediate (the reference rounds to uint8 there)
                    s = p.stages[0]
                    mid = torch.empty((d, s.wh, s.ww, 3), dtype=torch.uint8, device=self.device)
                    keep.append(mid)
                    first.append(job(any(yuv[0]), src, d, sh, sw, flip, s, mid.data_ptr(), fmt))
                    src, sh, sw, flip, fmt = mid.data_ptr(), s.wh, s.ww, False, ("rgb24", "bt601", False)
                s = p.stages[-1]
                assert (s.wh, s.ww) == tuple(p.hw)
                final.append(job(any(yuv[1]), src, d, sh, sw, flip, s, vid_dev.data_ptr(), fmt, planar=True, frame_off=off, H=H, W=W, mask=msk_dev.data_ptr()))
                off += d
            t_off = 0
            for jobs, nb, src_fmt in ((first, tb[0], any(yuv[0])), (final, tb[1], any(yuv[1]))):
                if jobs:
                    if src_fmt:
                        arr = (_hip.ResampleSrcJob * len(jobs))(*jobs)
                        _hip.check(lib.td_clip_resample_src(arr, len(jobs), tab_pin.data_ptr() + t_off, tab_dev.data_ptr() + t_off, nb, _hip.stream_ptr()), "td_clip_resample_src")
                    else:
                        arr = (_hip.ResampleJob * len(jobs))(*jobs)
                        _hip.check(lib.td_clip_resample(arr, len(jobs), tab_pin.data_ptr() + t_off, tab_dev.data_ptr() + t_off, nb, _hip.stream_ptr()), "td_clip_resample")
                t_off += nb
            idx_dev = torch.tensor(slow_idx, dtype=torch.int32).pin_memory().to(self.device, non_blocking=True)
            vhw_dev = torch.tensor(valid_hw, dtype=torch.int32).pin_memory().to(self.device, non_blocking=True) if ragged else None
            ids_dev = input_ids.pin_memory().to(self.device, non_blocking=True)
            att_dev = attention_mask.pin_memory().to(self.device, non_blocking=True)
            box_dev = target_boxes.pin_memory().to(self.device, non_blocking=True)
            ev = torch.cuda.Event()
            ev.record(self.copy_stream)
        slot[2] = ev
        return {"event": ev, "video": vid_dev, "mask": msk_dev, "slow_index": idx_dev, "valid_hw": vhw_dev, "durations": durations, "input_ids": ids_dev,
                "attention_mask": att_dev, "target_boxes": box_dev, "inter_idx": [list(x) for x in inter_idx], "n_slow": len(slow_idx), "slow_index_host": tuple(slow_idx)}

    def collect(self, ticket: dict) -> dict:
        """Batch dict for ``harness.forward_step``; the current stream waits for the ticket's copies (no host sync)."""
        cur = torch.cuda.current_stream(self.device)
        cur.wait_event(ticket["event"])
        for k_ in ("video", "mask", "slow_index", "valid_hw", "input_ids", "attention_mask", "target_boxes"):
            if ticket[k_] is not None:
                ticket[k_].record_stream(cur)  # allocated on the copy stream, consumed on the compute stream
        video, mask, idx, vhw = ticket["video"], ticket["mask"], ticket["slow_index"], ticket["valid_hw"]
        return {
            "frames": FrameSources([(video, idx)], [vhw], [ticket["slow_index_host"]]),   # slow clip: an index list over the same pixels (+ its host copy: the model proves slow = fast[::k] from it)
            "frames_mask": mask[idx.long()],
            "frames_fast": FrameSources([(video, None)], [vhw]) if vhw is not None else video,  # uint8; normalised by the trunk's input kernel
            "fast_mask": mask,
            "durations": ticket["durations"],
            "input_ids": ticket["input_ids"],
            "attention_mask": ticket["attention_mask"],
            "target_boxes": ticket["target_boxes"],
            "inter_idx": ticket["inter_idx"],
        }
