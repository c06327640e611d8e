"""Spatial clip augmentation with the pixel work on the device (td_clip_resample, csrc/augment.hip).

The reference transforms a decoded clip on the host, frame by frame (``make_video_transforms``,
datasets/video_transforms.py:327-443: random horizontal flip, random resize, random size crop, second resize, box
bookkeeping, caption left/right swap; at evaluation one resize).  Here the host only DRAWS: ``plan`` consumes Python's
``random`` and torch's generator in the reference's order, does the box arithmetic in the reference's fp32 operations,
and returns a small record that says which resamples the device has to run; ``ClipPipeline.stage_raw``
(tubedetr_amd/data.py) sends the decoded frames once, as they came out of the decoder - rgb24 arrays, or yuv420p / nv12
buffers described by a ``DecodedClip``, half the bytes - and enqueues those launches.
"""
from __future__ import annotations

import random
from dataclasses import dataclass, field
from typing import List, Optional, Sequence, Tuple

import torch

from . import _hip
from .frame_jobs import _MATRICES, _PIX_FMTS, _describe, _frame_bytes, _planes, _put_planes, clip_resample, clip_resample_src  # noqa: F401  (the launchers are part of this module's interface)

# resolution -> (scales, max_size, resizes, crop, test_size)  (datasets/video_transforms.py:339-405)
_TABLE = {
    128: ([96, 128], 213, [80, 100, 120], 64, [128]),
    224: ([128, 160, 192, 224], 373, [100, 150, 200], 96, [224]),
    256: ([160, 192, 224, 256], 427, [140, 180, 220], 128, [256]),
    288: ([160, 192, 224, 256, 288], 480, [150, 200, 250], 128, [288]),
    320: ([192, 224, 256, 288, 320], 533, [200, 240, 280], 160, [320]),
    352: ([224, 256, 288, 320, 352], 587, [200, 250, 300], 192, [352]),
    384: ([224, 256, 288, 320, 352, 384], 640, [200, 250, 300], 192, [384]),
    416: ([256, 288, 320, 352, 384, 416], 693, [240, 300, 360], 224, [416]),
    448: ([256, 288, 320, 352, 384, 416, 448], 746, [240, 300, 360], 224, [448]),
    480: ([288, 320, 352, 384, 416, 448, 480], 800, [240, 300, 360], 240, [480]),
    800: ([480, 512, 544, 576, 608, 640, 672, 704, 736, 768, 800], 1333, [400, 500, 600], 384, [800]),
}


def get_size_with_aspect_ratio(image_size: Tuple[int, int], size: int, max_size: Optional[int] = None) -> Tuple[int, int]:
    """(w, h), shorter-side target, longer-side limit -> (oh, ow), with the reference's ``int(round(...))`` and
    ``int(size * h / w)`` truncations (datasets/video_transforms.py:138-158)."""
    w, h = image_size
    if max_size is not None:
        lo, hi = float(min((w, h))), float(max((w, h)))
        if hi / lo * size > max_size:
            size = int(round(max_size * lo / hi))
    if (w <= h and w == size) or (h <= w and h == size):
        return (h, w)
    if w < h:
        return (int(size * h / w), size)
    return (size, int(size * w / h))


@dataclass
class ResampleStage:
    """Virtual bilinear resize of the stage's input to rh x rw, of which the window (wy, wx, wh, ww) is produced."""
    rh: int
    rw: int
    wy: int
    wx: int
    wh: int
    ww: int


@dataclass
class ClipPlan:
    flip: bool                      # the FIRST stage reads source column j as column w - 1 - j
    stages: List[ResampleStage]     # one (plain resize) or two (resize + crop, then resize; uint8 in between)
    hw: Tuple[int, int]             # final (H, W)
    targets: List[dict]             # per frame: boxes (normalised cxcywh, fp32), size, orig_size
    caption: str
    crop_tries: int = 0             # draws of the random size crop (100 with a fall-back to the uncropped clip)
    src_hw: Tuple[int, int] = field(default=(0, 0))


def _swap_left_right(caption: str) -> str:
    return caption.replace("left", "[TMP]").replace("right", "left").replace("[TMP]", "right")


def _crop_boxes(boxes: torch.Tensor, region):
    """Boxes after a crop and which of them keep an area (the others are dropped, datasets/video_transforms.py:249-277)."""
    i, j, h, w = region
    c = boxes - torch.as_tensor([j, i, j, i])
    c = torch.min(c.reshape(-1, 2, 2), torch.as_tensor([w, h], dtype=torch.float32)).clamp(min=0)
    keep = torch.all(c[:, 1, :] > c[:, 0, :], dim=1)
    return c.reshape(-1, 4), keep


class VideoTransformPlanner:
    def __init__(self, image_set: str, cautious: bool, scales, max_size, resizes, crop, test_size):
        self.image_set, self.cautious = image_set, bool(cautious)
        self.scales, self.max_size, self.resizes, self.crop, self.test_size = scales, max_size, resizes, crop, test_size

    def _resize(self, st: dict, sizes, max_size) -> Tuple[int, int]:
        """One RandomResize on the running state: the size draw and the box scaling."""
        size = random.choice(sizes)
        w, h = st["w"], st["h"]
        oh, ow = get_size_with_aspect_ratio((w, h), size, max_size)
        rw_, rh_ = float(ow) / float(w), float(oh) / float(h)
        scale = torch.as_tensor([rw_, rh_, rw_, rh_])
        st["boxes"] = st["boxes"] * scale
        st["w"], st["h"] = ow, oh
        return oh, ow

    def _size_crop(self, st: dict):
        """RandomSizeCrop(crop, max_size, respect_boxes=cautious), datasets/video_transforms.py:277-324.  Returns the
        region, or None for the fall-back to the uncropped clip, and the number of draws.  As in the reference, a try
        crops the boxes the PREVIOUS try left behind (the reference writes them back into the dicts its loop holds), so
        once a try has dropped a box no later try can restore the count: the loop runs all its 100 draws and falls back."""
        w, h = st["w"], st["h"]
        orig, orig_frame = st["boxes"], st["frame"]
        init = len(orig)
        cur, frame = orig, orig_frame
        for i_try in range(100):
            tw = random.randint(self.crop, min(w, self.max_size))
            th = random.randint(self.crop, min(h, self.max_size))
            if h + 1 < th or w + 1 < tw:
                raise ValueError("Required crop size {} is larger then input image size {}".format((th, tw), (h, w)))
            if w == tw and h == th:
                region = (0, 0, h, w)
            else:
                i = torch.randint(0, h - th + 1, size=(1,)).item()
                j = torch.randint(0, w - tw + 1, size=(1,)).item()
                region = (i, j, th, tw)
            cur, keep = _crop_boxes(cur, region)
            cur, frame = cur[keep], frame[keep]
            if (not self.cautious) or len(cur) == init:
                st["boxes"], st["frame"], st["w"], st["h"] = cur, frame, region[3], region[2]
                return region, i_try + 1
        st["boxes"], st["frame"] = orig, orig_frame
        return None, 100

    def plan(self, w: int, h: int, targets: Sequence[dict], caption: str) -> ClipPlan:
        """w, h: the decoded frames' size; targets: per frame a dict with ``boxes`` = (n, 4) fp32 xyxy in source pixels
        (what the reference's ``prepare`` makes); caption: the clip's sentence."""
        w, h = int(w), int(h)
        # the boxes of all frames as ONE (N, 4) tensor + the frame each belongs to: the same fp32 operations per element as frame by frame
        per_frame = [torch.as_tensor(t["boxes"], dtype=torch.float32).reshape(-1, 4) for t in targets]
        st = {"w": w, "h": h, "boxes": torch.cat(per_frame) if per_frame else torch.zeros(0, 4),
              "frame": torch.tensor([i for i, b in enumerate(per_frame) for _ in range(len(b))], dtype=torch.long)}
        flip, stages, tries = False, [], 0
        if self.image_set == "train":
            if not self.cautious and random.random() < 0.5:
                flip = True
                st["boxes"] = st["boxes"][:, [2, 1, 0, 3]] * torch.as_tensor([-1, 1, -1, 1]) + torch.as_tensor([w, 0, w, 0])
                caption = _swap_left_right(caption)
            if random.random() < 0.5:
                oh, ow = self._resize(st, self.scales, self.max_size)
                stages.append(ResampleStage(oh, ow, 0, 0, oh, ow))
            else:
                h1, w1 = self._resize(st, self.resizes, None)
                region, tries = self._size_crop(st)
                wy, wx, wh, ww = region if region is not None else (0, 0, h1, w1)
                stages.append(ResampleStage(h1, w1, wy, wx, wh, ww))
                oh, ow = self._resize(st, self.scales, self.max_size)
                stages.append(ResampleStage(oh, ow, 0, 0, oh, ow))
        else:
            oh, ow = self._resize(st, self.test_size, self.max_size)
            stages.append(ResampleStage(oh, ow, 0, 0, oh, ow))
        H, W = st["h"], st["w"]
        b = st["boxes"]
        cxcywh = torch.stack([(b[:, 0] + b[:, 2]) / 2, (b[:, 1] + b[:, 3]) / 2, b[:, 2] - b[:, 0], b[:, 3] - b[:, 1]], dim=-1)
        cxcywh = cxcywh / torch.tensor([W, H, W, H], dtype=torch.float32)
        counts = torch.bincount(st["frame"], minlength=len(targets)).tolist()
        size, out = torch.tensor([H, W]), []
        for t, bx in zip(targets, torch.split(cxcywh, counts)):
            out.append({"boxes": bx, "size": size, "orig_size": torch.as_tensor(t["orig_size"]) if "orig_size" in t else torch.as_tensor([h, w])})
        return ClipPlan(flip, stages, (H, W), out, caption, tries, (h, w))


def make_video_transforms(image_set: str, cautious: bool, resolution: int = 224) -> VideoTransformPlanner:
    """The reference's signature and size table (datasets/video_transforms.py:327-443); the returned object plans the
    transform instead of running it on host pixels."""
    if resolution not in _TABLE:
        raise NotImplementedError
    if image_set not in ("train", "val", "test"):
        raise ValueError(f"unknown {image_set}")
    return VideoTransformPlanner(image_set, cautious, *_TABLE[resolution])


def resample_job(src: int, T: int, sh: int, sw: int, flip: bool, stage: ResampleStage, dst: int, planar: bool = False, frame_off: int = 0, H: int = 0, W: int = 0,
                 mask: Optional[int] = None, src_pitch: Optional[int] = None, src_frame_stride: Optional[int] = None):
    """One ``td_resample_job``: T packed rgb24 frames of sh x sw at device address ``src`` through ``stage`` into ``dst``
    (interleaved (T, wh, ww, 3), or planar frames frame_off.. of a padded (n, 3, H, W) video with its (n, H, W) mask)."""
    pitch = 3 * sw if src_pitch is None else src_pitch
    j = _hip.ResampleJob()
    j.src, j.src_frame_stride, j.src_pitch = src, (pitch * sh if src_frame_stride is None else src_frame_stride), pitch
    j.T, j.sh, j.sw, j.flip = T, sh, sw, int(bool(flip))
    j.rh, j.rw, j.wy, j.wx, j.wh, j.ww = stage.rh, stage.rw, stage.wy, stage.wx, stage.wh, stage.ww
    j.dst, j.planar, j.frame_off, j.H, j.W, j.mask = dst, int(bool(planar)), frame_off, H, W, mask
    return j


@dataclass
class DecodedClip:
    """T decoded frames of h x w as they came off the decoder's pipe: ``data`` is the flat uint8 buffer, tightly packed
    (ffmpeg ``-f rawvideo -pix_fmt <pix_fmt>``).  yuv420p: per frame the Y plane, then U, then V ((h + 1) // 2 rows of
    (w + 1) // 2 bytes each); nv12: the Y plane, then the interleaved UV plane; rgb24: (h, w, 3).  ``matrix`` and
    ``full_range`` say how yuv becomes rgb (include/tubedetr_hip.h; yuvj420p is yuv420p with ``full_range=True``)."""
    data: object
    T: int
    h: int
    w: int
    pix_fmt: str = "yuv420p"
    matrix: str = "bt601"
    full_range: bool = False

    def __post_init__(self):
        if self.pix_fmt not in _PIX_FMTS:
            raise ValueError(f"pix_fmt {self.pix_fmt!r}: one of {_PIX_FMTS}")
        if self.matrix not in _MATRICES:
            raise ValueError(f"matrix {self.matrix!r}: one of {_MATRICES}")
        self.T, self.h, self.w = int(self.T), int(self.h), int(self.w)
        d = torch.as_tensor(self.data)
        if d.dtype != torch.uint8 or d.is_cuda:
            raise ValueError("data is a uint8 buffer on the host")
        d = d.contiguous().view(-1)
        if d.numel() != self.T * self.nbytes_per_frame:
            raise ValueError(f"{d.numel()} bytes for {self.T} {self.pix_fmt} frames of {self.h} x {self.w} ({self.nbytes_per_frame} bytes each)")
        self.data = d

    @property
    def chroma_hw(self) -> Tuple[int, int]:
        return (self.h + 1) // 2, (self.w + 1) // 2

    @property
    def nbytes_per_frame(self) -> int:
        return _frame_bytes(self.pix_fmt, self.h, self.w)

    @property
    def nbytes(self) -> int:
        return self.T * self.nbytes_per_frame


def resample_src_job(src: int, T: int, sh: int, sw: int, flip: bool, stage: ResampleStage, dst: int, pix_fmt: str = "rgb24", matrix: str = "bt601",
                     full_range: bool = False, planar: bool = False, frame_off: int = 0, H: int = 0, W: int = 0, mask: Optional[int] = None,
                     planes: Optional[Sequence[int]] = None, pitches: Optional[Sequence[int]] = None, frame_stride: Optional[int] = None):
    """One ``td_resample_src_job``: ``resample_job`` for T frames in ``pix_fmt`` at device address ``src``.  Without
    ``planes`` / ``pitches`` / ``frame_stride`` the frames are tightly packed (``DecodedClip``); else ``planes`` are the
    device addresses of frame 0's planes (``src`` is ignored) and ``pitches`` their row pitches."""
    fmt, tight, sizes = _planes(pix_fmt, sh, sw)
    j = _hip.ResampleSrcJob()
    _put_planes(j, "", _describe(src, sizes, tight, planes, pitches, frame_stride))
    j.fmt, j.matrix, j.full_range = fmt, _MATRICES.index(matrix), int(bool(full_range))
    j.T, j.sh, j.sw, j.flip = T, sh, sw, int(bool(flip))
    j.rh, j.rw, j.wy, j.wx, j.wh, j.ww = stage.rh, stage.rw, stage.wy, stage.wx, stage.wh, stage.ww
    j.dst, j.planar, j.frame_off, j.H, j.W, j.mask = dst, int(bool(planar)), frame_off, H, W, mask
    return j
