"""Decoded frames on the device (``DeviceFrames``) and an RGB colour in their colour space (``color_in_space``)."""
from __future__ import annotations

from dataclasses import dataclass
from typing import Tuple

import torch

from ..augment import DecodedClip
from ..frame_jobs import _MATRICES, _PIX_FMTS, _check_geometry, _frame_bytes, _rgb3

_ONE = 1 << 20  # fixed-point one of color_in_space


def _forward_coefficients(matrix: str, full_range: bool):
    kr, kb = (0.299, 0.114) if matrix == "bt601" else (0.2126, 0.0722)
    kg = 1.0 - kr - kb
    sy, sc = (1.0, 1.0) if full_range else (219.0 / 255.0, 224.0 / 255.0)
    rows = ((kr * sy, kg * sy, kb * sy),
            (-kr / (2 * (1 - kb)) * sc, -kg / (2 * (1 - kb)) * sc, 0.5 * sc),
            (0.5 * sc, -kg / (2 * (1 - kr)) * sc, -kb / (2 * (1 - kr)) * sc))
    return rows, (0 if full_range else 16, 128, 128)


def color_in_space(rgb, pix_fmt: str = "rgb24", matrix: str = "bt601", full_range: bool = False) -> Tuple[int, int, int]:
    """The three bytes a job needs for the RGB colour ``rgb``: itself for rgb24; (Y, U, V) for yuv420p / nv12, by the exact
    integer forward of the header's conversion: component = clamp((c_r R + c_g G + c_b B + 2^20 offset + 2^19) >> 20) with
    round(2^20 x) coefficients of the textbook matrix (include/tubedetr_hip.h lists them by Kr, Kb and the range).  Within
    0.5004 of a level of the float64 formula for every (R, G, B).  20 fraction bits, not the 16 of the device's yuv -> rgb
    rule: the three limited-range U coefficients all round the same way at 16 bits, which puts bright colours 0.5036 off."""
    r, g, b = _rgb3("rgb", rgb)
    if pix_fmt not in _PIX_FMTS:
        raise ValueError(f"pix_fmt {pix_fmt!r}: one of {_PIX_FMTS}")
    if pix_fmt == "rgb24":
        return r, g, b
    if matrix not in _MATRICES:
        raise ValueError(f"matrix {matrix!r}: one of {_MATRICES}")
    rows, offs = _forward_coefficients(matrix, bool(full_range))
    out = []
    for (cr, cg, cb), off in zip(rows, offs):
        acc = round(_ONE * cr) * r + round(_ONE * cg) * g + round(_ONE * cb) * b + _ONE * off + _ONE // 2
        out.append(min(max(acc >> 20, 0), 255))
    return tuple(out)


@dataclass
class DeviceFrames:
    """T decoded frames of h x w ON THE DEVICE, laid out as ``DecodedClip`` lays them out on the host: ``data`` is the flat
    uint8 tensor, tightly packed, frame after frame (yuv420p: Y, U, V; nv12: Y, UV; rgb24: (h, w, 3))."""
    data: torch.Tensor
    T: int
    h: int
    w: int
    pix_fmt: str = "yuv420p"
    matrix: str = "bt601"
    full_range: bool = False

    def __post_init__(self):
        self.T, self.h, self.w = int(self.T), int(self.h), int(self.w)
        _check_geometry(self.pix_fmt, self.T, self.h, self.w)
        if self.matrix not in _MATRICES:
            raise ValueError(f"matrix {self.matrix!r}: one of {_MATRICES}")
        d = self.data
        if not torch.is_tensor(d) or d.dtype != torch.uint8 or not d.is_cuda or not d.is_contiguous():
            raise ValueError("data is a contiguous uint8 tensor on the device")
        if d.numel() != self.T * self.nbytes_per_frame:
            raise ValueError(f"{d.numel()} bytes for {self.T} {self.pix_fmt} frames of {self.h} x {self.w} ({self.nbytes_per_frame} bytes each)")
        self.data = d.view(-1)

    @property
    def nbytes_per_frame(self) -> int:
        return _frame_bytes(self.pix_fmt, self.h, self.w)

    @classmethod
    def from_decoded(cls, clip: DecodedClip, device) -> "DeviceFrames":
        """One upload of a ``DecodedClip`` through page-locked memory (asynchronous on the current stream)."""
        host = clip.data if clip.data.is_pinned() else clip.data.pin_memory()
        return cls(host.to(device, non_blocking=True), clip.T, clip.h, clip.w, clip.pix_fmt, clip.matrix, clip.full_range)

    def to_decoded(self) -> DecodedClip:
        """The inverse of ``from_decoded``: one download into page-locked memory, asynchronous on the current stream - the
        ``DecodedClip``'s bytes are there once the stream has passed the copy (``torch.cuda.current_stream().synchronize()``)."""
        host = torch.empty(self.data.numel(), dtype=torch.uint8, pin_memory=True)
        host.copy_(self.data, non_blocking=True)
        return DecodedClip(host, self.T, self.h, self.w, self.pix_fmt, self.matrix, self.full_range)

    def empty_like(self) -> "DeviceFrames":
        return DeviceFrames(torch.empty_like(self.data), self.T, self.h, self.w, self.pix_fmt, self.matrix, self.full_range)
