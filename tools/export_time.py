"""Time td_frame_export (tubedetr_amd.render.export's launch): 16 clips of 100 decoded frames of 1280 x 720.

Cases: rgb24 -> yuv420p at the same size; rgb24 -> yuv420p at 360p; yuv420p -> nv12 at the same size; yuv420p -> rgb24 at 360p;
rgb24 -> yuv420p at 360p taking every second frame.  Three candidates per case, alternating in ONE process for 3 rounds (the same
frames, the same process, so that a drifting clock or a neighbour on the host hits all of them):
  ``kernel``  one td_frame_export launch for all clips: every launch timed by its own pair of device events after 3 warm-up
              launches, the MEDIAN of >= 20 launches per round.  ``read_bytes`` / ``written_bytes`` are what the rule has to read
              and write once, computed from the shapes;
  ``copy``    a torch ``copy_`` of the SOURCE frames' bytes into a second buffer, timed the same way: the floor for reading the
              frames at all (it also writes as many bytes, which an export to a smaller format does not);
  ``torch``   the route a user had before: per clip ``F.interpolate(mode="area")`` on float frames plus a matmul with the colour
              matrix, rounded and clamped (rgb24 -> yuv420p: luma from the resized picture, chroma from its 2 x 2 means; yuv420p
              -> rgb24: chroma replicated first; yuv420p -> nv12: a stack of the two chroma planes).  Float arithmetic: close to the
              rule, not equal to it, so only its time is recorded.  Timed by the host clock around the loop over the clips with a
              synchronise at both ends, once per round after one warm-up.
Beside them the device-to-host copy of one exported clip and of its source clip into page-locked memory (device events, median).
The engine clocks and the socket power are read (rocm-smi --showclocks / --showpower, read-only) before, between the cases and
after, and recorded.

  python tools/export_time.py [--out profiles/export_time.json] [--clips 16] [--frames 100] [--launches 20] [--rounds 3]
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from tubedetr_amd import _hip  # noqa: E402
from tubedetr_amd.render import DeviceFrames, _forward_coefficients, _frame_bytes, export_job  # noqa: E402

H, W = 720, 1280
CASES = [("rgb24", "yuv420p", (720, 1280), 1), ("rgb24", "yuv420p", (360, 640), 1), ("yuv420p", "nv12", (720, 1280), 1), ("yuv420p", "rgb24", (360, 640), 1),
         ("rgb24", "yuv420p", (360, 640), 2)]  # source, destination, picture, every n-th frame


def smi():
    out = {}
    for key, flag, words in (("clocks", "--showclocks", ("sclk", "mclk", "fclk")), ("power", "--showpower", ("Power", "power"))):
        try:
            txt = subprocess.run(["rocm-smi", flag, "-d", "0"], capture_output=True, text=True, timeout=30).stdout
            out[key] = [" ".join(l.split()) for l in txt.splitlines() if any(w in l for w in words)] or "not available"
        except Exception as e:  # noqa: BLE001
            out[key] = f"not available ({type(e).__name__})"
    return out


def median_ms(fn, launches, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(launches)]
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    ms = sorted(a.elapsed_time(b) for a, b in ev)
    return float(np.median(ms)), ms[0], ms[-1]


def host_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0)


def make_clips(fmt, n_clips, T, dev, g):
    return [DeviceFrames(torch.randint(0, 256, (T * _frame_bytes(fmt, H, W),), dtype=torch.uint8, device=dev, generator=g), T, H, W, fmt) for _ in range(n_clips)]


class Kernel:
    """One launch for all clips, with one job-table pair per launch of a timing window."""

    def __init__(self, clips, dst_fmt, size, every, ring, dev):
        self.lib, self.n = _hip.lib(), len(clips)
        T = clips[0].T
        self.To = len(range(0, T, every))
        self.take = torch.arange(0, T, every, dtype=torch.int32, device=dev) if every > 1 else None
        self.out = [torch.empty(self.To * _frame_bytes(dst_fmt, *size), dtype=torch.uint8, device=dev) for _ in clips]
        jobs = [export_job(c.data.data_ptr(), T, H, W, o.data_ptr(), c.pix_fmt, dst_fmt, size, take=_hip.ptr(self.take), To=self.To) for c, o in zip(clips, self.out)]
        self.arr = (_hip.ExportJob * self.n)(*jobs)
        self.nb = int(self.lib.td_frame_export_table_bytes(self.n))
        self.ring, self.slot = ring, 0
        self.tab_h = torch.empty(ring * self.nb, dtype=torch.uint8, pin_memory=True)
        self.tab_d = torch.empty(ring * self.nb, dtype=torch.uint8, device=dev)

    def __call__(self):
        o = (self.slot % self.ring) * self.nb
        self.slot += 1
        _hip.check(self.lib.td_frame_export(self.arr, self.n, self.tab_h.data_ptr() + o, self.tab_d.data_ptr() + o, self.nb, _hip.stream_ptr()), "td_frame_export")


def torch_route(clips, dst_fmt, size, every):
    """The operators a user would reach for; returns the exported clips (uint8, the destination's tight layout)."""
    rows, offs = _forward_coefficients("bt601", False)
    dev = clips[0].data.device
    fwd, off = torch.tensor(rows, device=dev), torch.tensor(offs, dtype=torch.float32, device=dev)
    inv = torch.linalg.inv(fwd.double()).float()
    oh, ow = size
    out = []
    for c in clips:
        T = c.T
        if c.pix_fmt == "rgb24":
            x = c.data.view(T, H, W, 3)[::every].permute(0, 3, 1, 2).float()
            if size != (H, W):
                x = F.interpolate(x, size=size, mode="area").round_()
            y = (torch.einsum("kc,tchw->tkhw", fwd[:1], x) + off[0]).round_().clamp_(0, 255).to(torch.uint8)
            uv = (torch.einsum("kc,tchw->tkhw", fwd[1:], F.avg_pool2d(x, 2)) + 128.0).round_().clamp_(0, 255).to(torch.uint8)
            out.append(torch.cat([y.reshape(len(x), -1), uv.reshape(len(x), -1)], 1).view(-1))
        else:
            frames = c.data.view(T, -1)[::every]
            y = frames[:, :H * W].view(-1, 1, H, W)
            uv = frames[:, H * W:].view(-1, 2, H // 2, W // 2)
            if dst_fmt == "nv12":
                out.append(torch.cat([y.reshape(len(y), -1), uv.permute(0, 2, 3, 1).reshape(len(y), -1)], 1).view(-1))
            else:
                yuv = torch.cat([y.float() - off[0], uv.float().repeat_interleave(2, 2).repeat_interleave(2, 3) - 128.0], 1)
                rgb = torch.einsum("kc,tchw->tkhw", inv, yuv).round_().clamp_(0, 255)
                rgb = F.interpolate(rgb, size=size, mode="area").round_().clamp_(0, 255).to(torch.uint8)
                out.append(rgb.permute(0, 2, 3, 1).reshape(-1))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "export_time.json"))
    ap.add_argument("--clips", type=int, default=16)
    ap.add_argument("--frames", type=int, default=100)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/export_time.py measures on the GPU; none is visible")
    if a.launches < 20:
        raise SystemExit("the median is taken over at least 20 launches")
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(0)
    samples, rows = [smi()], []
    for src_fmt in ("rgb24", "yuv420p"):
        clips = make_clips(src_fmt, a.clips, a.frames, dev, g)
        src = torch.cat([c.data for c in clips])
        dst = torch.empty_like(src)
        cases = [c for c in CASES if c[0] == src_fmt]
        kernels = [Kernel(clips, df, size, every, a.launches + 3, dev) for _, df, size, every in cases]
        got = [{"kernel": [], "torch": []} for _ in cases]
        copies = []
        for (_, df, size, every) in cases:  # warm-up of the operators
            torch_route(clips[:1], df, size, every)
        for _ in range(a.rounds):
            for i, (_, df, size, every) in enumerate(cases):
                got[i]["kernel"].append(median_ms(kernels[i], a.launches))
                copies.append(median_ms(lambda: dst.copy_(src), a.launches))
                got[i]["torch"].append(host_ms(lambda: torch_route(clips, df, size, every)))
        copy_ms = float(np.median([m for m, _, _ in copies]))
        host_src = torch.empty(clips[0].data.numel(), dtype=torch.uint8, pin_memory=True)
        d2h_src = median_ms(lambda: host_src.copy_(clips[0].data, non_blocking=True), a.launches)[0]
        for i, (_, df, size, every) in enumerate(cases):
            k = kernels[i]
            host_out = torch.empty(k.out[0].numel(), dtype=torch.uint8, pin_memory=True)
            d2h_out = median_ms(lambda: host_out.copy_(k.out[0], non_blocking=True), a.launches)[0]
            med = float(np.median([m for m, _, _ in got[i]["kernel"]]))
            tmed = float(np.median(got[i]["torch"]))
            read = a.clips * k.To * _frame_bytes(src_fmt, H, W)
            written = a.clips * k.To * _frame_bytes(df, *size)
            r = {"src_fmt": src_fmt, "dst_fmt": df, "src_size": [H, W], "size": list(size), "take_every": every, "clips": a.clips, "frames_per_clip": a.frames,
                 "frames_out_per_clip": k.To, "launches_timed_per_round": a.launches, "rounds": a.rounds,
                 "kernel_ms_median_per_round": [round(m, 4) for m, _, _ in got[i]["kernel"]], "kernel_ms_min": round(min(lo for _, lo, _ in got[i]["kernel"]), 4),
                 "kernel_ms_max": round(max(hi for _, _, hi in got[i]["kernel"]), 4), "kernel_ms_median": round(med, 4), "read_bytes": int(read), "written_bytes": int(written),
                 "read_plus_written_GBps": round((read + written) / (med * 1e-3) / 1e9, 1), "copy_of_all_source_frames_ms_median": round(copy_ms, 4),
                 "copy_bytes_read_and_written": int(2 * src.numel()), "copy_GBps": round(2 * src.numel() / (copy_ms * 1e-3) / 1e9, 1), "kernel_over_copy": round(med / copy_ms, 3),
                 "torch_ms_per_round": [round(m, 2) for m in got[i]["torch"]], "torch_ms_median": round(tmed, 2), "torch_over_kernel": round(tmed / med, 1),
                 "d2h_one_source_clip_ms": round(d2h_src, 4), "d2h_one_source_clip_bytes": int(host_src.numel()), "d2h_one_exported_clip_ms": round(d2h_out, 4),
                 "d2h_one_exported_clip_bytes": int(host_out.numel())}
            rows.append(r)
            print(f"{src_fmt:8s} -> {df:8s} {size[0]:4d} x {size[1]:4d} every {every}  kernel {med:8.4f} ms ({r['read_plus_written_GBps']:7.1f} GB/s r+w)   copy {copy_ms:8.4f} ms "
                  f"({r['copy_GBps']:7.1f} GB/s r+w)  x{r['kernel_over_copy']}   torch route {tmed:9.2f} ms  x{r['torch_over_kernel']}   d2h {d2h_src:.3f} -> {d2h_out:.3f} ms", flush=True)
        del clips, src, dst, kernels
        torch.cuda.empty_cache()
        samples.append(smi())
    out = {"device": torch.cuda.get_device_name(0), "smi_samples_before_between_after": samples,
           "method": "kernel, copy and the device-to-host copies: device events around every single launch, 3 warm-up launches, median of `launches_timed_per_round`; the torch "
                     "route: host clock around the loop over the clips, a synchronise at both ends; the three alternate for `rounds` rounds in one process and the medians over "
                     "the rounds are reported",
           "cases": rows}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
