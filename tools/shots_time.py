"""Time td_frame_stats + td_shot_cuts (tubedetr_amd.render.shot_cuts' two launches): 16 clips of 100 decoded frames of 1280 x 720,
yuv420p and rgb24, at step 1, 2 and 4.

Three candidates per format, alternating in ONE process for 3 rounds (the same frames, the same process, so that a drifting clock
or a neighbour on the host hits all of them):
  ``kernel``  td_frame_stats and td_shot_cuts for all clips, back to back on one stream: every pair timed by its own pair of
              device events after 3 warm-up pairs, the MEDIAN of >= 20 pairs per round.  ``read_bytes`` is what the rule has to
              read once - the sampled rows of the luma plane (rgb24: of the pixels) - computed from the shapes;
              ``read_GBps`` = read_bytes / median.
  ``copy``    a torch ``copy_`` of the same frames' bytes into a second buffer, timed the same way: the rate at which this
              device streams these bytes, reading AND writing them (``copy_GBps`` counts both).  It does not depend on step.
  ``torch``   the route a user had before: per frame a ``bincount`` of luma >> 2 and ``(a.int() - b.int()).abs().sum()`` (rgb24:
              the integer luma first; step > 1: a strided slice first), in a Python loop over all 1 600 frames; no host copy, so
              it is timed by the host clock around the whole loop with a synchronise at both ends, once per round after one
              warm-up.  Its integers ARE the rule's: clip 0's histograms and differences are compared for equality.
The engine clocks and the socket power are read (rocm-smi --showclocks / --showpower, read-only) before, between the formats and
after, and recorded.

  python tools/shots_time.py [--out profiles/shots_time.json] [--clips 16] [--frames 100] [--launches 25] [--rounds 3]
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

from tubedetr_amd import _hip  # noqa: E402
from tubedetr_amd.render import DeviceFrames, cuts_job, sampled_pixels, stats_job  # noqa: E402

H, W = 720, 1280
STEPS = (1, 2, 4)


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


def make_clips(fmt, n_clips, T, dev, g):
    """Clips with structure: a smooth picture that drifts, and a hard cut in the middle of every clip."""
    clips = []
    y, x = torch.meshgrid(torch.arange(H, device=dev), torch.arange(W, device=dev), indexing="ij")
    for c in range(n_clips):
        t = torch.arange(T, device=dev).view(T, 1, 1)
        scene = (t >= T // 2).to(torch.int64) * (60 + 5 * c)
        luma = ((x + 2 * y + 3 * t + 17 * c) % 160 + scene + torch.randint(0, 16, (T, H, W), device=dev, generator=g)).clamp_(0, 255).to(torch.uint8)
        if fmt == "rgb24":
            data = luma.unsqueeze(-1).expand(T, H, W, 3).contiguous()
        else:
            data = torch.cat([luma.view(T, -1), torch.full((T, H * W // 2), 128, dtype=torch.uint8, device=dev)], 1).contiguous()
        clips.append(DeviceFrames(data.view(-1), T, H, W, fmt))
    return clips


class Kernel:
    """The two launches for all clips, with one job-table pair per launch of a timing window."""

    def __init__(self, clips, step, ring, dev):
        self.lib, self.n = _hip.lib(), len(clips)
        T = clips[0].T
        self.out = [torch.empty(65 * T, dtype=torch.int32, device=dev) for _ in clips]
        self.cut = [(torch.empty(T, dtype=torch.uint8, device=dev), torch.empty(2 * T + 1, dtype=torch.int32, device=dev)) for _ in clips]
        n_px = sampled_pixels(H, W, step)
        sj = [stats_job(c.data.data_ptr(), T, H, W, c.pix_fmt, step, o.data_ptr(), o.data_ptr() + 256 * T) for c, o in zip(clips, self.out)]
        cj = [cuts_job(o.data_ptr(), o.data_ptr() + 256 * T, T, n_px, cut.data_ptr(), w.data_ptr() + 4 * T, w.data_ptr() + 8 * T, w.data_ptr()) for o, (cut, w) in zip(self.out, self.cut)]
        self.sarr, self.carr = (_hip.StatsJob * self.n)(*sj), (_hip.CutsJob * self.n)(*cj)
        self.nb = [int(self.lib.td_frame_stats_table_bytes(self.n)), int(self.lib.td_shot_cuts_table_bytes(self.n))]
        self.ring, self.slot = ring, 0
        self.tab_h = torch.empty(ring * sum(self.nb), dtype=torch.uint8, pin_memory=True)
        self.tab_d = torch.empty(ring * sum(self.nb), dtype=torch.uint8, device=dev)

    def __call__(self):
        o = (self.slot % self.ring) * sum(self.nb)
        self.slot += 1
        st = _hip.stream_ptr()
        _hip.check(self.lib.td_frame_stats(self.sarr, self.n, self.tab_h.data_ptr() + o, self.tab_d.data_ptr() + o, self.nb[0], st), "td_frame_stats")
        o += self.nb[0]
        _hip.check(self.lib.td_shot_cuts(self.carr, self.n, self.tab_h.data_ptr() + o, self.tab_d.data_ptr() + o, self.nb[1], st), "td_shot_cuts")


def torch_route(clips, step):
    """Per frame a bincount and a difference; returns per clip (hist (T, 64), sad (T,)) as int64 tensors on the device."""
    out = []
    for c in clips:
        T = c.T
        if c.pix_fmt == "rgb24":
            px = c.data.view(T, H, W, 3)[:, ::step, ::step].to(torch.int32)
            luma = (77 * px[..., 0] + 150 * px[..., 1] + 29 * px[..., 2] + 128) >> 8
        else:
            luma = c.data.view(T, -1)[:, : H * W].view(T, H, W)[:, ::step, ::step]
        hist, sad = [], [torch.zeros((), dtype=torch.int64, device=c.data.device)]
        for t in range(T):
            a = luma[t].reshape(-1)
            hist.append(torch.bincount((a >> 2).to(torch.int64), minlength=64))
            if t > 0:
                sad.append((a.int() - luma[t - 1].reshape(-1).int()).abs().sum())
        out.append((torch.stack(hist), torch.stack(sad)))
    return out


def host_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "shots_time.json"))
    ap.add_argument("--clips", type=int, default=16)
    ap.add_argument("--frames", type=int, default=100)
    ap.add_argument("--launches", type=int, default=25)
    ap.add_argument("--rounds", type=int, default=3)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/shots_time.py measures on the GPU; none is visible")
    if a.launches < 20:
        raise SystemExit("the median is taken over at least 20 launches")
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(0)
    samples, rows = [smi()], []
    for fmt in ("yuv420p", "rgb24"):
        clips = make_clips(fmt, a.clips, a.frames, dev, g)
        src = torch.cat([c.data for c in clips])
        dst = torch.empty_like(src)
        kernels = {s: Kernel(clips, s, a.launches + 3, dev) for s in STEPS}
        got = {s: {"kernel": [], "torch": []} for s in STEPS}
        copies = []
        torch_route(clips[:1], 1)  # warm-up of the operators
        for _ in range(a.rounds):
            for s in STEPS:
                got[s]["kernel"].append(median_ms(kernels[s], a.launches))
                copies.append(median_ms(lambda: dst.copy_(src), a.launches))
                got[s]["torch"].append(host_ms(lambda s=s: torch_route(clips, s)))
        copy_ms = float(np.median([m for m, _, _ in copies]))
        frame_bytes = src.numel() // (a.clips * a.frames)
        for s in STEPS:
            kernels[s]()
            ref = torch_route(clips[:1], s)[0]
            hist, sad = kernels[s].out[0][: 64 * a.frames].view(a.frames, 64), kernels[s].out[0][64 * a.frames:]
            cuts = torch.nonzero(kernels[s].cut[0][0]).view(-1).tolist()
            agrees = bool(torch.equal(hist.to(torch.int64), ref[0])) and bool(torch.equal(sad.to(torch.int64) & 0xFFFFFFFF, ref[1]))
            med = float(np.median([m for m, _, _ in got[s]["kernel"]]))
            tmed = float(np.median(got[s]["torch"]))
            read = a.clips * a.frames * ((H + s - 1) // s) * (3 * W if fmt == "rgb24" else W)
            r = {"pix_fmt": fmt, "step": s, "clips": a.clips, "frames_per_clip": a.frames, "size": [H, W], "launches_timed_per_round": a.launches, "rounds": a.rounds,
                 "kernel_ms_median_per_round": [round(m, 4) for m, _, _ in got[s]["kernel"]], "kernel_ms_min": round(min(lo for _, lo, _ in got[s]["kernel"]), 4),
                 "kernel_ms_max": round(max(hi for _, _, hi in got[s]["kernel"]), 4), "kernel_ms_median": round(med, 4), "read_bytes": int(read),
                 "read_GBps": round(read / (med * 1e-3) / 1e9, 1), "copy_ms_median": round(copy_ms, 4), "copy_bytes_read_and_written": int(2 * src.numel()),
                 "copy_GBps": round(2 * src.numel() / (copy_ms * 1e-3) / 1e9, 1), "frame_bytes": int(frame_bytes), "kernel_over_copy": round(med / copy_ms, 3),
                 "torch_ms_per_round": [round(m, 2) for m in got[s]["torch"]], "torch_ms_median": round(tmed, 2), "torch_over_kernel": round(tmed / med, 1),
                 "agrees_with_torch_route": agrees, "cuts_of_clip_0": cuts}
            rows.append(r)
            print(f"{fmt:8s} step {s}  kernel {med:8.4f} ms  read {r['read_GBps']:7.1f} GB/s   copy {copy_ms:8.4f} ms ({r['copy_GBps']:7.1f} GB/s r+w)   torch route {tmed:9.2f} ms  x{r['torch_over_kernel']}"
                  f"   agrees {agrees}   cuts {cuts}", flush=True)
        del clips, src, dst, kernels
        torch.cuda.empty_cache()
        samples.append(smi())
    out = {"device": torch.cuda.get_device_name(0), "smi_samples_before_between_after": samples,
           "method": "kernel and copy: device events around every single launch (pair), 3 warm-up launches, median of `launches_timed_per_round`; the torch route: host clock around "
                     "the whole loop over all frames, a synchronise at both ends; the three alternate for `rounds` rounds in one process and the medians over the rounds are reported",
           "cases": rows}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
