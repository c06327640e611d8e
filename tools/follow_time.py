"""Time td_tube_follow (tubedetr_amd.render.follow's one launch): 16 clips of 100 decoded frames of 1280 x 720, every sixth frame an
anchor, boxes of 200 x 300 pixels that move with the picture; yuv420p and rgb24, K = 1 and 4 tubes, radius 4, 8 and 16.

Candidates per format, alternating in ONE process for 3 rounds (the same frames, the same process, so that a drifting clock or a
neighbour on the host hits all of them):
  ``kernel``  td_tube_follow for all clips, one launch: every launch timed by its own pair of device events after 3 warm-up
              launches, the MEDIAN of >= 20 launches per round.  Beside the time: ``fetched_bytes``, the bytes that the matching
              units' loads ask for (the template's 256 samples and, per grid row, 16 neighbourhoods of (2 R + 1) rows of
              4 ceil((2 R + 1) / 4) pixels; rgb24: 3 bytes per pixel) - the neighbourhoods of neighbouring samples overlap, so the
              caches serve most of them -, and ``candidate_samples_per_s`` = matching units x (2 R + 1)^2 x 256 / median.
  ``copy``    a torch ``copy_`` of the same frames' bytes into a second buffer, timed the same way: the rate at which this
              device streams the clips, reading AND writing them (``copy_GBps`` counts both).
  ``torch``   for ONE configuration (yuv420p, K = 1, radius 4) the route a user had before: per clip, the 256 samples of every
              candidate of every frame gathered with tensor indexing, the sums, the tie order as one integer key and argmin; no host
              copy, timed by the host clock around all clips with a synchronise at both ends, once per round after one warm-up.
              Its offsets are compared with the kernel's for equality (``agrees_with_torch_route``).
The engine clocks and the socket power are read (rocm-smi --showclocks / --showpower, read-only) before, between the formats and
after, and recorded.

  python tools/follow_time.py [--out profiles/follow_time.json] [--clips 16] [--frames 100] [--launches 25] [--rounds 3]
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
from tubedetr_amd.render import DeviceFrames, anchors, follow_job  # noqa: E402

H, W = 720, 1280
BOX_W, BOX_H = 200, 300
ANCHOR_STEP, REACH, ACCEPT = 6, 3, (24, 1)
KS, RADII = (1, 4), (4, 8, 16)
TORCH_CASE = ("yuv420p", 1, 4)


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
    """A blocky texture that drifts by (2, 3) pixels per frame, with a little noise: a match has a definite place."""
    clips = []
    y, x = torch.meshgrid(torch.arange(H, device=dev), torch.arange(W, device=dev), indexing="ij")
    for c in range(n_clips):
        t = torch.arange(T, device=dev).view(T, 1, 1)
        luma = ((((x + 3 * t + 11 * c) >> 2) * 37 + ((y + 2 * t) >> 2) * 91) % 200 + torch.randint(0, 8, (T, H, W), device=dev, generator=g)).to(torch.uint8)
        if fmt == "rgb24":
            data = luma.unsqueeze(-1).expand(T, H, W, 3).contiguous()
        else:
            data = torch.cat([luma.view(T, -1), torch.full((T, H * W // 2), 128, dtype=torch.uint8, device=dev)], 1).contiguous()
        clips.append(DeviceFrames(data.view(-1), T, H, W, fmt))
    return clips


def make_boxes(n_clips, T, K, dev):
    """Tube k of clip c: a 200 x 300 box on a straight line that lags the picture's drift by a pixel or two between the anchors."""
    t = torch.arange(T, device=dev, dtype=torch.float32).view(T, 1)
    k = torch.arange(K, device=dev, dtype=torch.float32).view(1, K)
    out = []
    for c in range(n_clips):
        lag = ((t % ANCHOR_STEP) > 0).float() * (1 + (t % 2))
        x0, y0 = 700 - 3 * t + 90 * k + 7 * c + lag, 330 - 2 * t + 20 * k - lag
        out.append(torch.stack([x0, y0, x0 + BOX_W, y0 + BOX_H], -1).contiguous())
    return out


class Kernel:
    """The launch for all clips, with one job-table pair per launch of a timing window."""

    def __init__(self, clips, boxes, anchor, K, radius, ring, dev):
        self.lib, self.n = _hip.lib(), len(clips)
        T = clips[0].T
        self.out = [torch.empty_like(b) for b in boxes]
        self.words = [torch.empty(3 * T * K, dtype=torch.int32, device=dev) for _ in clips]
        self.status = [torch.empty(T * K, dtype=torch.uint8, device=dev) for _ in clips]
        jobs = [follow_job(c.data.data_ptr(), T, H, W, b.data_ptr(), anchor.data_ptr(), o.data_ptr(), K, c.pix_fmt, None, radius, REACH, ACCEPT, w.data_ptr(),
                           w.data_ptr() + 8 * T * K, s.data_ptr()) for c, b, o, w, s in zip(clips, boxes, self.out, self.words, self.status)]
        self.keep = (boxes, anchor)
        self.arr = (_hip.FollowJob * self.n)(*jobs)
        self.nb = int(self.lib.td_tube_follow_table_bytes(self.n))
        self.ring, self.slot, self.T, self.K = ring, 0, T, K
        self.tab_h = torch.empty(ring * self.nb, dtype=torch.uint8, pin_memory=True)
        self.tab_d = torch.empty(ring * self.nb, dtype=torch.uint8, device=dev)

    def __call__(self):
        o = (self.slot % self.ring) * self.nb
        self.slot += 1
        _hip.check(self.lib.td_tube_follow(self.arr, self.n, self.tab_h.data_ptr() + o, self.tab_d.data_ptr() + o, self.nb, _hip.stream_ptr()), "td_tube_follow")

    def offsets(self, i):
        return self.words[i][:2 * self.T * self.K].view(self.T, self.K, 2)


def torch_route(clips, boxes, anchor, radius):
    """Per clip (yuv420p, K = 1): the offsets (T, 2) as int64 on the device, by tensor indexing."""
    out = []
    R, S = radius, 2 * radius + 1
    j = torch.arange(16, device=anchor.device)
    d = torch.arange(-R, R + 1, device=anchor.device)
    dy, dx = d.view(S, 1).expand(S, S).reshape(-1), d.view(1, S).expand(S, S).reshape(-1)
    tie = ((dy * dy + dx * dx) << 12) + ((dy + R) << 6) + (dx + R)
    for c, b in zip(clips, boxes):
        T = c.T
        luma = c.data.view(T, -1)[:, :H * W].view(T, H, W)
        t = torch.arange(T, device=b.device)
        m = t % ANCHOR_STEP
        g = torch.where(m <= ANCHOR_STEP // 2, t - m, t + ANCHOR_STEP - m)  # the nearer anchor, of two equally near the earlier: all exist for T = 6 n + 4
        between = (m != 0) & (g < T)
        t, g = t[between], g[between]
        r = torch.floor(b[:, 0].clamp(-1048576.0, 1048576.0) + 0.5).long()
        a, q = r[g], r[t]
        x0, y0, x1, y1 = a[:, 0].clamp(min=0), a[:, 1].clamp(min=0), a[:, 2].clamp(max=W), a[:, 3].clamp(max=H)
        px = x0.view(-1, 1) + ((2 * j + 1).view(1, -1) * (x1 - x0).view(-1, 1)) // 32
        py = y0.view(-1, 1) + ((2 * j + 1).view(1, -1) * (y1 - y0).view(-1, 1)) // 32
        tem = luma[g.view(-1, 1, 1), py.view(-1, 16, 1), px.view(-1, 1, 16)].int()
        ddx, ddy = ((q[:, 0] + q[:, 2]) - (a[:, 0] + a[:, 2])) >> 1, ((q[:, 1] + q[:, 3]) - (a[:, 1] + a[:, 3])) >> 1
        yy = (py.view(-1, 1, 16, 1) + (ddy.view(-1, 1) + dy.view(1, -1)).view(-1, S * S, 1, 1)).clamp(0, H - 1)
        xx = (px.view(-1, 1, 1, 16) + (ddx.view(-1, 1) + dx.view(1, -1)).view(-1, S * S, 1, 1)).clamp(0, W - 1)
        cost = (luma[t.view(-1, 1, 1, 1), yy, xx].int() - tem.view(-1, 1, 16, 16)).abs().sum((2, 3)).long()
        best = ((cost << 22) + tie.view(1, -1)).argmin(1)
        ok = cost.gather(1, best.view(-1, 1)).view(-1) * ACCEPT[1] <= ACCEPT[0] * 256
        off = torch.zeros((T, 2), dtype=torch.int64, device=b.device)
        off[t] = torch.stack([dy[best], dx[best]], 1) * ok.view(-1, 1)
        out.append(off)
    return out


def host_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "follow_time.json"))
    ap.add_argument("--clips", type=int, default=16)
    ap.add_argument("--frames", type=int, default=100)
    ap.add_argument("--launches", type=int, default=25)
    ap.add_argument("--rounds", type=int, default=3)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/follow_time.py measures on the GPU; none is visible")
    if a.launches < 20:
        raise SystemExit("the median is taken over at least 20 launches")
    if a.frames % ANCHOR_STEP != 4:
        raise SystemExit(f"the torch route takes a frame count of {ANCHOR_STEP} n + 4: every frame then has an anchor within reach")
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(0)
    anchor = anchors(first=0, step=ANCHOR_STEP, T=a.frames, device=dev)
    samples, rows = [smi()], []
    for fmt in ("yuv420p", "rgb24"):
        clips = make_clips(fmt, a.clips, a.frames, dev, g)
        src = torch.cat([c.data for c in clips])
        dst = torch.empty_like(src)
        boxes = {K: make_boxes(a.clips, a.frames, K, dev) for K in KS}
        cases = [(K, R) for K in KS for R in RADII]
        kernels = {kr: Kernel(clips, boxes[kr[0]], anchor, kr[0], kr[1], a.launches + 3, dev) for kr in cases}
        got = {kr: [] for kr in cases}
        copies, torch_ms = [], []
        with_torch = fmt == TORCH_CASE[0]
        if with_torch:
            torch_route(clips[:1], boxes[1][:1], anchor, TORCH_CASE[2])  # warm-up of the operators
        for _ in range(a.rounds):
            for kr in cases:
                got[kr].append(median_ms(kernels[kr], a.launches))
                copies.append(median_ms(lambda: dst.copy_(src), a.launches))
                if with_torch and kr == TORCH_CASE[1:]:
                    torch_ms.append(host_ms(lambda: torch_route(clips, boxes[1], anchor, TORCH_CASE[2])))
        copy_ms = float(np.median([m for m, _, _ in copies]))
        for K, R in cases:
            kern = kernels[(K, R)]
            kern()
            torch.cuda.synchronize()
            status = torch.stack(kern.status)
            matched, accepted = int((status != 0).sum()), int((status == 1).sum())
            moved = int(sum((kern.offsets(i) != 0).any(-1).sum() for i in range(a.clips)))
            med = float(np.median([m for m, _, _ in got[(K, R)]]))
            S = 2 * R + 1
            fetched = matched * (256 + 16 * 16 * S * 4 * ((S + 3) // 4)) * (3 if fmt == "rgb24" else 1)
            r = {"pix_fmt": fmt, "K": K, "radius": R, "reach": REACH, "accept": list(ACCEPT), "clips": a.clips, "frames_per_clip": a.frames, "size": [H, W], "box": [BOX_W, BOX_H],
                 "anchor_every": ANCHOR_STEP, "launches_timed_per_round": a.launches, "rounds": a.rounds, "units": a.clips * a.frames * K, "matching_units": matched,
                 "accepted_units": accepted, "moved_units": moved, "kernel_ms_median_per_round": [round(m, 4) for m, _, _ in got[(K, R)]],
                 "kernel_ms_min": round(min(lo for _, lo, _ in got[(K, R)]), 4), "kernel_ms_max": round(max(hi for _, _, hi in got[(K, R)]), 4), "kernel_ms_median": round(med, 4),
                 "fetched_bytes": int(fetched), "fetched_GBps": round(fetched / (med * 1e-3) / 1e9, 1), "candidate_samples_per_s": float(f"{matched * S * S * 256 / (med * 1e-3):.4g}"),
                 "copy_ms_median": round(copy_ms, 4), "copy_bytes_read_and_written": int(2 * src.numel()), "copy_GBps": round(2 * src.numel() / (copy_ms * 1e-3) / 1e9, 1),
                 "kernel_over_copy": round(med / copy_ms, 4)}
            if with_torch and (K, R) == TORCH_CASE[1:]:
                ref = torch_route(clips, boxes[1], anchor, R)
                tmed = float(np.median(torch_ms))
                r.update({"torch_ms_per_round": [round(m, 2) for m in torch_ms], "torch_ms_median": round(tmed, 2), "torch_over_kernel": round(tmed / med, 1),
                          "agrees_with_torch_route": all(bool(torch.equal(kern.offsets(i)[:, 0].long(), ref[i])) for i in range(a.clips))})
            rows.append(r)
            print(f"{fmt:8s} K {K} radius {R:2d}  kernel {med:8.4f} ms  {r['candidate_samples_per_s']:.3g} candidate samples/s  fetched {r['fetched_GBps']:8.1f} GB/s   copy {copy_ms:8.4f} ms "
                  f"({r['copy_GBps']:7.1f} GB/s r+w)   matching {matched} accepted {accepted} moved {moved}"
                  + (f"   torch route {r['torch_ms_median']:9.2f} ms  x{r['torch_over_kernel']}  agrees {r['agrees_with_torch_route']}" if "torch_ms_median" in r else ""), flush=True)
        del clips, src, dst, kernels, boxes
        torch.cuda.empty_cache()
        samples.append(smi())
    out = {"device": torch.cuda.get_device_name(0), "smi_samples_before_between_after": samples,
           "method": "kernel and copy: device events around every single launch, 3 warm-up launches, median of `launches_timed_per_round`; the torch route: host clock around all "
                     "clips, a synchronise at both ends; the candidates alternate for `rounds` rounds in one process and the medians over the rounds are reported",
           "cases": rows}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
