"""Time td_tube_redact (tubedetr_amd.render.redact's launch): 16 clips of 100 decoded frames of 1280 x 720 redacted along a tube
predicted at 5 fps (20 tube rows per clip, frame_map t // 5).

Cases: yuv420p and rgb24; fill, mosaic with cell 16, blur with radius 8 and with radius 64; a box of about 1/16 of the frame
(320 x 180 at a random place per tube row) and a box covering the frame; out of place, and in place where that is legal (not
blur); one inverted case per format.  Per case: every launch timed by its own pair of device events after 3 warm-up launches,
the MEDIAN of >= 20 launches, as tools/overlay_time.py does.

Two baselines beside each case, in the same process, right after it:
  ``copy_*``   a torch ``copy_`` of the frames' bytes (every byte read once and written once), timed the same way.
               ``time_over_copy`` = case / copy; for an out-of-place case, which moves the same bytes, its inverse is the
               fraction of the copy's bandwidth that the case reaches (``fraction_of_copy_bandwidth``).
  ``torch_*``  the route a user had before: ``boxes.cpu()``, a host loop over the frames, and per frame and plane a slice,
               ``avg_pool2d`` (+ ``interpolate`` for the mosaic) and an assignment - in place.  It synchronises and is thousands
               of launches, so it is timed by the host clock around ONE clip (a synchronise at both ends, 1 warm-up + 2 runs, the
               faster) and scaled to the batch: ``torch_ms_scaled``.  Its pixels are float means, not the rule's integers: it is
               a cost yardstick, not a reference.
The engine clocks and the socket power are read (rocm-smi --showclocks / --showpower, read-only) before, between the formats
and after, and recorded.

  python tools/redact_time.py [--out profiles/redact_time.json] [--clips 16] [--frames 100] [--launches 25]
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
from tubedetr_amd.render import DeviceFrames, color_in_space, redact_job  # noqa: E402

H, W, FPS_RATIO = 720, 1280, 5
MODES = [("fill", {}), ("mosaic", {"cell": 16}), ("blur", {"radius": 8}), ("blur", {"radius": 64})]


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


def make_boxes(n_tube, box, dev, g):
    if box == "frame":
        return torch.tensor([[0.0, 0.0, float(W), float(H)]], device=dev).repeat(n_tube, 1).contiguous()
    x0, y0 = torch.rand(n_tube, 1, device=dev, generator=g) * (W * 0.75), torch.rand(n_tube, 1, device=dev, generator=g) * (H * 0.75)
    return torch.cat([x0, y0, x0 + W * 0.25, y0 + H * 0.25], 1).contiguous()  # 1/16 of the frame


def torch_route(clip, boxes, fmap, mode, what, invert):
    """The route without td_tube_redact, on one clip, in place: returns the host-clock milliseconds of the faster of two runs."""
    T, fmt = clip.T, clip.pix_fmt
    ch, cw = (H + 1) // 2, (W + 1) // 2
    frames = clip.data.view(T, -1)
    if fmt == "rgb24":
        planes = [(frames.view(T, H, W, 3).permute(0, 3, 1, 2), 1, what.get("cell", 0), what.get("radius", 0))]  # a strided view: slices assign through it
    else:
        planes = [(frames[:, : H * W].view(T, 1, H, W), 1, what.get("cell", 0), what.get("radius", 0)),
                  (frames[:, H * W :].view(T, 2, ch, cw), 2, what.get("cell", 0) // 2, (what.get("radius", 0) + 1) // 2)]

    def once():
        host = boxes.cpu()  # the synchronisation
        rows = fmap.cpu().tolist()
        for t in range(T):
            bx = host[rows[t]]
            x0, y0, x1, y1 = (int(v + 0.5) for v in bx.tolist())
            x0, y0, x1, y1 = max(x0, 0) & ~1, max(y0, 0) & ~1, min(x1 + (x1 & 1), W), min(y1 + (y1 & 1), H)
            for p, s, cp, rp in planes:
                px0, py0, px1, py1 = x0 // s, y0 // s, (x1 + s - 1) // s, (y1 + s - 1) // s
                whole = p[t]
                regions = [(py0, py1, px0, px1)] if not invert else [(0, py0, 0, whole.shape[2]), (py1, whole.shape[1], 0, whole.shape[2]), (py0, py1, 0, px0), (py0, py1, px1, whole.shape[2])]
                for a0, a1, b0, b1 in regions:
                    if a1 <= a0 or b1 <= b0:
                        continue
                    if mode == "fill":
                        whole[:, a0:a1, b0:b1] = 16
                    elif mode == "mosaic":
                        if cp < 2:
                            continue
                        win = whole[:, a0:a1, b0:b1].float().unsqueeze(0)
                        small = F.avg_pool2d(win, cp, ceil_mode=True, count_include_pad=False)
                        whole[:, a0:a1, b0:b1] = F.interpolate(small, scale_factor=cp, mode="nearest")[0, :, : a1 - a0, : b1 - b0].round().to(torch.uint8)
                    else:
                        h0, h1, w0, w1 = max(a0 - rp, 0), min(a1 + rp, whole.shape[1]), max(b0 - rp, 0), min(b1 + rp, whole.shape[2])  # the region and its neighbours
                        pooled = F.avg_pool2d(whole[:, h0:h1, w0:w1].float().unsqueeze(0), 2 * rp + 1, stride=1, padding=rp, count_include_pad=False)
                        whole[:, a0:a1, b0:b1] = pooled[0, :, a0 - h0 : a1 - h0, b0 - w0 : b1 - w0].round().to(torch.uint8)

    best = None
    for i in range(3):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        once()
        torch.cuda.synchronize()
        dt = 1e3 * (time.perf_counter() - t0)
        if i > 0:
            best = dt if best is None else min(best, dt)
    return best


def case(pix_fmt, mode, what, box, in_place, invert, n_clips, T, launches, dev, cache):
    lib = _hip.lib()
    n_tube = T // FPS_RATIO
    g = torch.Generator(device=dev).manual_seed(0)
    per_frame = 3 * H * W if pix_fmt == "rgb24" else H * W + 2 * ((H + 1) // 2) * ((W + 1) // 2)
    clips = [DeviceFrames(torch.randint(0, 256, (T * per_frame,), dtype=torch.uint8, device=dev, generator=g), T, H, W, pix_fmt, "bt709") for _ in range(n_clips)]
    outs = clips if in_place else [c.empty_like() for c in clips]
    fmap = (torch.arange(T, device=dev) // FPS_RATIO).int()
    jobs, keep = [], []
    for c, o in zip(clips, outs):
        boxes = make_boxes(n_tube, box, dev, g)
        keep.append(boxes)
        jobs.append(redact_job(c.data.data_ptr(), T, H, W, boxes.data_ptr(), n_tube, 1, o.data.data_ptr(), pix_fmt, None, fmap.data_ptr(), mode, what.get("cell", 16), what.get("radius", 8),
                               color_in_space((0, 0, 0), pix_fmt, "bt709", False), (0, 1), invert))
    arr = (_hip.RedactJob * n_clips)(*jobs)
    nb = int(lib.td_tube_redact_table_bytes(n_clips))
    ring = launches + 3  # one job-table pair per launch of a timing window: none is rewritten while a launch may still read it
    tab_h = torch.empty(ring * nb, dtype=torch.uint8, pin_memory=True)
    tab_d = torch.empty(ring * nb, dtype=torch.uint8, device=dev)
    slot = [0]

    def launch():
        o = (slot[0] % ring) * nb
        slot[0] += 1
        _hip.check(lib.td_tube_redact(arr, n_clips, tab_h.data_ptr() + o, tab_d.data_ptr() + o, nb, _hip.stream_ptr()), "td_tube_redact")

    med, lo, hi = median_ms(launch, launches)
    frame_bytes = sum(c.data.numel() for c in clips)
    a = torch.empty(frame_bytes, dtype=torch.uint8, device=dev)
    b = torch.empty_like(a)
    a.random_()
    cmed, clo, chi = median_ms(lambda: b.copy_(a), launches)
    del a, b
    key = (pix_fmt, mode, tuple(sorted(what.items())), box, invert)
    if key not in cache:
        cache[key] = torch_route(clips[0], keep[0], fmap, mode, what, invert)
    row = {"pix_fmt": pix_fmt, "mode": mode, **what, "box": box, "in_place": in_place, "invert": invert, "clips": n_clips, "frames_per_clip": T, "frame_hw": [H, W],
           "tube_rows_per_clip": n_tube, "launches_timed": launches, "device_ms_median": round(med, 4), "device_ms_min": round(lo, 4), "device_ms_max": round(hi, 4),
           "frame_bytes": int(frame_bytes), "copy_ms_median": round(cmed, 4), "copy_ms_min": round(clo, 4), "copy_ms_max": round(chi, 4),
           "copy_GBps": round(2 * frame_bytes / (cmed * 1e-3) / 1e9, 1), "time_over_copy": round(med / cmed, 4),
           "fraction_of_copy_bandwidth": None if in_place else round(cmed / med, 4), "us_per_frame": round(1e3 * med / (n_clips * T), 3),
           "torch_ms_one_clip": round(cache[key], 2), "torch_ms_scaled": round(cache[key] * n_clips, 1), "torch_over_kernel": round(cache[key] * n_clips / med, 1)}
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "redact_time.json"))
    ap.add_argument("--clips", type=int, default=16)
    ap.add_argument("--frames", type=int, default=100)
    ap.add_argument("--launches", type=int, default=25)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/redact_time.py measures on the GPU; none is visible")
    if a.launches < 20:
        raise SystemExit("the median is taken over at least 20 launches")
    dev = torch.device("cuda:0")
    samples = [smi()]
    rows, cache = [], {}
    for pix_fmt in ("yuv420p", "rgb24"):
        plan = [(mode, what, box, in_place, False) for mode, what in MODES for box in ("sixteenth", "frame") for in_place in ((False,) if mode == "blur" else (False, True))]
        plan.append(("mosaic", {"cell": 16}, "sixteenth", True, True))  # the spotlight: everything but the box
        for mode, what, box, in_place, invert in plan:
            r = case(pix_fmt, mode, what, box, in_place, invert, a.clips, a.frames, a.launches, dev, cache)
            rows.append(r)
            frac = "      -" if r["fraction_of_copy_bandwidth"] is None else f"{r['fraction_of_copy_bandwidth']:7.3f}"
            print(f"{pix_fmt:8s} {mode:6s} {str(what):14s} {box:9s} {'in place' if in_place else 'apart':8s} {'inv' if invert else '   '} {r['device_ms_median']:9.3f} ms   copy {r['copy_ms_median']:8.3f} ms   "
                  f"time/copy {r['time_over_copy']:7.3f}   fraction {frac}   torch route x{r['torch_over_kernel']}", flush=True)
            torch.cuda.empty_cache()
        samples.append(smi())
    out = {"device": torch.cuda.get_device_name(0), "smi_samples_before_between_after": samples,
           "method": "device events around every single launch, 3 warm-up launches, median of `launches_timed`; the copy is timed the same way right after its case; "
                     "the torch route by the host clock around one clip with a synchronise at both ends, scaled by the number of clips",
           "cases": rows}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
