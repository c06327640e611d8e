"""Time td_tube_overlay (tubedetr_amd.render.annotate's launch): 16 clips of 100 decoded frames of 1280 x 720 annotated with a
tube predicted at 5 fps (20 tube rows per clip, frame_map t // 5, span rows 5..14).

Cases: yuv420p and rgb24; the box alone and box + attention map (23 x 40 tokens) + dimming; in place and out of place.
Per case: every launch timed by its own pair of device events after 3 warm-up launches, the MEDIAN of >= 20 launches;
``bytes_moved`` = every source byte read once + every destination byte written once (+ the maps and boxes, once);
``copy_*``: a plain device copy (torch ``copy_``, what tools/hbm_copy_bw.py times) of the same number of bytes - bytes_moved / 2
read and as many written - timed the same way in the SAME process right after the case; ``fraction_of_copy_bandwidth`` is
the number to report.  The engine clocks are read (rocm-smi --showclocks, read-only) before and after and recorded.

``host_route`` - labelled as such, not a device number - is what the reference's demo pays instead: the frames go back over
PCIe, are drawn on the host cores (here: tests/overlay_ref.py, numpy, one core, per frame) and return over PCIe.

  python tools/overlay_time.py [--out profiles/overlay_time.json] [--clips 16] [--frames 100] [--launches 25]
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from tubedetr_amd import _hip  # noqa: E402
from tubedetr_amd.render import DeviceFrames, TubeStyle, color_in_space, overlay_job  # noqa: E402

H, W, GRID, FPS_RATIO = 720, 1280, (23, 40), 5


def clocks():
    try:
        txt = subprocess.run(["rocm-smi", "--showclocks", "-d", "0"], capture_output=True, text=True, timeout=30).stdout
        return [" ".join(l.split()) for l in txt.splitlines() if "sclk" in l or "mclk" in l or "fclk" in l] or "not available"
    except Exception as e:  # noqa: BLE001
        return f"not available ({type(e).__name__})"


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


def case(pix_fmt, layers, in_place, n_clips, T, launches, dev):
    lib = _hip.lib()
    style = TubeStyle(thickness=4, heat_alpha=144 if layers == "box+heat+dim" else 0, dim_alpha=96 if layers == "box+heat+dim" else 0, heat_color=(255, 64, 0))
    space = (pix_fmt, "bt709", False)
    n_tube = T // FPS_RATIO
    g = torch.Generator(device=dev).manual_seed(0)
    clips = [DeviceFrames(torch.randint(0, 256, (T * (3 * H * W if pix_fmt == "rgb24" else H * W * 3 // 2),), dtype=torch.uint8, device=dev, generator=g), T, H, W, pix_fmt, "bt709")
             for _ in range(n_clips)]
    outs = clips if in_place else [c.empty_like() for c in clips]
    fmap = (torch.arange(T, device=dev) // FPS_RATIO).int()
    span = torch.tensor([n_tube // 4, 3 * n_tube // 4 - 1], device=dev)
    jobs, keep, extra = [], [], 0
    for i, (c, o) in enumerate(zip(clips, outs)):
        x0, y0 = torch.rand(n_tube, 1, device=dev, generator=g) * W * 0.5, torch.rand(n_tube, 1, device=dev, generator=g) * H * 0.5
        boxes = torch.cat([x0, y0, x0 + W * 0.3, y0 + H * 0.4], 1).contiguous()
        heat = torch.randint(0, 256, (n_tube,) + GRID, dtype=torch.uint8, device=dev, generator=g) if layers == "box+heat+dim" else None
        keep.append((boxes, heat))
        extra += boxes.numel() * 4 + (heat.numel() if heat is not None else 0) + fmap.numel() * 4 + 16
        jobs.append(overlay_job(c.data.data_ptr(), T, H, W, o.data.data_ptr(), pix_fmt, boxes.data_ptr(), n_tube, span.data_ptr() if heat is not None else None, fmap.data_ptr(),
                                heat.data_ptr() if heat is not None else None, GRID if heat is not None else (0, 0), color_in_space(style.box_color, *space),
                                color_in_space(style.heat_color, *space), color_in_space(style.dim_color, *space), style.thickness, style.heat_alpha, style.dim_alpha))
    arr = (_hip.OverlayJob * n_clips)(*jobs)
    nb = int(lib.td_tube_overlay_table_bytes(n_clips))
    ring = launches + 3  # one job-table pair per launch of a timing window: none is rewritten while a launch may still read it
    tab_h = torch.empty(ring * nb, dtype=torch.uint8, pin_memory=True)
    tab_d = torch.empty(ring * nb, dtype=torch.uint8, device=dev)
    slot = [0]

    def launch():
        o = (slot[0] % ring) * nb
        slot[0] += 1
        _hip.check(lib.td_tube_overlay(arr, n_clips, tab_h.data_ptr() + o, tab_d.data_ptr() + o, nb, _hip.stream_ptr()), "td_tube_overlay")

    med, lo, hi = median_ms(launch, launches)
    frame_bytes = sum(c.data.numel() for c in clips)
    moved = 2 * frame_bytes + extra
    # the copy yardstick: as many bytes read and as many written, same process, same moment
    a = torch.empty(moved // 2, dtype=torch.uint8, device=dev)
    b = torch.empty_like(a)
    a.random_()
    cmed, clo, chi = median_ms(lambda: b.copy_(a), launches)
    return {"pix_fmt": pix_fmt, "layers": layers, "in_place": in_place, "clips": n_clips, "frames_per_clip": T, "frame_hw": [H, W], "tube_rows_per_clip": n_tube,
            "launches_timed": launches, "device_ms_median": round(med, 4), "device_ms_min": round(lo, 4), "device_ms_max": round(hi, 4),
            "bytes_moved": int(moved), "achieved_GBps": round(moved / (med * 1e-3) / 1e9, 1),
            "copy_ms_median": round(cmed, 4), "copy_ms_min": round(clo, 4), "copy_ms_max": round(chi, 4), "copy_GBps": round(moved / (cmed * 1e-3) / 1e9, 1),
            "fraction_of_copy_bandwidth": round(cmed / med, 4), "us_per_frame": round(1e3 * med / (n_clips * T), 3)}


def host_route(pix_fmt, layers, T, dev):
    """The demo's route for ONE clip, per frame: device -> host, draw on one host core (tests/overlay_ref.py), host -> device."""
    from overlay_ref import overlay_ref

    rng = np.random.default_rng(0)
    ch, cw = (H + 1) // 2, (W + 1) // 2
    planes = rng.integers(0, 256, (1, H, W, 3), dtype=np.uint8) if pix_fmt == "rgb24" else tuple(rng.integers(0, 256, s, dtype=np.uint8) for s in ((1, H, W), (1, ch, cw), (1, ch, cw)))
    kw = {"boxes": np.array([[300.2, 200.7, 700.1, 500.5]], dtype=np.float32), "thickness": 4}
    if layers == "box+heat+dim":
        kw.update(heat=rng.integers(0, 256, (1,) + GRID, dtype=np.uint8), heat_alpha=144, span=(0, 0), dim_alpha=96)
    draw = []
    for _ in range(5):
        t0 = time.perf_counter()
        overlay_ref(planes, pix_fmt, **kw)
        draw.append(time.perf_counter() - t0)
    clip_bytes = T * (3 * H * W if pix_fmt == "rgb24" else H * W + 2 * ch * cw)
    d = torch.empty(clip_bytes, dtype=torch.uint8, device=dev)
    pin = torch.empty(clip_bytes, dtype=torch.uint8, pin_memory=True)
    d2h = median_ms(lambda: pin.copy_(d, non_blocking=True), 20)[0]
    h2d = median_ms(lambda: d.copy_(pin, non_blocking=True), 20)[0]
    return {"label": "HOST ROUTE (not a device number): per frame of one clip, numpy reference on one host core + the two PCIe copies", "pix_fmt": pix_fmt, "layers": layers,
            "host_draw_ms_per_frame": round(1e3 * float(np.median(draw)), 2), "d2h_ms_per_frame": round(d2h / T, 4), "h2d_ms_per_frame": round(h2d / T, 4),
            "pcie_GBps_d2h": round(clip_bytes / (d2h * 1e-3) / 1e9, 1), "pcie_GBps_h2d": round(clip_bytes / (h2d * 1e-3) / 1e9, 1),
            "host_route_ms_per_frame": round(1e3 * float(np.median(draw)) + (d2h + h2d) / T, 2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "overlay_time.json"))
    ap.add_argument("--clips", type=int, default=16)
    ap.add_argument("--frames", type=int, default=100)
    ap.add_argument("--launches", type=int, default=25)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/overlay_time.py measures on the GPU; none is visible")
    if a.launches < 20:
        raise SystemExit("the median is taken over at least 20 launches")
    dev = torch.device("cuda:0")
    before = clocks()
    rows, host = [], []
    for pix_fmt in ("yuv420p", "rgb24"):
        for layers in ("box", "box+heat+dim"):
            for in_place in (False, True):
                r = case(pix_fmt, layers, in_place, a.clips, a.frames, a.launches, dev)
                rows.append(r)
                print(f"{pix_fmt:8s} {layers:13s} {'in place' if in_place else 'out of place':12s} {r['device_ms_median']:8.3f} ms  {r['achieved_GBps']:7.1f} GB/s   "
                      f"copy {r['copy_ms_median']:8.3f} ms {r['copy_GBps']:7.1f} GB/s   fraction {r['fraction_of_copy_bandwidth']:.3f}   {r['us_per_frame']} us/frame", flush=True)
                torch.cuda.empty_cache()
            host.append(host_route(pix_fmt, layers, a.frames, dev))
            print(f"  host route: {host[-1]['host_route_ms_per_frame']} ms/frame (draw {host[-1]['host_draw_ms_per_frame']}, PCIe {host[-1]['d2h_ms_per_frame']} + {host[-1]['h2d_ms_per_frame']})", flush=True)
    out = {"device": torch.cuda.get_device_name(0), "clocks_before": before, "clocks_after": clocks(),
           "method": "device events around every single launch, 3 warm-up launches, median of `launches_timed`; the copy is timed the same way right after its case",
           "cases": rows, "host_route": host}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
