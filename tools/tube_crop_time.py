"""Time td_tube_crop (tubedetr_amd.render.crop_tubes' launch) against the route a user had before it existed: 16 clips of 100
decoded frames of 1280 x 720, one tube per clip at full rate (100 boxes of about 384 x 288 at random places), cropped with a
margin of 1/4 to 224 x 224, keep_aspect on; yuv420p and rgb24.

Two routes, in one process on the same boxes:
  crop_tubes   one call for the 16 clips.  ``device_ms_per_batch``: device events around enough consecutive calls to fill
               >= 200 ms (so the number includes what the calls do between launches: output allocation, the table copy);
               ``launch_only_ms``: the same around bare td_tube_crop launches into fixed outputs; ``enqueue_ms_per_call``: host
               wall clock of one call (nothing in it waits for the device).
  host_windows what the chain had to do before: boxes.cpu() (a synchronisation), the windows on the host (numpy, vectorised, the
               same rule), 1 600 one-frame resample_src_jobs, ONE td_clip_resample_src launch.  ``end_to_end_ms_per_batch``:
               host wall clock from before boxes.cpu() until the launch has finished, the median of several batches, with its parts;
               ``launch_only_ms``: device events around >= 200 ms of launches of the already built 1 600 jobs.
               For yuv420p this route cannot express a window whose origin is odd (its chroma is addressed from the sub-image):
               the origin is rounded down to even, so its pixels differ slightly there; the byte counts are the same.
``algorithmic_bytes``: the source bytes of the windows (ch cw 3, or ch cw 3 / 2 for yuv420p) read once + every output byte
written once (pixels, mask; crop_tubes: + valid, windows) + the boxes.  The engine clocks are read (rocm-smi --showclocks,
read-only) before and after and recorded.

  python tools/tube_crop_time.py [--out profiles/tube_crop_time.json] [--clips 16] [--frames 100]
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
from tubedetr_amd.augment import ResampleStage, resample_src_job  # noqa: E402
from tubedetr_amd.render import DeviceFrames, crop_job, crop_tubes  # noqa: E402

H, W, OUT, MARGIN = 720, 1280, (224, 224), (1, 4)
FILL_MS = 200.0


def clocks():
    try:
        txt = subprocess.run(["rocm-smi", "--showclocks", "-d", "0"], capture_output=True, text=True, timeout=30).stdout
        return [" ".join(l.split()) for l in txt.splitlines() if "sclk" in l or "mclk" in l or "fclk" in l] or "not available"
    except Exception as e:  # noqa: BLE001
        return f"not available ({type(e).__name__})"


def filled_ms(fn, warmup=3):
    """Device ms per call of fn, from one pair of events around enough consecutive calls to last >= FILL_MS."""
    for _ in range(warmup):
        fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    n = 4
    while True:
        torch.cuda.synchronize()
        a.record()
        for _ in range(n):
            fn()
        b.record()
        torch.cuda.synchronize()
        ms = a.elapsed_time(b)
        if ms >= FILL_MS:
            return ms / n, n
        n = max(2 * n, int(n * 1.3 * FILL_MS / max(ms, 1e-3)) + 1)


def host_windows(boxes: np.ndarray, even_origin: bool):
    """The rule of include/tubedetr_hip.h (steps 3 - 6, keep_aspect on) for finite boxes (n, 4), vectorised: (n, 6) int64, zeros for empties."""
    oh, ow = OUT
    r = np.floor(np.clip(boxes.astype(np.float32), -1048576.0, 1048576.0) + np.float32(0.5)).astype(np.int64)
    x0, y0, x1, y1 = r.T
    ok = (x1 > x0) & (y1 > y0)
    mx, my = (x1 - x0) * MARGIN[0] // MARGIN[1], (y1 - y0) * MARGIN[0] // MARGIN[1]
    wx0, wx1, wy0, wy1 = np.maximum(x0 - mx, 0), np.minimum(x1 + mx, W), np.maximum(y0 - my, 0), np.minimum(y1 + my, H)
    if even_origin:
        wx0, wy0 = wx0 & ~1, wy0 & ~1
    cw, ch = wx1 - wx0, wy1 - wy0
    ok &= (cw > 0) & (ch > 0)
    cw1, ch1 = np.maximum(cw, 1), np.maximum(ch, 1)
    wide = cw * oh >= ch * ow
    rh = np.where(wide, np.minimum(oh, np.maximum(1, (2 * ch * ow + cw) // (2 * cw1))), oh)
    rw = np.where(wide, ow, np.minimum(ow, np.maximum(1, (2 * cw * oh + ch) // (2 * ch1))))
    return np.stack([wy0, wx0, ch, cw, rh, rw], 1) * ok[:, None]


def case(pix_fmt, n_clips, T, dev):
    lib = _hip.lib()
    oh, ow = OUT
    g = torch.Generator(device=dev).manual_seed(0)
    yuv = pix_fmt != "rgb24"
    frame_bytes = H * W * 3 // 2 if yuv else 3 * H * W
    clips = [DeviceFrames(torch.randint(0, 256, (T * frame_bytes,), dtype=torch.uint8, device=dev, generator=g), T, H, W, pix_fmt, "bt709") for _ in range(n_clips)]
    boxes = []
    for _ in clips:
        x0, y0 = torch.rand(T, 1, device=dev, generator=g) * W * 0.7, torch.rand(T, 1, device=dev, generator=g) * H * 0.6
        boxes.append(torch.cat([x0, y0, x0 + W * 0.3, y0 + H * 0.4], 1).contiguous())
    all_boxes = torch.stack(boxes)
    kw = dict(size=OUT, margin=MARGIN, keep_aspect=True)

    # ---- crop_tubes
    crops = crop_tubes(clips, boxes, **kw)
    torch.cuda.synchronize()
    windows = np.concatenate([c.windows.cpu().numpy() for c in crops]).astype(np.int64)
    assert all(bool(c.valid.all()) for c in crops)
    del crops
    api_ms, api_n = filled_ms(lambda: crop_tubes(clips, boxes, **kw))
    t0 = time.perf_counter()
    for _ in range(20):
        crop_tubes(clips, boxes, **kw)
    enqueue_ms = (time.perf_counter() - t0) / 20 * 1e3
    torch.cuda.synchronize()
    pixels = torch.empty((n_clips * T, 3, oh, ow), dtype=torch.uint8, device=dev)
    mask = torch.empty((n_clips * T, oh, ow), dtype=torch.uint8, device=dev)
    valid = torch.empty((n_clips * T,), dtype=torch.uint8, device=dev)
    wins = torch.empty((n_clips * T, 6), dtype=torch.int32, device=dev)
    jobs = [crop_job(c.data.data_ptr(), T, H, W, b.data_ptr(), T, pixels[i * T :].data_ptr(), OUT, pix_fmt, "bt709", False, None, None, MARGIN, True,
                     mask[i * T :].data_ptr(), valid[i * T :].data_ptr(), wins[i * T :].data_ptr()) for i, (c, b) in enumerate(zip(clips, boxes))]
    arr = (_hip.CropJob * n_clips)(*jobs)
    nb = int(lib.td_tube_crop_table_bytes(n_clips))
    ring = 4096  # one job-table pair per launch of a timing window: none is rewritten while a launch may still read it
    tab_h = torch.empty(ring * nb, dtype=torch.uint8, pin_memory=True)
    tab_d = torch.empty(ring * nb, dtype=torch.uint8, device=dev)
    slot = [0]

    def crop_launch():
        o = (slot[0] % ring) * nb
        slot[0] += 1
        _hip.check(lib.td_tube_crop(arr, n_clips, tab_h.data_ptr() + o, tab_d.data_ptr() + o, nb, _hip.stream_ptr()), "td_tube_crop")

    crop_ms, crop_n = filled_ms(crop_launch)
    src_bytes = int((windows[:, 2] * windows[:, 3]).sum() * (1.5 if yuv else 3))
    out_bytes = n_clips * T * (3 * oh * ow + oh * ow)
    crop_bytes = src_bytes + out_bytes + n_clips * T * (1 + 24 + 16)

    # ---- the route without td_tube_crop
    n = n_clips * T
    nb2 = int(lib.td_clip_resample_src_table_bytes(n))
    ring2 = 64
    tab2_h = torch.empty(ring2 * nb2, dtype=torch.uint8, pin_memory=True)
    tab2_d = torch.empty(ring2 * nb2, dtype=torch.uint8, device=dev)
    cw2, ch2 = (W + 1) // 2, (H + 1) // 2
    state = {}

    def build():
        t0 = time.perf_counter()
        host_boxes = all_boxes.cpu().numpy().reshape(-1, 4)  # the synchronisation
        t1 = time.perf_counter()
        win = host_windows(host_boxes, even_origin=yuv)
        t2 = time.perf_counter()
        jobs2 = []
        for k in range(n):
            wy0, wx0, ch, cw, rh, rw = (int(v) for v in win[k])
            if rh == 0:
                continue
            base = clips[k // T].data.data_ptr() + (k % T) * frame_bytes
            if yuv:
                planes = [base + wy0 * W + wx0, base + H * W + (wy0 // 2) * cw2 + wx0 // 2, base + H * W + ch2 * cw2 + (wy0 // 2) * cw2 + wx0 // 2]
                pitches = [W, cw2, cw2]
            else:
                planes, pitches = [base + (wy0 * W + wx0) * 3], [3 * W]
            jobs2.append(resample_src_job(0, 1, ch, cw, False, ResampleStage(rh, rw, 0, 0, rh, rw), pixels.data_ptr(), pix_fmt, "bt709", False, planar=True, frame_off=k, H=oh, W=ow,
                                          mask=mask.data_ptr(), planes=planes, pitches=pitches, frame_stride=frame_bytes))
        state["arr"] = (_hip.ResampleSrcJob * len(jobs2))(*jobs2)
        state["n"] = len(jobs2)
        t3 = time.perf_counter()
        return t1 - t0, t2 - t1, t3 - t2

    def legacy_launch():
        o = (slot[0] % ring2) * nb2
        slot[0] += 1
        _hip.check(lib.td_clip_resample_src(state["arr"], state["n"], tab2_h.data_ptr() + o, tab2_d.data_ptr() + o, nb2, _hip.stream_ptr()), "td_clip_resample_src")

    parts, totals = [], []
    for i in range(7):
        crop_launch()  # the chain has work in flight when the host asks for the boxes
        t0 = time.perf_counter()
        p = build()
        legacy_launch()
        torch.cuda.synchronize()
        totals.append(time.perf_counter() - t0)
        parts.append(p)
    parts, totals = np.array(parts[2:]) * 1e3, np.array(totals[2:]) * 1e3
    legacy_ms, legacy_n = filled_ms(legacy_launch)
    legacy_bytes = src_bytes + out_bytes
    row = {"pix_fmt": pix_fmt, "clips": n_clips, "frames_per_clip": T, "frame_hw": [H, W], "crop_hw": list(OUT), "margin": list(MARGIN), "keep_aspect": True,
           "mean_window_hw": [round(float(windows[:, 2].mean()), 1), round(float(windows[:, 3].mean()), 1)],
           "crop_tubes": {"device_ms_per_batch": round(api_ms, 4), "calls_in_the_timed_window": api_n, "enqueue_ms_per_call": round(enqueue_ms, 4),
                          "launch_only_ms": round(crop_ms, 4), "launches_in_the_timed_window": crop_n, "algorithmic_bytes": crop_bytes,
                          "launch_only_GBps": round(crop_bytes / (crop_ms * 1e-3) / 1e9, 1), "jobs": n_clips},
           "host_windows": {"end_to_end_ms_per_batch": round(float(np.median(totals)), 4), "boxes_cpu_ms": round(float(np.median(parts[:, 0])), 4),
                            "windows_on_host_ms": round(float(np.median(parts[:, 1])), 4), "job_build_ms": round(float(np.median(parts[:, 2])), 4), "batches_timed": len(totals),
                            "launch_only_ms": round(legacy_ms, 4), "launches_in_the_timed_window": legacy_n, "algorithmic_bytes": legacy_bytes,
                            "launch_only_GBps": round(legacy_bytes / (legacy_ms * 1e-3) / 1e9, 1), "jobs": state["n"]}}
    row["launch_only_ratio_crop_over_resample_src"] = round(crop_ms / legacy_ms, 3)
    row["end_to_end_ratio_host_windows_over_crop_tubes"] = round(float(np.median(totals)) / api_ms, 2)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tube_crop_time.json"))
    ap.add_argument("--clips", type=int, default=16)
    ap.add_argument("--frames", type=int, default=100)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/tube_crop_time.py measures on the GPU; none is visible")
    dev = torch.device("cuda:0")
    before = clocks()
    rows = []
    for pix_fmt in ("yuv420p", "rgb24"):
        r = case(pix_fmt, a.clips, a.frames, dev)
        rows.append(r)
        c, h = r["crop_tubes"], r["host_windows"]
        print(f"{pix_fmt:8s} crop_tubes {c['device_ms_per_batch']:8.3f} ms/batch (launch {c['launch_only_ms']:.3f} ms, {c['launch_only_GBps']} GB/s, enqueue {c['enqueue_ms_per_call']:.3f} ms)   "
              f"host windows {h['end_to_end_ms_per_batch']:8.3f} ms/batch (boxes.cpu {h['boxes_cpu_ms']:.3f}, windows {h['windows_on_host_ms']:.3f}, jobs {h['job_build_ms']:.3f}, "
              f"launch {h['launch_only_ms']:.3f} ms, {h['launch_only_GBps']} GB/s)", flush=True)
        torch.cuda.empty_cache()
    out = {"device": torch.cuda.get_device_name(0), "clocks_before": before, "clocks_after": clocks(),
           "method": f"device numbers: one pair of events around >= {FILL_MS:.0f} ms of consecutive calls after 3 warm-up calls; host numbers: perf_counter, median of 5 batches after 2 warm-up batches",
           "cases": rows}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
