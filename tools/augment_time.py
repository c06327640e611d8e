"""Time the device-side clip augmentation (td_clip_resample / td_clip_resample_src) for one training batch: 16 clips of
100 decoded frames.

Scenarios: (a) final 352 x 352 (what bench.py feeds) from 360 x 360 and 720 x 720 sources, (b) final 330 x 586 from
360 x 640 and 1280 x 720 sources (16:9 video at resolution 352); each with the evaluation plan (one resize) and with the
training transform's second arm (resize, crop, second resize: two launches through a uint8 intermediate).  Every
scenario runs twice in the same process, with the same plans: the source as packed rgb24 (3 bytes per pixel) and as
yuv420p (I420, 1.5 bytes per pixel, converted by the launch that reads it); ``pairs`` in the output puts the two side by side.

Per scenario:
  device_ms_per_batch      device events around >= 200 ms of repeated launches of the whole batch, after warm-up
  algorithmic_bytes        source bytes the windows touch, once, + bytes written (intermediates: written + read once)
  share_of_hbm_peak        algorithmic bytes / time / 8 TB/s (the HBM3E peak of the micro-architecture notes)
  host_plan_ms_per_clip    plan() for a 100-frame clip (draws + box arithmetic), one core
  host_pack_ms_per_clip    copying the decoded clip into page-locked memory, one core
  h2d_bytes_per_clip, h2d_ms_per_clip   the one host-to-device copy of the decoded frames (events)
  cv2_host_ms_per_clip     the reference-style host path (cv2.resize frame by frame, float64 clip array, normalise) on one
                           core where cv2 is importable, else "not measured"

  python tools/augment_time.py [--out profiles/augment_time.json] [--clips 16] [--frames 100]
"""
import argparse
import json
import os
import random
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from tubedetr_amd import _hip  # noqa: E402
from tubedetr_amd.augment import make_video_transforms, resample_job, resample_src_job  # noqa: E402

HBM_PEAK = 8.0e12


def first_tap(v, n_src, n_dst):
    num = (2 * v + 1) * n_src - n_dst
    return num // (2 * n_dst) if num > 0 else 0


def source_bytes(T, sh, sw, st, pix_fmt="rgb24"):
    rows = min(first_tap(st.wy + st.wh - 1, sh, st.rh) + 1, sh - 1) - first_tap(st.wy, sh, st.rh) + 1
    cols = min(first_tap(st.wx + st.ww - 1, sw, st.rw) + 1, sw - 1) - first_tap(st.wx, sw, st.rw) + 1
    if pix_fmt == "rgb24":
        return T * rows * cols * 3
    return T * (rows * cols + 2 * ((rows + 1) // 2) * ((cols + 1) // 2))  # the window's Y samples + their share of the two chroma planes


def plans_for(kind, n, T, h, w):
    tr = make_video_transforms("train" if kind == "train-branch-2" else "val", False, 352)
    targets = [{"boxes": torch.tensor([[0.3 * w, 0.3 * h, 0.7 * w, 0.7 * h]])} for _ in range(T)]
    plans, seed, t_plan = [], 0, []
    while len(plans) < n:
        random.seed(seed)
        torch.manual_seed(seed)
        seed += 1
        t0 = time.perf_counter()
        p = tr.plan(w, h, targets, "the person on the left")
        dt = time.perf_counter() - t0
        if len(p.stages) == (2 if kind == "train-branch-2" else 1):
            plans.append(p)
            t_plan.append(dt)
    return plans, 1e3 * float(np.median(t_plan))


def cv2_host_ms(T, h, w, plan):
    try:
        import cv2
    except ImportError:
        return "not measured"
    cv2.setNumThreads(1)
    clip = [np.random.randint(0, 256, (h, w, 3), dtype=np.uint8) for _ in range(T)]
    t0 = time.perf_counter()
    cur = clip
    for i, s in enumerate(plan.stages):
        if i == 0 and plan.flip:
            cur = [np.fliplr(f) for f in cur]
        cur = [cv2.resize(f, (s.rw, s.rh), interpolation=cv2.INTER_LINEAR)[s.wy : s.wy + s.wh, s.wx : s.wx + s.ww] for f in cur]
    arr = np.zeros([3, T, plan.hw[0], plan.hw[1]])
    for i, f in enumerate(cur):
        arr[:, i] = f.transpose(2, 0, 1)
    t = torch.from_numpy(arr).float().div(255)
    t.sub_(torch.tensor([0.485, 0.456, 0.406])[:, None, None, None]).div_(torch.tensor([0.229, 0.224, 0.225])[:, None, None, None])
    return round(1e3 * (time.perf_counter() - t0), 2)


def scenario(name, kind, h, w, n_clips, T, dev, min_ms, pix_fmt, plans, plan_ms):
    lib = _hip.lib()
    yuv = pix_fmt != "rgb24"
    H, W = max(p.hw[0] for p in plans), max(p.hw[1] for p in plans)
    clip_bytes = T * (h * w + 2 * ((h + 1) // 2) * ((w + 1) // 2)) if yuv else T * h * w * 3
    # decoded frames: random pixels made on the device (the timed launches do not care where they came from)
    raw = torch.randint(0, 256, (n_clips, clip_bytes), dtype=torch.uint8, device=dev)
    video = torch.empty((n_clips * T, 3, H, W), dtype=torch.uint8, device=dev)
    mask = torch.empty((n_clips * T, H, W), dtype=torch.bool, device=dev)
    first, final, mids, abytes = [], [], [], 0
    src_first, src_final = yuv, yuv and len(plans[0].stages) == 1  # the launch that reads the decoded frames takes their format

    def job(use_src, fmt, *a, **kw):
        return resample_src_job(*a, fmt, **kw) if use_src else resample_job(*a, **kw)

    for i, p in enumerate(plans):
        src, sh, sw, flip, fmt = raw[i].data_ptr(), h, w, p.flip, pix_fmt
        if len(p.stages) == 2:
            s = p.stages[0]
            mid = torch.empty((T, s.wh, s.ww, 3), dtype=torch.uint8, device=dev)
            mids.append(mid)
            first.append(job(src_first, fmt, src, T, sh, sw, flip, s, mid.data_ptr()))
            abytes += source_bytes(T, sh, sw, s, fmt) + mid.numel()
            src, sh, sw, flip, fmt = mid.data_ptr(), s.wh, s.ww, False, "rgb24"
        s = p.stages[-1]
        final.append(job(src_final, fmt, src, T, sh, sw, flip, s, video.data_ptr(), planar=True, frame_off=i * T, H=H, W=W, mask=mask.data_ptr()))
        abytes += source_bytes(T, sh, sw, s, fmt) + T * 4 * H * W
    launches = [((_hip.ResampleSrcJob if use_src else _hip.ResampleJob) * len(j))(*j) for j, use_src in ((first, src_first), (final, src_final)) if j]
    nb = int(max(lib.td_clip_resample_table_bytes(n_clips), lib.td_clip_resample_src_table_bytes(n_clips)))
    ring = 64  # job-table pairs: a pair is rewritten only after `ring` later launches, each synchronised batch-wise below
    tab_h = torch.empty(ring * nb, dtype=torch.uint8, pin_memory=True)
    tab_d = torch.empty(ring * nb, dtype=torch.uint8, device=dev)
    slot = [0]

    def batch():
        for arr in launches:
            o = (slot[0] % ring) * nb
            slot[0] += 1
            fn = lib.td_clip_resample_src if isinstance(arr[0], _hip.ResampleSrcJob) else lib.td_clip_resample
            _hip.check(fn(arr, len(arr), tab_h.data_ptr() + o, tab_d.data_ptr() + o, nb, _hip.stream_ptr()), "td_clip_resample")

    def timed(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            batch()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    timed(3)  # warm-up
    one = timed(4) / 4
    reps = min(max(int(min_ms / max(one, 1e-3)) + 1, 8), ring // len(launches))
    total, done = 0.0, 0
    while total < min_ms:  # windows of `reps` batches (bounded by the table ring), summed to >= min_ms of device time
        total += timed(reps)
        done += reps
    ms = total / done
    # the one host-to-device copy of a decoded clip, and packing it into page-locked memory
    host_clip = np.random.randint(0, 256, clip_bytes, dtype=np.uint8)
    pin = torch.empty(clip_bytes, dtype=torch.uint8, pin_memory=True)
    pack = []
    for _ in range(3):
        t0 = time.perf_counter()
        pin.copy_(torch.from_numpy(host_clip))
        pack.append(time.perf_counter() - t0)
    dst = torch.empty(clip_bytes, dtype=torch.uint8, device=dev)
    dst.copy_(pin, non_blocking=True)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(4):
        dst.copy_(pin, non_blocking=True)
    e1.record()
    torch.cuda.synchronize()
    h2d_ms = e0.elapsed_time(e1) / 4
    return {
        "name": name, "plan": kind, "pix_fmt": pix_fmt, "source_hw": [h, w], "final_hw_max": [H, W], "clips": n_clips, "frames_per_clip": T, "launches_per_batch": len(launches),
        "device_ms_per_batch": round(ms, 4), "timed_batches": done, "timed_device_ms": round(total, 1),
        "algorithmic_bytes": int(abytes), "achieved_GBps": round(abytes / (ms * 1e-3) / 1e9, 1), "share_of_hbm_peak": round(abytes / (ms * 1e-3) / HBM_PEAK, 4),
        "host_plan_ms_per_clip": round(plan_ms, 3), "host_pack_ms_per_clip": round(1e3 * float(np.median(pack)), 2),
        "h2d_bytes_per_clip": clip_bytes, "h2d_ms_per_clip": round(h2d_ms, 3), "h2d_GBps": round(clip_bytes / (h2d_ms * 1e-3) / 1e9, 1),
        "h2d_ms_per_batch": round(h2d_ms * n_clips, 2),
        "cv2_host_ms_per_clip": cv2_host_ms(T, h, w, plans[0]) if not yuv else "not measured",
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "augment_time.json"))
    ap.add_argument("--clips", type=int, default=16)
    ap.add_argument("--frames", type=int, default=100)
    ap.add_argument("--min-ms", type=float, default=200.0)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/augment_time.py measures on the GPU; none is visible")
    dev = torch.device("cuda:0")
    step_ms = None
    try:
        step_ms = json.load(open(os.path.join(ROOT, "BENCH_r06.json")))["parsed"]["ms_per_step"]
    except Exception:  # noqa: BLE001
        pass
    rows, pairs = [], []
    paired = ("h2d_bytes_per_clip", "h2d_ms_per_batch", "host_pack_ms_per_clip", "device_ms_per_batch")
    for name, h, w in (("352x352 from 360x360", 360, 360), ("352x352 from 720x720", 720, 720), ("330x586 from 360x640", 360, 640), ("330x586 from 720x1280", 720, 1280)):
        for kind in ("eval", "train-branch-2"):
            plans, plan_ms = plans_for(kind, a.clips, a.frames, h, w)
            for pix_fmt in ("rgb24", "yuv420p"):  # the twin: same plans, same process, source in I420
                rows.append(scenario(name, kind, h, w, a.clips, a.frames, dev, a.min_ms, pix_fmt, plans, plan_ms))
                r = rows[-1]
                if pix_fmt == "yuv420p":
                    pairs.append({"name": name, "plan": kind, "rgb24": {k: rows[-2][k] for k in paired}, "yuv420p": {k: r[k] for k in paired}})
                print(f"{name:24s} {kind:15s} {pix_fmt:8s} {r['device_ms_per_batch']:8.3f} ms/batch  {r['achieved_GBps']:7.1f} GB/s ({100 * r['share_of_hbm_peak']:.1f} % of 8 TB/s)  "
                      f"H2D {r['h2d_ms_per_batch']:.1f} ms/batch at {r['h2d_GBps']} GB/s  plan {r['host_plan_ms_per_clip']} ms  pack {r['host_pack_ms_per_clip']} ms/clip  "
                      f"cv2 {r['cv2_host_ms_per_clip']}", flush=True)
    out = {"device": torch.cuda.get_device_name(0), "hbm_peak_Bps": HBM_PEAK, "step_ms_of_the_16_clip_training_step": step_ms,
           "step_ms_source": "BENCH_r06.json (bench.py --gpus 1 --steps 20 --warmup 5)", "scenarios": rows, "pairs": pairs}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
