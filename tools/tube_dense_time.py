"""Time td_tube_densify (tubedetr_amd.render.densify's launch): 16 clips of 100 tube rows, sampled every 6th frame, interpolated
to 600 decoded frames each.

Cases: K = 1 and K = 8 rectangles per row; without and with a 22 x 22 attention map per row; hold, lerp and hull; a table of
frame numbers on the device (what a sampler with irregular gaps gives).  Per case: every launch timed by its own pair of device
events after 3 warm-up launches, the MEDIAN of >= 20 launches, as tools/redact_time.py does.  ``bytes_moved`` is what the
algorithm has to read and write once (boxes, table, maps in; boxes, valid, span, maps out), computed from the shapes.

The baseline beside each case, in the same process, right after it: ``torch_ms_median`` - the same work with torch operators,
per clip a searchsorted, two gathers, the blend and the ``where``s for the frames outside the rows (and the same for the maps,
in float, rounded), in a Python loop over the clips; no host copy, so it is timed by device events around the whole loop, the
same way.  It does not smooth, has no span and no per-row presence: it is a cost yardstick for the plain case, not a reference.
The engine clocks and the socket power are read (rocm-smi --showclocks / --showpower, read-only) before and after, and recorded.

  python tools/tube_dense_time.py [--out profiles/tube_dense_time.json] [--clips 16] [--rows 100] [--frames 600] [--launches 25]
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from tubedetr_amd import _hip  # noqa: E402
from tubedetr_amd.render import DENSE_MODES, dense_job  # noqa: E402

MAP = (22, 22)


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


def torch_route(boxes, rf, heat, T, mode):
    """One clip with torch operators: (dense (T, K, 4), valid (T,), dense heat or None)."""
    f = torch.arange(T, device=boxes.device, dtype=torch.int32)
    a = (torch.searchsorted(rf, f, right=True) - 1).clamp_(0, rf.numel() - 1)
    b = (a + 1).clamp_(max=rf.numel() - 1)
    fa, fb = rf[a], rf[b]
    inside = (f >= rf[0]) & (f <= rf[-1])
    wgt = ((f - fa).float() / (fb - fa).clamp_(min=1).float())
    A, B = boxes[a], boxes[b]
    if mode == "hold":
        v = A
    elif mode == "lerp":
        v = A + wgt[:, None, None] * (B - A)
    else:
        v = torch.where((f == fa)[:, None, None], A, torch.cat([torch.minimum(A[..., :2], B[..., :2]), torch.maximum(A[..., 2:], B[..., 2:])], -1))
    v = torch.where(inside[:, None, None], v, torch.full_like(v, float("nan")))
    h = None
    if heat is not None:
        qa, qb = heat[a].float(), heat[b].float()
        h = qa if mode == "hold" else qa + wgt[:, None, None] * (qb - qa) if mode == "lerp" else torch.where((f == fa)[:, None, None], qa, torch.maximum(qa, qb))
        h = torch.where(inside[:, None, None], (h + 0.5).floor(), torch.zeros_like(h)).to(torch.uint8)
    return v, inside, h


def case(K, with_heat, mode, n_clips, n_tube, T, launches, dev):
    lib = _hip.lib()
    g = torch.Generator(device=dev).manual_seed(0)
    step = max(T // n_tube, 1)
    clips, jobs = [], []
    for _ in range(n_clips):
        x0, y0 = torch.rand(n_tube, K, 1, device=dev, generator=g) * 900, torch.rand(n_tube, K, 1, device=dev, generator=g) * 500
        boxes = torch.cat([x0, y0, x0 + 320, y0 + 180], -1).contiguous()
        rf = (torch.arange(n_tube, device=dev, dtype=torch.int32) * step).contiguous()
        heat = torch.randint(0, 256, (n_tube,) + MAP, dtype=torch.uint8, device=dev, generator=g) if with_heat else None
        out = dict(dense=torch.empty(T, K, 4, device=dev), valid=torch.empty(T, K, dtype=torch.uint8, device=dev), span=torch.empty(K, 2, dtype=torch.int64, device=dev),
                   heat=torch.empty((T,) + MAP, dtype=torch.uint8, device=dev) if with_heat else None)
        clips.append((boxes, rf, heat, out))
        jobs.append(dense_job(boxes.data_ptr(), n_tube, T, out["dense"].data_ptr(), K, row_frame=rf.data_ptr(), heat=_hip.ptr(heat), heat_hw=MAP if with_heat else (0, 0), mode=mode,
                              valid=out["valid"].data_ptr(), dense_span=out["span"].data_ptr(), dense_heat=_hip.ptr(out["heat"])))
    arr = (_hip.DenseJob * n_clips)(*jobs)
    nb = int(lib.td_tube_densify_table_bytes(n_clips))
    ring = launches + 3  # one job-table pair per launch of a timing window: none is rewritten while a launch may still read it
    tab_h = torch.empty(ring * nb, dtype=torch.uint8, pin_memory=True)
    tab_d = torch.empty(ring * nb, dtype=torch.uint8, device=dev)
    slot = [0]

    def launch():
        o = (slot[0] % ring) * nb
        slot[0] += 1
        _hip.check(lib.td_tube_densify(arr, n_clips, tab_h.data_ptr() + o, tab_d.data_ptr() + o, nb, _hip.stream_ptr()), "td_tube_densify")

    def torch_batch():
        return [torch_route(boxes, rf, heat, T, mode) for boxes, rf, heat, _ in clips]

    med, lo, hi = median_ms(launch, launches)
    tmed, tlo, thi = median_ms(torch_batch, launches)
    mb = MAP[0] * MAP[1] if with_heat else 0
    moved = n_clips * (n_tube * K * 16 + 4 * n_tube + n_tube * mb + T * K * 16 + T * K + 16 * K + T * mb)
    # the plain case is the one both routes define: where both have a box, it is the same box to a rounding or two
    v, inside, _ = torch_batch()[0]
    got = clips[0][3]["dense"]
    close = bool(torch.allclose(got[inside], v[inside], rtol=1e-5, atol=1e-3)) and bool(torch.isnan(got[~inside]).all())
    return {"K": K, "heat": list(MAP) if with_heat else None, "mode": mode, "clips": n_clips, "tube_rows_per_clip": n_tube, "frames_per_clip": T, "launches_timed": launches,
            "device_ms_median": round(med, 4), "device_ms_min": round(lo, 4), "device_ms_max": round(hi, 4), "bytes_moved": int(moved),
            "GBps_of_bytes_moved": round(moved / (med * 1e-3) / 1e9, 2), "torch_ms_median": round(tmed, 4), "torch_ms_min": round(tlo, 4), "torch_ms_max": round(thi, 4),
            "torch_over_kernel": round(tmed / med, 1), "agrees_with_torch_route": close}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tube_dense_time.json"))
    ap.add_argument("--clips", type=int, default=16)
    ap.add_argument("--rows", type=int, default=100)
    ap.add_argument("--frames", type=int, default=600)
    ap.add_argument("--launches", type=int, default=25)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/tube_dense_time.py measures on the GPU; none is visible")
    if a.launches < 20:
        raise SystemExit("the median is taken over at least 20 launches")
    dev = torch.device("cuda:0")
    samples = [smi()]
    rows = []
    for K in (1, 8):
        for with_heat in (False, True):
            for mode in DENSE_MODES:
                r = case(K, with_heat, mode, a.clips, a.rows, a.frames, a.launches, dev)
                rows.append(r)
                print(f"K {K}  heat {'22x22' if with_heat else '  -  '}  {mode:4s} {r['device_ms_median']:9.4f} ms   {r['bytes_moved']:9d} bytes   torch route {r['torch_ms_median']:9.4f} ms  x{r['torch_over_kernel']}"
                      f"   agrees {r['agrees_with_torch_route']}", flush=True)
    samples.append(smi())
    out = {"device": torch.cuda.get_device_name(0), "smi_samples_before_after": samples,
           "method": "device events around every single launch, 3 warm-up launches, median of `launches_timed`; the torch route (a Python loop over the clips, no host copy) is timed "
                     "the same way right after its case",
           "cases": rows}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
