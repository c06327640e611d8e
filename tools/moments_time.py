"""Time td_sted_topk (tubedetr_amd.models.postprocessors.moments_topk's launch) beside a torch-op route for the same rule.

Cases: 16 videos x one window of T = 200, K = 5, nms 1/2 (a served batch of short clips); 1 video x P = 3840 positions as 16
windows of 240, K = 8, nms 1/2 (the longest video the kernel takes).

Per case: the SAME seeded logits for both routes in one process; 3 warm-up calls each, then 25 timed rounds, every call
between its own pair of device events, the order of the two routes alternating from round to round; the MEDIAN per route.
``kernel``: the single td_sted_topk launch into preallocated outputs.  ``torch_baseline`` - labelled as such, written here,
not part of the product - is what torch ops can express: two log-softmaxes, a (B, P, P) score tensor, and K rounds of
arg-max + a masked fill of the pairs whose temporal IoU with the pick is above the threshold; nothing in it synchronises.
Both routes are checked once to return the same pairs and counts (scores within 1e-5).

  python tools/moments_time.py [--out profiles/moments_time.json] [--launches 25]
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

NEG = float("-inf")


def clocks():
    try:
        txt = subprocess.run(["rocm-smi", "--showclocks", "-d", "0"], capture_output=True, text=True, timeout=30).stdout
        return [" ".join(l.split()) for l in txt.splitlines() if "sclk" in l or "mclk" in l or "fclk" in l] or "not available"
    except Exception as e:  # noqa: BLE001
        return f"not available ({type(e).__name__})"


def torch_baseline(z, K, num, den):
    """z fp32 [B, P, 2] (one row per video, windows already concatenated) -> pairs [B, K, 2], scores [B, K], count [B]."""
    B, P, _ = z.shape
    ls, le = z[:, :, 0].log_softmax(1), z[:, :, 1].log_softmax(1)
    score = le[:, :, None] + ls[:, None, :]  # [b, e, s]: the flat arg-max then prefers the smaller e, then the smaller s
    E, S = torch.arange(P, device=z.device)[:, None], torch.arange(P, device=z.device)[None, :]
    score = score.masked_fill((S >= E)[None], NEG)
    pairs, scores = [], []
    for _ in range(K):
        val, i = score.view(B, -1).max(1)
        e, s = (i // P)[:, None, None], (i % P)[:, None, None]
        ok = torch.isfinite(val)
        pairs.append(torch.where(ok[:, None], torch.stack([s.view(B), e.view(B)], 1), -1))
        scores.append(torch.where(ok, val, NEG))
        inter = (torch.minimum(E[None], e) - torch.maximum(S[None], s) + 1).clamp_(min=0)
        union = (E - S + 1)[None] + (e - s + 1) - inter
        drop = (inter * den > num * union) | ((E[None] == e) & (S[None] == s))
        score.masked_fill_(drop & ok[:, None, None], NEG)
    scores = torch.stack(scores, 1)
    return torch.stack(pairs, 1), scores, torch.isfinite(scores).sum(1).int()


def case(name, n_videos, n_win, T, K, nms, launches, dev):
    lib = _hip.lib()
    g = torch.Generator(device=dev).manual_seed(0)
    steds = torch.randn(n_videos * n_win, T, 2, device=dev, generator=g) * 4
    table = torch.arange(0, n_videos * n_win + 1, n_win, dtype=torch.int32, device=dev)
    pairs = torch.empty(n_videos, K, 2, dtype=torch.int64, device=dev)
    scores = torch.empty(n_videos, K, device=dev)
    count = torch.empty(n_videos, dtype=torch.int32, device=dev)
    flat = steds.view(n_videos, n_win * T, 2)
    ref = []

    def kernel():
        _hip.check(lib.td_sted_topk(steds.data_ptr(), None, table.data_ptr(), n_videos, n_videos * n_win, T, n_win, K, nms[0], nms[1],
                                    pairs.data_ptr(), scores.data_ptr(), count.data_ptr(), _hip.stream_ptr()), "td_sted_topk")

    def baseline():
        ref[:] = torch_baseline(flat, K, nms[0], nms[1])

    for _ in range(3):
        kernel()
        baseline()
    torch.cuda.synchronize()
    same = torch.equal(pairs, ref[0]) and torch.equal(count, ref[2]) and bool(((scores - ref[1]).abs()[torch.isfinite(ref[1])] <= 1e-5).all())
    if not same:
        raise SystemExit(f"{name}: the two routes disagree")
    routes = {"kernel": kernel, "torch_baseline": baseline}
    ev = {r: [] for r in routes}
    for i in range(launches):
        for r in (("kernel", "torch_baseline") if i % 2 == 0 else ("torch_baseline", "kernel")):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            routes[r]()
            b.record()
            ev[r].append((a, b))
    torch.cuda.synchronize()
    row = {"case": name, "videos": n_videos, "windows_per_video": n_win, "T": T, "positions_per_video": n_win * T, "K": K, "nms": list(nms),
           "launches_timed": launches, "routes_agree": same, "picks_made": count.tolist()}
    for r in routes:
        ms = sorted(a.elapsed_time(b) for a, b in ev[r])
        row[r] = {"device_ms_median": round(float(np.median(ms)), 4), "device_ms_min": round(ms[0], 4), "device_ms_max": round(ms[-1], 4)}
    row["torch_baseline"]["label"] = "BASELINE written in tools/moments_time.py from torch ops: (B, P, P) scores, K rounds of arg-max + masked fill"
    row["baseline_over_kernel"] = round(row["torch_baseline"]["device_ms_median"] / row["kernel"]["device_ms_median"], 2)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "moments_time.json"))
    ap.add_argument("--launches", type=int, default=25)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/moments_time.py measures on the GPU; none is visible")
    dev = torch.device("cuda:0")
    before = clocks()
    rows = []
    for name, n_videos, n_win, T, K in (("16 videos x 200", 16, 1, 200, 5), ("1 video x 3840 (16 windows of 240)", 1, 16, 240, 8)):
        r = case(name, n_videos, n_win, T, K, (1, 2), a.launches, dev)
        rows.append(r)
        print(f"{name:38s} kernel {r['kernel']['device_ms_median']:8.4f} ms   torch baseline {r['torch_baseline']['device_ms_median']:8.4f} ms   "
              f"x{r['baseline_over_kernel']}", flush=True)
        torch.cuda.empty_cache()
    out = {"device": torch.cuda.get_device_name(0), "clocks_before": before, "clocks_after": clocks(),
           "method": "device events around every single call, 3 warm-up calls per route, the two routes alternate, median of `launches_timed`",
           "cases": rows}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
