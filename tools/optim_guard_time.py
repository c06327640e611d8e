"""Time the optimizer tail with and without the non-finite-step guard at the real model's parameter count.

Buffers: 185 234 182 fp32 elements (the reference's trainable parameters), EMA on, the three reference groups in
five segments - transformer + heads (group 0) in two pieces, the text encoder (group 2) with its pooler as an INACTIVE segment
(it never receives a gradient), the backbone (group 1); the piece lengths are odd so that segment boundaries fall inside
float4s, as they do in the model.  Seeded finite gradients of norm ~1, max_norm 0.1.

Routes, on the SAME buffers in one process:
  ``unguarded``        td_grad_norm_clip + td_adamw_ema_step                    (FusedAdamWEMA's default launches)
  ``guarded``          td_grad_norm_clip_guarded + td_adamw_ema_step_guarded    (skip_nonfinite=True), every step applied
  ``guarded_skipped``  the guarded pair over a gradient buffer with one NaN: the norm pass and an update that returns at once
3 warm-up calls per route, then ``--rounds`` timed rounds in which ``unguarded`` and ``guarded`` alternate, each leading every
other round, and after them ``--rounds`` calls of ``guarded_skipped``; every call sits between its own pair of device events.
Reported per route: median, min, max and the quartiles of the device times; the spread of the unguarded runs (max - min and
the inter-quartile range, relative to its median) and guarded / unguarded.

  python tools/optim_guard_time.py [--out profiles/optim_guard_time.json] [--rounds 30]
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

N_TOTAL = 185_234_182
TEXT_ENCODER, POOLER, BACKBONE = 124_645_632, 590_592, 42_170_001  # roberta-base (its pooler included); ResNet-101 layer2-4
# (length, group, active) in flat-buffer order
PIECES = [(9_000_001, 0, 1), (TEXT_ENCODER - POOLER, 2, 1), (POOLER, 2, 0), (N_TOTAL - TEXT_ENCODER - BACKBONE - 9_000_001, 0, 1), (BACKBONE, 1, 1)]
LRS = (5e-5, 1e-5, 5e-5, 0.0)
BETA1, BETA2, EPS, WD, EMA_DECAY, MAX_NORM = 0.9, 0.999, 1e-8, 1e-4, 0.9998, 0.1
HISTORY = 64


def clocks():
    try:
        txt = subprocess.run(["rocm-smi", "--showclocks", "-d", "0"], capture_output=True, text=True, timeout=30).stdout
        return [" ".join(l.split()) for l in txt.splitlines() if "sclk" in l or "mclk" in l or "fclk" in l] or "not available"
    except Exception as e:  # noqa: BLE001
        return f"not available ({type(e).__name__})"


def stats(ms):
    ms = np.sort(np.asarray(ms, np.float64))
    q1, med, q3 = (float(np.percentile(ms, q)) for q in (25, 50, 75))
    return {"device_ms_median": round(med, 4), "device_ms_min": round(float(ms[0]), 4), "device_ms_max": round(float(ms[-1]), 4),
            "device_ms_q1": round(q1, 4), "device_ms_q3": round(q3, 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "optim_guard_time.json"))
    ap.add_argument("--rounds", type=int, default=30)
    ap.add_argument("--scale", type=float, default=1.0, help="shrink every segment (a rehearsal; the committed profile is scale 1)")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/optim_guard_time.py measures on the GPU; none is visible")
    dev = torch.device("cuda:0")
    L = _hip.lib()
    pieces = [(max(1, int(ln * a.scale)) | 1 if a.scale != 1.0 else ln, g, act) for ln, g, act in PIECES]
    n = sum(ln for ln, _, _ in pieces)
    assert a.scale != 1.0 or n == N_TOTAL
    segs, at = (_hip.OptimSegment * len(pieces))(), 0
    for s, (ln, g, act) in zip(segs, pieces):
        s.begin, s.end, s.group, s.active = at, at + ln, g, act
        at += ln
    gen = torch.Generator(device=dev).manual_seed(0)
    p = torch.randn(n, device=dev, generator=gen) * 0.02
    ema = p.clone()
    m, v = torch.zeros_like(p), torch.zeros_like(p)
    grad = torch.randn(n, device=dev, generator=gen) / float(np.sqrt(n))  # norm ~1: clipped to 0.1 like most training steps
    grad_bad = grad.clone()
    grad_bad[n // 3] = float("nan")  # inside the text encoder's active segment
    lr = torch.tensor(LRS, dtype=torch.float32, device=dev)
    step = torch.zeros(1, dtype=torch.int32, device=dev)
    norm_clip = torch.zeros(2, dtype=torch.float32, device=dev)
    loss = torch.ones(1, dtype=torch.float32, device=dev)
    ws = torch.empty(L.td_grad_norm_guard_ws_bytes(), dtype=torch.uint8, device=dev)  # (the unguarded call uses its first part)
    guard = torch.zeros(L.td_guard_bytes(HISTORY), dtype=torch.uint8, device=dev)
    hyper = (BETA1, BETA2, EPS, WD, EMA_DECAY)

    def tail(g, guarded):
        st = _hip.stream_ptr()
        norm_args = (g.data_ptr(), n, segs, len(segs), MAX_NORM, ws.data_ptr(), ws.numel(), norm_clip.data_ptr(), step.data_ptr())
        adam_args = (p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), ema.data_ptr(), n, segs, len(segs), lr.data_ptr(), norm_clip.data_ptr(),
                     step.data_ptr()) + hyper
        if guarded:
            _hip.check(L.td_grad_norm_clip_guarded(*norm_args, loss.data_ptr(), guard.data_ptr(), HISTORY, st), "td_grad_norm_clip_guarded")
            _hip.check(L.td_adamw_ema_step_guarded(*adam_args, guard.data_ptr(), st), "td_adamw_ema_step_guarded")
        else:
            _hip.check(L.td_grad_norm_clip(*norm_args, st), "td_grad_norm_clip")
            _hip.check(L.td_adamw_ema_step(*adam_args, st), "td_adamw_ema_step")

    routes = {"unguarded": lambda: tail(grad, False), "guarded": lambda: tail(grad, True), "guarded_skipped": lambda: tail(grad_bad, True)}
    before = clocks()
    for _ in range(3):
        for r in routes.values():
            r()
    torch.cuda.synchronize()
    ev = {r: [] for r in routes}

    def timed(r):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        routes[r]()
        e1.record()
        ev[r].append((e0, e1))

    for i in range(a.rounds):  # the two routes that are compared alternate strictly, each one leading every other round
        for r in (("unguarded", "guarded") if i % 2 == 0 else ("guarded", "unguarded")):
            timed(r)
    for _ in range(a.rounds):  # the skipped step leaves other data in the caches behind it: timed after the comparison, not inside it
        timed("guarded_skipped")
    torch.cuda.synchronize()
    counters = guard[:16].view(torch.int32).tolist()
    applied = 2 * (3 + a.rounds)
    if not (torch.isfinite(p).all().item() and torch.isfinite(ema).all().item() and step.item() == applied and counters[:2] == [applied, 3 + a.rounds]):
        raise SystemExit(f"the run itself went wrong: step {step.item()}, guard header {counters}")
    rows = {r: stats([e0.elapsed_time(e1) for e0, e1 in ev[r]]) for r in routes}
    u, g = rows["unguarded"], rows["guarded"]
    n_inactive = sum(ln for ln, _, act in pieces if not act)
    # the norm pass reads grad; the update reads 5 and writes 4 buffers (inactive: reads param and ema, writes ema)
    tail_bytes = 4 * (n + 9 * (n - n_inactive) + 3 * n_inactive)
    out = {"device": torch.cuda.get_device_name(0), "clocks_before": before, "clocks_after": clocks(),
           "method": "device events around every call of a pair of entry points, 3 warm-up calls per route, unguarded and guarded alternate (each leads every "
                     "other round), guarded_skipped is timed after them; one process, the same buffers",
           "elements": n, "segments": [{"begin": s.begin, "end": s.end, "group": s.group, "active": s.active} for s in segs], "ema": True,
           "history": HISTORY, "rounds_timed": a.rounds, "routes": rows,
           "unguarded_spread_max_minus_min_over_median": round((u["device_ms_max"] - u["device_ms_min"]) / u["device_ms_median"], 4),
           "unguarded_spread_iqr_over_median": round((u["device_ms_q3"] - u["device_ms_q1"]) / u["device_ms_median"], 4),
           "guarded_over_unguarded_median": round(g["device_ms_median"] / u["device_ms_median"], 4),
           "guarded_median_inside_unguarded_min_max": bool(u["device_ms_min"] <= g["device_ms_median"] <= u["device_ms_max"]),
           "unguarded_algorithmic_GB_per_s": round(tail_bytes / (u["device_ms_median"] * 1e-3) / 1e9, 1),
           "steps_applied": step.item(), "guard_header_after": dict(zip(("attempts", "skipped", "consecutive_skipped", "applied_now"), counters))}
    for r, row in rows.items():
        print(f"{r:16s} median {row['device_ms_median']:8.4f} ms   min {row['device_ms_min']:8.4f}   max {row['device_ms_max']:8.4f}", flush=True)
    print("guarded / unguarded", out["guarded_over_unguarded_median"], "  unguarded (max - min) / median", out["unguarded_spread_max_minus_min_over_median"])
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
