"""Time td_tube_overlay_multi (tubedetr_amd.render.annotate_tubes' launch) against what it replaces: 16 clips of 100 decoded
frames of 1280 x 720, K tubes predicted at 5 fps (20 tube rows per clip, frame_map t // 5, tube k's span a third of the rows).

Configurations: yuv420p and rgb24; K = 1 / 4 / 8; outlines alone or with tags (scale 2) and the timeline (lanes of 6 rows);
without and with the attention map (23 x 40 tokens) and dimming.  Everything writes src -> dst (out of place).  Candidates:
  multi       ONE td_tube_overlay_multi launch;
  sequential  what ``annotate`` needs for the same K outlines: K td_tube_overlay launches, the first src -> dst (it carries the
              heat and dim layers when they are on), the others in place on dst with tube k's boxes, span and colour.  It draws
              neither tags nor timeline - it cannot - so with those on it is the cheaper picture;
  copy        a plain device copy (torch ``copy_``) of the frames, src -> dst: the floor of any out-of-place pass;
  overlay     K = 1 only: td_tube_overlay itself on the same inputs (the identity case of the rule).
The candidates ALTERNATE within one process: a round times each candidate once (every launch by its own pair of device events
after 2 warm-up launches, the median of ``--launches``), and there are ``--rounds`` >= 3 rounds, so that each candidate's own
spread between rounds is recorded next to the ratios (two runs understate it).  ``*_ms`` is the median of the round medians,
``*_ms_rounds`` the round medians.  ``k1_inside_overlay_spread`` says whether multi's median at K = 1 lies inside
[min, max] of td_tube_overlay's round medians.

  python tools/overlay_multi_time.py [--out profiles/overlay_multi_time.json] [--clips 16] [--frames 100] [--launches 10] [--rounds 3]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from tubedetr_amd import _hip  # noqa: E402
from tubedetr_amd.render import PALETTE, color_in_space, label_tags, overlay_job, overlay_multi_job  # noqa: E402

H, W, GRID, FPS_RATIO = 720, 1280, (23, 40), 5


def median_ms(fn, launches, warmup=2):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(launches)]
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    return float(np.median([a.elapsed_time(b) for a, b in ev]))


class Launcher:
    """A prepared array of jobs and a ring of job tables: one table per launch of a timing window, none rewritten while a launch may read it."""

    def __init__(self, entry, jobs, ring, dev):
        self.lib, self.entry, self.n = _hip.lib(), entry, len(jobs)
        self.arr = (type(jobs[0]) * len(jobs))(*jobs)
        self.nb = int(getattr(self.lib, entry + "_table_bytes")(len(jobs)))
        self.ring, self.slot = ring, 0
        self.host = torch.empty(ring * self.nb, dtype=torch.uint8, pin_memory=True)
        self.dev = torch.empty(ring * self.nb, dtype=torch.uint8, device=dev)

    def __call__(self):
        o = (self.slot % self.ring) * self.nb
        self.slot += 1
        _hip.check(getattr(self.lib, self.entry)(self.arr, self.n, self.host.data_ptr() + o, self.dev.data_ptr() + o, self.nb, _hip.stream_ptr()), self.entry)


def case(pix_fmt, K, extras, heat_on, n_clips, T, launches, rounds, dev):
    space = (pix_fmt, "bt709", False)
    n_tube = T // FPS_RATIO
    per_frame = 3 * H * W if pix_fmt == "rgb24" else H * W * 3 // 2
    g = torch.Generator(device=dev).manual_seed(0)
    src = [torch.randint(0, 256, (T * per_frame,), dtype=torch.uint8, device=dev, generator=g) for _ in range(n_clips)]
    dst = [torch.empty_like(s) for s in src]
    fmap = (torch.arange(T, device=dev) // FPS_RATIO).int()
    third = max(n_tube // 3, 1)
    span = torch.tensor([[(k * third // 2) % n_tube, min((k * third // 2) % n_tube + third - 1, n_tube - 1)] for k in range(K)], device=dev)
    tags = label_tags([f"{k}: SENTENCE {k}" for k in range(K)], dev) if extras else None
    colors = [color_in_space(c, *space) for c in PALETTE]
    heat_c, dim_c = color_in_space((255, 64, 0), *space), color_in_space((0, 0, 0), *space)
    heat_kw = dict(heat_color=heat_c, dim_color=dim_c, heat_alpha=144 if heat_on else 0, dim_alpha=96 if heat_on else 0, thickness=4)
    multi, seq, one, keep = [], [[] for _ in range(K)], [], []
    for s, d in zip(src, dst):
        x0, y0 = torch.rand(n_tube, K, 1, device=dev, generator=g) * W * 0.5, torch.rand(n_tube, K, 1, device=dev, generator=g) * H * 0.5
        boxes = torch.cat([x0, y0, x0 + W * 0.3, y0 + H * 0.4], 2).contiguous()
        heat = torch.randint(0, 256, (n_tube,) + GRID, dtype=torch.uint8, device=dev, generator=g) if heat_on else None
        per_tube = [boxes[:, k].contiguous() for k in range(K)]
        keep.append((boxes, heat, per_tube))
        hp, hw = (heat.data_ptr(), GRID) if heat_on else (None, (0, 0))
        multi.append(overlay_multi_job(s.data_ptr(), T, H, W, d.data_ptr(), pix_fmt, boxes.data_ptr(), n_tube, K, span.data_ptr(), fmap.data_ptr(), hp, hw,
                                       tags.data_ptr() if extras else None, tuple(tags.shape[1:]) if extras else (0, 0), 2, 224, color_in_space((0, 0, 0), *space), colors,
                                       lane_h=6 if extras else 0, bar_color=color_in_space((32, 32, 32), *space), bar_alpha=160, seg_alpha=256,
                                       cursor_color=color_in_space((255, 255, 255), *space), **heat_kw))
        for k in range(K):  # pass 0 reads src and carries heat and dim; the others run in place on dst
            first = k == 0
            seq[k].append(overlay_job(s.data_ptr() if first else d.data_ptr(), T, H, W, d.data_ptr(), pix_fmt, per_tube[k].data_ptr(), n_tube, span[k].data_ptr(), fmap.data_ptr(),
                                      hp if first else None, hw if first else (0, 0), box_color=colors[k], **(heat_kw if first else dict(thickness=4))))
        if K == 1:
            one.append(overlay_job(s.data_ptr(), T, H, W, d.data_ptr(), pix_fmt, boxes.data_ptr(), n_tube, span.data_ptr(), fmap.data_ptr(), hp, hw, box_color=colors[0], **heat_kw))
    ring = launches + 2
    run_multi = Launcher("td_tube_overlay_multi", multi, ring, dev)
    run_seq = [Launcher("td_tube_overlay", j, ring, dev) for j in seq]
    run_one = Launcher("td_tube_overlay", one, ring, dev) if K == 1 else None

    def sequential():
        for r in run_seq:
            r()

    def copy():
        for s, d in zip(src, dst):
            d.copy_(s)

    cands = {"multi": run_multi, "sequential": sequential, "copy": copy}
    if run_one is not None:
        cands["overlay"] = run_one
    per_round = {k: [] for k in cands}
    for _ in range(rounds):
        for name, fn in cands.items():
            per_round[name].append(median_ms(fn, launches))
    med = {k: float(np.median(v)) for k, v in per_round.items()}
    row = {"pix_fmt": pix_fmt, "K": K, "tags_and_timeline": extras, "heat_and_dim": heat_on, "clips": n_clips, "frames_per_clip": T, "frame_hw": [H, W],
           "launches_per_round": launches, "rounds": rounds, "frame_bytes": int(sum(s.numel() for s in src))}
    for k, v in per_round.items():
        row[k + "_ms"] = round(med[k], 4)
        row[k + "_ms_rounds"] = [round(x, 4) for x in v]
    row["multi_over_sequential"] = round(med["multi"] / med["sequential"], 4)
    row["multi_over_copy"] = round(med["multi"] / med["copy"], 4)
    if run_one is not None:
        row["multi_over_overlay"] = round(med["multi"] / med["overlay"], 4)
        row["k1_inside_overlay_spread"] = bool(min(per_round["overlay"]) <= med["multi"] <= max(per_round["overlay"]))
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "overlay_multi_time.json"))
    ap.add_argument("--clips", type=int, default=16)
    ap.add_argument("--frames", type=int, default=100)
    ap.add_argument("--launches", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/overlay_multi_time.py measures on the GPU; none is visible")
    if a.rounds < 3:
        raise SystemExit("at least three alternations: two understate a candidate's own spread")
    dev = torch.device("cuda:0")
    rows = []
    for pix_fmt in ("yuv420p", "rgb24"):
        for K in (1, 4, 8):
            for extras in (False, True):
                for heat_on in (False, True):
                    r = case(pix_fmt, K, extras, heat_on, a.clips, a.frames, a.launches, a.rounds, dev)
                    rows.append(r)
                    print(f"{pix_fmt:8s} K={K} {'tags+timeline' if extras else 'outlines     '} {'heat+dim' if heat_on else '        '}  multi {r['multi_ms']:8.3f} ms  sequential {r['sequential_ms']:8.3f}"
                          f"  copy {r['copy_ms']:8.3f}" + (f"  overlay {r['overlay_ms']:8.3f} (rounds {r['overlay_ms_rounds']})" if K == 1 else "") +
                          f"   multi/sequential {r['multi_over_sequential']:.3f}  multi/copy {r['multi_over_copy']:.3f}", flush=True)
                    torch.cuda.empty_cache()
    out = {"device": torch.cuda.get_device_name(0),
           "method": "device events around every single launch (a candidate of several launches: around the group), 2 warm-up launches, median of `launches_per_round`; "
                     "the candidates alternate within a round; *_ms is the median of the `rounds` round medians",
           "cases": rows}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
