"""Time a training step (bf16, train mode, forward + backward through harness.forward_step, eager) on batches of videos of DIFFERENT
lengths, where every step brings a durations pattern the index-vector cache has never seen - as real VidSTG / HC-STVG data does - with
the pattern's vectors built

  (a) host     by the host builders (Transformer._indices, functional.ReplicaMaps, a dozen pageable host-to-device copies), TD_HOST_MAPS=1
  (b) device   by ONE td_replica_maps launch per pass from a page-locked table copy (functional.ReplicaMaps.from_table), the default

and, as the floor, (c) one fixed pattern repeated, so that every lookup hits the cache.

``--videos`` videos per step at ``--res``, stride ``--stride``, ``--tokens`` tokens; durations drawn per step from random.Random(0), uniform in
[--min-frames, --max-frames].  Pixels are views of one uint8 pool on the device, the slow clip an index list over the fast frames (what
data.ClipPipeline hands over).  A round draws ``--steps`` patterns and runs them once with each builder (the order alternates from round
to round; the harness's and the criterion's own per-pattern caches are emptied in between, so both windows miss alike), then ``--steps``
steps of the fixed pattern.  Device events around each window give ms per step; a host clock around the pattern construction alone (the
two cache-miss sites, Transformer._pattern and TubeDETR._frame_layout) gives the host ms per step spent there - for (a) that includes
waiting for the stream at every pageable copy.  Per variant: the median and the min / max over the rounds.

Both builders see the same patterns inside a round, so the comparison is PAIRED: host minus device ms per step, per round (the spread of a
builder's own window means over the rounds is mostly workload - each round draws other patterns - and says nothing about the builders).
The default builder is whichever has the lower step time by the median paired difference; if the paired differences do not all have one
sign the run cannot tell them apart and the device builder stays the default, because it builds these vectors without a synchronising
copy.  The file records which case holds.

  python tools/ragged_batch_time.py [--out profiles/ragged_batch_time.json] [--rounds 7] [--steps 20] [--head <git head>]
"""
import argparse
import json
import os
import random
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ.setdefault("TD_ALLOW_RANDOM_TEXT_ENCODER", "1")  # no roberta-base files offline: random-init stand-in (timing does not care)
import torch  # noqa: E402


class Tok:
    """Feeds preset token ids to the model."""

    ids = None

    def batch_encode_plus(self, text, padding="longest", return_tensors="pt"):
        from transformers import BatchEncoding

        assert self.ids.shape[0] == len(text)
        be = BatchEncoding({"input_ids": self.ids.clone(), "attention_mask": torch.ones_like(self.ids)})
        be._encodings = [None] * len(text)
        be._td_no_padding = True
        return be


def git_head():
    try:
        return subprocess.run(["git", "rev-parse", "HEAD"], cwd=ROOT, capture_output=True, text=True, check=True).stdout.strip()
    except Exception:  # noqa: BLE001
        return "unknown"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ragged_batch_time.json"))
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=4, help="steps per builder before the first round (patterns of their own)")
    ap.add_argument("--videos", type=int, default=16)
    ap.add_argument("--min-frames", type=int, default=12)
    ap.add_argument("--max-frames", type=int, default=100)
    ap.add_argument("--stride", type=int, default=4)
    ap.add_argument("--res", type=int, default=352)
    ap.add_argument("--tokens", type=int, default=30)
    ap.add_argument("--head", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/ragged_batch_time.py measures on the GPU; none is visible")
    import tubedetr_amd
    from tubedetr_amd import functional as Fk
    from tubedetr_amd import harness
    from tubedetr_amd.models import build_model
    from tubedetr_amd.util.misc import FrameSources

    dev = torch.device("cuda:0")
    B, k, res, L = a.videos, a.stride, a.res, a.tokens
    torch.manual_seed(0)
    model, criterion, weight_dict = build_model(tubedetr_amd.default_args(stride=k, compute_dtype=torch.bfloat16, video_max_len_train=max(200, a.max_frames)))
    model.to(dev).train()
    tok = model.transformer.tokenizer = Tok()
    g = torch.Generator().manual_seed(7)
    tok.ids = torch.randint(3, 50000, (B, L), generator=g)
    tok.ids[:, 0], tok.ids[:, -1] = 0, 2
    pool_frames = B * a.max_frames
    pool = torch.randint(0, 256, (pool_frames, 3, res, res), generator=g, dtype=torch.uint8).to(dev)
    no_pad = torch.zeros((pool_frames, res, res), dtype=torch.bool, device=dev)
    boxes = torch.cat([torch.rand(pool_frames, 2, generator=g) * 0.6 + 0.2, torch.rand(pool_frames, 2, generator=g) * 0.3 + 0.1], 1).to(dev)
    rng = random.Random(0)

    def draw():
        return [rng.randint(a.min_frames, a.max_frames) for _ in range(B)]

    def batch_of(durations):
        """the first sum(durations) pool frames as the videos, back to back; built per step like a loader's collate would"""
        V = sum(durations)
        host, off = [], 0
        for d in durations:
            host += list(range(off, off + d, k))
            off += d
        fast = pool[:V]
        slow = FrameSources([(fast, torch.tensor(host, dtype=torch.int32).pin_memory().to(dev, non_blocking=True))], None, [tuple(host)])
        return {"frames": slow, "frames_mask": no_pad[: len(host)], "frames_fast": fast, "fast_mask": no_pad[:V], "durations": list(durations),
                "target_boxes": boxes[:V], "inter_idx": [[0, d - 1] for d in durations]}

    host_s = [0.0]

    def clocked(fn):
        def wrapper(*args, **kw):
            t0 = time.perf_counter()
            try:
                return fn(*args, **kw)
            finally:
                host_s[0] += time.perf_counter() - t0
        return wrapper

    model.transformer._pattern = clocked(model.transformer._pattern)
    model._frame_layout = clocked(model._frame_layout)
    params = [p for p in model.parameters() if p.requires_grad]

    def step(durations):
        for p in params:
            p.grad = None
        loss, _, _, _ = harness.forward_step(model, criterion, weight_dict, batch_of(durations))
        loss.backward()

    def forget_step_caches():
        for c in (harness._IDX, criterion._pm_cache, criterion._tgt_cache):
            c._d.clear()

    def window(patterns, host_builder):
        """-> (device ms per step, host ms per step inside the pattern construction, frames)"""
        Fk.set_host_maps(host_builder)
        forget_step_caches()
        torch.cuda.synchronize()
        host_s[0] = 0.0
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for d in patterns:
            step(d)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / len(patterns), 1e3 * host_s[0] / len(patterns), sum(map(sum, patterns))

    default_before = Fk.host_maps()
    # warm-up: every kernel's first launch, and the allocator's pools.  The longest batch comes first: the trunk's workspace and the activations
    # are tens of GiB whose size follows the frame count, and blocks cached at the largest size serve every later step, whereas sizes met in
    # growing order leave the pool fragmented around the small long-lived tensors until an allocation fails
    window([[a.max_frames] * B] * 2, False)
    for hb in (True, False):
        window([draw() for _ in range(a.warmup)], hb)
    fixed = draw()
    window([fixed] * 2, False)
    names = ("host", "device", "fixed")
    ms = {n: [] for n in names}
    host_ms = {n: [] for n in names}
    fps = {n: [] for n in names}
    for r in range(a.rounds):
        patterns = [draw() for _ in range(a.steps)]
        order = (("host", True), ("device", False)) if r % 2 == 0 else (("device", False), ("host", True))
        for name, hb in order:
            w = window(patterns, hb)
            ms[name].append(w[0]); host_ms[name].append(w[1]); fps[name].append(w[2] / (w[0] * len(patterns)) * 1e3)
        Fk.set_host_maps(False)
        step(fixed)  # (its pattern may have left the 32-entry caches during the window above)
        w = window([fixed] * a.steps, False)
        ms["fixed"].append(w[0]); host_ms["fixed"].append(w[1]); fps["fixed"].append(w[2] / (w[0] * a.steps) * 1e3)
        print(f"round {r}: " + "  ".join(f"{n} {ms[n][-1]:.2f} ms/step (host {host_ms[n][-1]:.3f} ms, {fps[n][-1]:.0f} frames/s)" for n in names), flush=True)
    Fk.set_host_maps(default_before)

    def stats(v, nd=3):
        return {"median": round(statistics.median(v), nd), "min": round(min(v), nd), "max": round(max(v), nd)}

    rows = {n: {"step_ms": stats(ms[n]), "pattern_build_host_ms_per_step": stats(host_ms[n], 4), "frames_per_s": stats(fps[n], 1)} for n in names}
    paired = [h - d for h, d in zip(ms["host"], ms["device"])]  # same patterns within a round
    diff = statistics.median(paired)
    if min(paired) > 0 or max(paired) < 0:
        default = "device" if diff > 0 else "host"
        verdict = f"every round's paired difference has one sign: the {default} builder has the lower step time and is the default"
    else:
        default = "device"
        verdict = "the paired differences change sign over the rounds: the run cannot tell the builders apart; the device builder stays the default, because it builds these vectors without a synchronising copy"
    out = {"device": torch.cuda.get_device_name(0), "git_head": a.head or git_head(), "dtype": "bf16",
           "mode": "train mode, forward + backward through harness.forward_step, eager",
           "batch": {"videos": B, "frames_uniform_in": [a.min_frames, a.max_frames], "durations_from": "random.Random(0)", "stride": k, "res": res, "tokens": L},
           "fixed_pattern": fixed, "rounds": a.rounds, "steps_per_window": a.steps,
           "timing": "device events around windows of steps, ms per step; host clock around Transformer._pattern + TubeDETR._frame_layout; median over the rounds (min, max alongside)",
           "variants": {"host": "new pattern every step, host builders (TD_HOST_MAPS=1)", "device": "the same patterns, td_replica_maps",
                        "fixed": "one pattern repeated: every lookup hits the cache"},
           "rows": rows, "host_minus_device_step_ms_per_round": [round(x, 3) for x in paired], "host_minus_device_step_ms": stats(paired),
           "default_builder": default, "conclusion": verdict}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote", a.out, "|", verdict)


if __name__ == "__main__":
    main()
