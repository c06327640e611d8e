"""Time grounding P captions on ONE clip three ways (bf16, eval mode, no_grad; encode + decode calls, outputs included):

  (a) expanded      the clip repeated P times in the batch, one caption each: the path without clip_index (trunk, input_proj and the fast
                    projection run once per caption)
  (b) clip_index    one call with clip_index=[0] * P: one trunk pass, the per-clip rows reach the per-pair tensors through index vectors
  (c) kept          TubeDETR.encode_video once, then P separate one-caption calls on the kept VideoFeatures (a server answering questions
                    about a fixed video)

for P in 1, 2, 4, 8 on one bench clip (T = 100 frames, stride 4, resolution 352, 30 tokens).  Device events around each variant; every
shape is warmed up first; a timed window repeats its variant until it holds >= ``--min-ms`` of work; the variants alternate inside each of
``--rounds`` rounds so that drift hits them alike; per variant the median and the min / max over the rounds are recorded (ms per call).
Conditions (recorded, and the exit status): (b) < (a) for every P >= 2, and (b) at P = 1 within
the run-to-run spread (max - min over the rounds) of (a) at P = 1.

  python tools/multi_sentence_time.py [--out profiles/multi_sentence_time.json] [--rounds 7] [--min-ms 200] [--head <git head>]
"""
import argparse
import json
import math
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ.setdefault("TD_ALLOW_RANDOM_TEXT_ENCODER", "1")  # no roberta-base files offline: random-init stand-in (timing does not care)
import torch  # noqa: E402


class Tok:
    """Feeds preset token ids to the model (set ``ids`` before a call)."""

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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "multi_sentence_time.json"))
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--min-ms", type=float, default=200.0, help="device time of one timed window (a variant is called repeatedly to fill it)")
    ap.add_argument("--frames", type=int, default=100)
    ap.add_argument("--stride", type=int, default=4)
    ap.add_argument("--res", type=int, default=352)
    ap.add_argument("--tokens", type=int, default=30)
    ap.add_argument("--pairs", type=int, nargs="+", default=[1, 2, 4, 8])
    ap.add_argument("--head", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/multi_sentence_time.py measures on the GPU; none is visible")
    import tubedetr_amd
    from tubedetr_amd.models import build_model
    from tubedetr_amd.util.misc import FrameSources, NestedTensor

    dev = torch.device("cuda:0")
    T, k, res, L = a.frames, a.stride, a.res, a.tokens
    torch.manual_seed(0)
    model, _, _ = build_model(tubedetr_amd.default_args(stride=k, compute_dtype=torch.bfloat16, video_max_len_train=max(200, T)))
    model.to(dev).eval()
    tok = model.transformer.tokenizer = Tok()
    g = torch.Generator().manual_seed(7)
    clip = torch.randint(0, 256, (T, 3, res, res), generator=g, dtype=torch.uint8).to(dev)
    n_slow = math.ceil(T / k)

    def samples_of(video, clips):
        """slow clip = video[::k] of every clip as an index list over the same pixels (what data.ClipPipeline hands over), fast = all frames"""
        host = tuple(c * T + j for c in range(clips) for j in range(0, T, k))
        slow = FrameSources([(video, torch.tensor(host, dtype=torch.int32, device=dev))], None, [host])
        return (NestedTensor(slow, torch.zeros((clips * n_slow, res, res), dtype=torch.bool, device=dev)),
                NestedTensor(video, torch.zeros((clips * T, res, res), dtype=torch.bool, device=dev)))

    def ids_of(P):
        ids = torch.randint(3, 50000, (P, L), generator=torch.Generator().manual_seed(100 + P))
        ids[:, 0], ids[:, -1] = 0, 2
        return ids

    one = samples_of(clip, 1)

    def variants(P):
        ids = ids_of(P)
        rep = samples_of(clip.repeat(P, 1, 1, 1), P) if P > 1 else one
        caps = ["caption"] * P

        def decode(cache, n):
            return model(None, None, caps[:n], encode_and_save=False, memory_cache=cache)["pred_boxes"]

        def expanded():
            tok.ids = ids
            return decode(model(rep[0], [T] * P, caps, encode_and_save=True, samples_fast=rep[1]), P)

        def clip_index():
            tok.ids = ids
            return decode(model(one[0], [T], caps, encode_and_save=True, samples_fast=one[1], clip_index=[0] * P), P)

        def kept():
            vf = model.encode_video(one[0], [T], one[1])
            out = None
            for p in range(P):
                tok.ids = ids[p : p + 1]
                out = decode(model(None, None, caps[:1], encode_and_save=True, video_features=vf, clip_index=[0]), 1)
            return out

        return {"expanded": expanded, "clip_index": clip_index, "kept": kept}

    def timed(fn, calls=1):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(calls):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / calls

    rows = []
    with torch.no_grad():
        for P in a.pairs:
            fns = variants(P)
            for fn in fns.values():  # warm-up: every shape of the timed window, twice
                fn()
                fn()
            torch.cuda.synchronize()
            calls = {name: max(1, math.ceil(a.min_ms / timed(fn))) for name, fn in fns.items()}  # a timed window holds >= --min-ms of work
            ms = {name: [] for name in fns}
            for _ in range(a.rounds):
                for name, fn in fns.items():
                    ms[name].append(timed(fn, calls[name]))
            row = {"P": P, "calls_per_window": calls}
            for name, v in ms.items():
                row[name + "_ms"] = round(statistics.median(v), 3)
                row[name + "_ms_min_max"] = [round(min(v), 3), round(max(v), 3)]
            rows.append(row)
            print(f"P={P}: " + "  ".join(f"{n} {row[n + '_ms']:.2f} ms [{row[n + '_ms_min_max'][0]:.2f}, {row[n + '_ms_min_max'][1]:.2f}]" for n in fns), flush=True)
    cond = {}
    for row in rows:
        if row["P"] >= 2:
            cond[f"clip_index_faster_than_expanded_P{row['P']}"] = row["clip_index_ms"] < row["expanded_ms"]
        elif row["P"] == 1:
            lo, hi = row["expanded_ms_min_max"]
            cond["clip_index_within_spread_of_expanded_P1"] = abs(row["clip_index_ms"] - row["expanded_ms"]) <= hi - lo
    out = {"device": torch.cuda.get_device_name(0), "git_head": a.head or git_head(), "clip": {"frames": T, "stride": k, "res": res, "tokens": L},
           "dtype": "bf16", "mode": "eval, no_grad, encode + decode calls", "rounds": a.rounds, "timing": f"device events around windows of >= {a.min_ms:g} ms, ms per call; median over the rounds (min, max alongside)",
           "rows": rows, "conditions": cond}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote", a.out, cond)
    if not all(cond.values()):
        raise SystemExit("a condition of the comparison is not met: " + ", ".join(k_ for k_, v in cond.items() if not v))


if __name__ == "__main__":
    main()
