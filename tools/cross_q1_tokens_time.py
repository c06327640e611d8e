"""Time the decoder's time-aligned cross-attention group (400 frames, one query per frame, E = 256 in 8 heads, bf16, six layers
sharing one memory, dropout 0.1) at the token counts per frame of larger frames, on both of its formulations, in one process:

  q1:    the query-side path - functional.cross_q1_memory + 6 x multihead_attention_q1, the memory gradient deferred to one
         td_cross_q1_dmem (S <= 320: the resident frame-core kernels, beyond: the streaming kernels of csrc/cross_attn.hip)
  proj:  the projected-memory path - functional.cross_kv (keys / values of all layers, [F*S, 1536] each) + 6 x
         multihead_attention_prekv (td_mha_fwd / td_mha_bwd at Lq = 1); what TD_CROSS_Q1=0 runs

For each S: forward + backward time of the whole group (device events around 10 calls after 3 warm-ups; the host launches ~100
small kernels per call, so small S are partly launch-bound on both paths), peak allocated bytes above the inputs, and the bytes each
path moves by its shapes.

  python tools/cross_q1_tokens_time.py [--out profiles/cross_q1_tokens.log] [--frames 400]
"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from tubedetr_amd import functional as Fk  # noqa: E402
from tubedetr_amd.models.transformer import MultiheadAttention  # noqa: E402

E, H, NL, P_DROP = 256, 8, 6, 0.1
TOKENS = (151, 319, 391, 553, 1080)  # 352^2, 544^2, 608^2 (+30 text tokens), 736^2 (+24), 800-resolution 16:9
RESIDENT_MAX = 320  # csrc/cross_attn.hip CQ_RESIDENT_MAX


def timed(fn, iters=10, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def bytes_by_shapes(F, S):
    """HBM bytes of the frame-sized tensors each path reads or writes (bf16 rows, fp32 probabilities); query-sized tensors left out."""
    R = 2.0 * F * S * E      # one [F*S, E] bf16 tensor
    P = 4.0 * F * H * S      # the fp32 probabilities of a layer
    C = 32.0 * F * S         # a layer's sixteen bf16 coefficients per row
    stream = S > RESIDENT_MAX
    fwd = (4 * R if stream else 2 * R) + P                    # mem + pos, twice when streaming; probs written
    bwd = (3 * R + 2 * P if stream else 2 * R + P) + C        # streaming: mem, then mem + pos; probs read per pass
    q1 = NL * (fwd + bwd) + (F * S * 2.0 * 96 + R)            # + td_cross_q1_dmem: coefficient rows read, d(memory) written
    kv = 2 * R + 2 * NL * R                                   # cross_kv forward: mem + pos read, K_all + V_all written
    lay = (2 * R + P) + (2 * R + 2 * P + 2 * P + 2 * R)       # per layer: K, V read, probs written | K, V, probs read, dS written + read, dK, dV written
    kvb = 2 * (2 * NL * R) + 2 * R + R                        # cross_kv backward: dK_all / dV_all read by the input- and the weight-gradient GEMMs, mem + pos, d(memory)
    return q1, kv + NL * lay + kvb


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "cross_q1_tokens.log"))
    ap.add_argument("--frames", type=int, default=400)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "cross_q1_tokens_time.py measures on the MI355X; there is no CPU fallback"
    dev = torch.device("cuda:0")
    F, dt = a.frames, torch.bfloat16
    torch.manual_seed(0)
    layers = [MultiheadAttention(E, H, dropout=P_DROP).to(dev) for _ in range(NL)]
    params = [p for m in layers for p in m.parameters()]
    lines = [f"# decoder cross-attention group: {F} frames x 1 query, E = {E} in {H} heads, bf16, {NL} layers over one memory, dropout {P_DROP}, key padding on 1/8 of the rows",
             f"# {torch.cuda.get_device_name(0)}, {time.strftime('%Y-%m-%d %H:%M')}; forward + backward of the group, device events around 10 calls after 3 warm-ups",
             "# q1 = cross_q1_memory + 6 x multihead_attention_q1 + td_cross_q1_dmem;  proj = cross_kv + 6 x multihead_attention_prekv (TD_CROSS_Q1=0)",
             f"# {'S':>5} {'path':>5} {'f+b ms':>8} {'peak MB':>9} {'GB moved':>9} {'GB/s':>7}"]
    for S in TOKENS:
        g = torch.Generator(device=dev).manual_seed(S)
        rnd = lambda *sh: torch.randn(*sh, device=dev, generator=g).to(dt)
        tgt, qpos, mem, pos = rnd(F, E).requires_grad_(True), rnd(F, E), rnd(F * S, E).requires_grad_(True), rnd(F * S, E)
        go, gw = rnd(F, E), torch.randn(F, 1, S, device=dev, generator=g) * 0.01
        kp = torch.zeros(F, S, dtype=torch.bool, device=dev)
        kp[:, -(S // 8):] = True

        def group(path):
            for p in params + [tgt, mem]:
                p.grad = None
            kv = Fk.cross_q1_memory(mem, pos) if path == "q1" else Fk.cross_kv(mem, pos, layers)
            x, outs = tgt, []
            for i, m in enumerate(layers):
                if path == "q1":
                    x, w = m.run_q1(x, kv, kp, F, S, True, P_DROP, True, q_pos=qpos)
                else:
                    x, w = m.run_prekv(x, kv, i, kp, F, 1, S, True, P_DROP, True, q_pos=qpos)
                outs += [x, w]
            torch.autograd.backward(outs, [go, gw] * NL)

        nbytes = dict(zip(("q1", "proj"), bytes_by_shapes(F, S)))
        res = {}
        for path in ("q1", "proj"):
            group(path)
            torch.cuda.synchronize()
            for p in params + [tgt, mem]:
                p.grad = None
            base = torch.cuda.memory_allocated()
            torch.cuda.reset_peak_memory_stats()
            group(path)
            torch.cuda.synchronize()
            peak = torch.cuda.max_memory_allocated() - base
            assert torch.isfinite(mem.grad.float()).all() and torch.isfinite(tgt.grad.float()).all()
            ms = timed(lambda: group(path))
            res[path] = ms
            lines.append(f"  {S:5d} {path:>5} {ms:8.3f} {peak / 2**20:9.1f} {nbytes[path] / 1e9:9.3f} {nbytes[path] / ms / 1e6:7.0f}")
            print(lines[-1], flush=True)
        lines.append(f"  {S:5d} proj / q1 forward + backward time: {res['proj'] / res['q1']:.2f}x")
        print(lines[-1], flush=True)
        del tgt, qpos, mem, pos, go, gw, kp
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    print(f"wrote {a.out}")


if __name__ == "__main__":
    main()
