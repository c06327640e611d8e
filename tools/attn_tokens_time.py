"""Time the encoder's attention core (400 frames, H = 8, head dim 32, bf16, self-attention over S tokens) at the token counts
of larger frames, on the kernels each S takes now and on the ones it took before:

  new: td_mha_lean_fwd / _bwd - S <= 256: one key block per row (the benchmark clip's kernels), beyond: the streaming kernels
  old: what the encoder ran before the lean path took any S - S <= 256: the same lean kernels; 256 < S <= 512: td_mha_fwd /
       td_mha_bwd (fp32-math VALU kernels that write and read the B*H*S*S fp32 probabilities and a same-sized dS workspace);
       S > 512: refused (no old path)

For each S: forward + backward time (device events around 10 calls after 3 warm-ups; dropout p = 0.1 as in training),
TFLOP/s of 12*B*H*S*S*32 FLOPs (the forward's two products and the backward's four, recomputation not counted), the bytes
each path moves by its shapes, and the bf16 output against an fp64 torch reference on the first frames.

  python tools/attn_tokens_time.py [--out profiles/attn_tokens.log] [--frames 400]
"""
import argparse
import math
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from tubedetr_amd import ops  # noqa: E402

H, HD = 8, 32
E = H * HD
TOKENS = (239, 300, 391, 553, 1038)  # --resolution 352, 384 (+30 text), 416 (+48-token caption / squared batch), 736^2, 800


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "attn_tokens.log"))
    ap.add_argument("--frames", type=int, default=400)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "attn_tokens_time.py measures on the MI355X; there is no CPU fallback"
    dev = torch.device("cuda:0")
    B, scale, p = a.frames, 1 / math.sqrt(HD), 0.1
    lines = [f"# encoder attention core: {B} frames x {H} heads x head dim {HD}, bf16, self-attention over S tokens, dropout {p}",
             f"# {torch.cuda.get_device_name(0)}, {time.strftime('%Y-%m-%d %H:%M')}",
             "# FLOPs = 12*B*H*S^2*32 (fwd QK^T, PV; bwd dP, dS K, dS^T Q, P^T dO); bytes by shapes (bf16 rows, fp32 stats / probs / dS)",
             f"# {'S':>5} {'path':>5} {'fwd ms':>8} {'bwd ms':>8} {'f+b ms':>8} {'TFLOP/s':>8} {'GB moved':>9} {'GB/s':>7}  rel err vs fp64 (out, dq, dk, dv)"]
    ratios = {}
    for S in TOKENS:
        g = torch.Generator(device=dev).manual_seed(S)
        q, k, v, do = (torch.randn(B, S, E, device=dev, generator=g).bfloat16() for _ in range(4))
        kp = torch.zeros(B, S, dtype=torch.bool, device=dev)
        kp[:, -S // 8:] = True  # a padded tail of keys, as in a batch of ragged frames
        dq, dk, dv = torch.empty_like(q), torch.empty_like(k), torch.empty_like(v)
        flops = 12.0 * B * H * S * S * HD
        rows = 2.0 * B * S * E  # bytes of one [B, S, E] bf16 tensor
        paths = {}
        st = {}

        def lean_f():
            st["out"], st["stats"], st["kp"] = ops.mha_lean_fwd(q, k, v, kp, H, scale, dropout_p=p, seed=11)

        def lean_b():
            ops.mha_lean_bwd(q, k, v, st["kp"], st["out"], do, st["stats"], H, scale, dq, dk, dv, dropout_p=p, seed=11)

        stats_b = B * H * S * 16.0
        paths["new"] = (lean_f, lean_b, 4 * rows + stats_b + 8 * rows + 2 * stats_b)
        if 256 < S <= 512:
            so = {}

            def old_f():
                so["out"], so["probs"], _ = ops.mha_fwd(q, k, v, kp, H, scale, dropout_p=p, seed=11)

            def old_b():
                ops.mha_bwd(q, k, v, do, so["probs"], None, H, scale, dq, dk, dv, dropout_p=p, seed=11)

            pr = 4.0 * B * H * S * S
            paths["old"] = (old_f, old_b, 4 * rows + pr + 7 * rows + 4 * pr)  # probs written; bwd: probs read twice, dS written + read
        res = {}
        for name, (f, b_, nbytes) in paths.items():
            tf = timed(f)
            f()
            tb = timed(b_)
            # output check (dropout off) on the first frames against fp64 torch
            n = min(B, 8)
            sl = [t[:n].contiguous() for t in (q, k, v, do)]
            kps = kp[:n].contiguous()
            d3 = [torch.empty_like(sl[0]), torch.empty_like(sl[1]), torch.empty_like(sl[2])]
            if name == "new":
                o, s_, kpu = ops.mha_lean_fwd(sl[0], sl[1], sl[2], kps, H, scale)
                ops.mha_lean_bwd(sl[0], sl[1], sl[2], kpu, o, sl[3], s_, H, scale, *d3)
            else:
                o, pr_, _ = ops.mha_fwd(sl[0], sl[1], sl[2], kps, H, scale)
                ops.mha_bwd(sl[0], sl[1], sl[2], sl[3], pr_, None, H, scale, *d3)
            qr, kr, vr = (t.double().requires_grad_(True) for t in sl[:3])
            qh, kh, vh = (t.view(n, S, H, HD).transpose(1, 2) for t in (qr, kr, vr))
            sc = ((qh @ kh.transpose(-1, -2)) * scale).masked_fill(kps[:, None, None, :], float("-inf"))
            ref = (sc.softmax(-1) @ vh).transpose(1, 2).reshape(n, S, E)
            (ref * sl[3].double()).sum().backward()
            errs = [((x.double() - r).abs().max() / r.abs().max()).item() for x, r in ((o, ref), (d3[0], qr.grad), (d3[1], kr.grad), (d3[2], vr.grad))]
            res[name] = tf + tb
            lines.append(f"  {S:5d} {name:>5} {tf:8.3f} {tb:8.3f} {tf + tb:8.3f} {flops / (tf + tb) / 1e9:8.1f} {nbytes / 1e9:9.3f} "
                         f"{nbytes / (tf + tb) / 1e6:7.0f}  " + " ".join(f"{e:.1e}" for e in errs))
            print(lines[-1], flush=True)
            del o
        if "old" in res:
            ratios[S] = res["old"] / res["new"]
            lines.append(f"  {S:5d} old / new fwd+bwd time: {ratios[S]:.2f}x")
            print(lines[-1], flush=True)
        del q, k, v, do, dq, dk, dv, st
        torch.cuda.empty_cache()
    lines.append("# no old path above S = 512 (td_mha_fwd refused Lk > 512 before ABI 10); at S <= 256 old and new are the same kernels")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    print(f"wrote {a.out}")


if __name__ == "__main__":
    main()
