"""The lean (no-weights) attention core at any token count: the streaming kernels behind td_mha_lean_fwd / _bwd that take
every shape the one-block kernels cannot (Lk > 256, Lq > 448, or 2^32 elements and more), against an fp64 torch reference,
against the probabilities path on the same dropout seed, run-to-run bit-identity, and the 64-bit dropout index."""
import math

import pytest
import torch

TOL = 1.2e-2  # max|err| / max|ref| of a bf16 result (tests/test_ops_gpu.py)
E_H = 8  # heads of TubeDETR's transformer, head dim 32


def dev():
    return torch.device("cuda:0")


def rel_err(got, ref):
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    return ((got - ref).abs().max() / ref.abs().max().clamp_min(1e-30)).item()


def _inputs(B, H, Lq, Lk, use_mask, seed=19):
    g = torch.Generator().manual_seed(seed)
    E = H * 32
    q, k, v, do = (torch.randn(s, generator=g).to(torch.bfloat16) for s in ((B, Lq, E), (B, Lk, E), (B, Lk, E), (B, Lq, E)))
    kpm = None
    if use_mask:
        kpm = torch.rand(B, Lk, generator=g) > 0.8
        kpm[:, 0] = False
    return q, k, v, do, kpm


def _reference(q, k, v, do, kpm, H):
    """fp64 torch on the device: output and the gradients of sum(out * do)."""
    B, Lq, E = q.shape
    hd = E // H
    qr, kr, vr = (t.to(dev(), torch.float64).requires_grad_(True) for t in (q, k, v))
    qh, kh, vh = (t.view(B, -1, H, hd).transpose(1, 2) for t in (qr, kr, vr))
    sc = (qh @ kh.transpose(-1, -2)) / math.sqrt(hd)
    if kpm is not None:
        sc = sc.masked_fill(kpm.to(dev())[:, None, None, :], float("-inf"))
    out = (sc.softmax(-1) @ vh).transpose(1, 2).reshape(B, Lq, E)
    (out * do.to(dev(), torch.float64)).sum().backward()
    return out.detach(), qr.grad, kr.grad, vr.grad


def _lean(q, k, v, do, kpm, H, p=0.0, seed=0):
    from tubedetr_amd import ops

    qd, kd, vd = (t.to(dev()) for t in (q, k, v))
    scale = 1 / math.sqrt(q.shape[2] // H)
    out, stats, kp = ops.mha_lean_fwd(qd, kd, vd, kpm.to(dev()) if kpm is not None else None, H, scale, dropout_p=p, seed=seed)
    grads = ops.mha_lean_bwd(qd, kd, vd, kp, out, do.to(dev()), stats, H, scale, torch.empty_like(qd), torch.empty_like(kd), torch.empty_like(vd),
                             dropout_p=p, seed=seed)
    return out, stats, grads


def test_lean_gate_takes_any_token_count():
    """CPU side of the boundary: the lean gate has no size terms any more (bf16, head dim 32 and 16-byte rows only)."""
    from tubedetr_amd import ops

    for Lq, Lk in ((151, 151), (600, 600), (1, 700), (37, 900), (1038, 1038)):
        q = torch.zeros(2, Lq, 256, dtype=torch.bfloat16)
        k = torch.zeros(2, Lk, 256, dtype=torch.bfloat16)
        assert ops.mha_lean_ok(q, k, k, E_H), (Lq, Lk)
    assert not ops.mha_lean_ok(torch.zeros(2, 600, 256), torch.zeros(2, 600, 256), torch.zeros(2, 600, 256), E_H)  # fp32: probabilities path
    assert not ops.mha_lean_ok(*(torch.zeros(2, 600, 256, dtype=torch.bfloat16),) * 3, 4)  # head dim 64


SHAPES = [(2, 8, 257, 257), (3, 8, 300, 300), (2, 8, 449, 449), (2, 8, 600, 600), (1, 8, 1038, 1038), (4, 8, 1, 700), (2, 8, 37, 900),
          (2, 8, 500, 200)]  # the last: Lk in the one-block range, Lq beyond it


@pytest.mark.gpu
@pytest.mark.parametrize("use_mask", [False, True])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_streaming_lean_matches_fp64_reference(shape, use_mask):
    B, H, Lq, Lk = shape
    q, k, v, do, kpm = _inputs(B, H, Lq, Lk, use_mask)
    out_ref, dq_ref, dk_ref, dv_ref = _reference(q, k, v, do, kpm, H)
    out, stats, (dq, dk, dv) = _lean(q, k, v, do, kpm, H)
    assert stats.shape == (B * H * Lq, 4)
    assert rel_err(out, out_ref) < TOL
    for name, got, ref in (("dq", dq, dq_ref), ("dk", dk, dk_ref), ("dv", dv, dv_ref)):
        assert rel_err(got, ref) < TOL, name
    # the row statistics are the softmax max and 1/sum of the whole row, as the one-block kernels write them
    hd = q.shape[2] // H
    qh = q.double().view(B, Lq, H, hd).transpose(1, 2)
    kh = k.double().view(B, Lk, H, hd).transpose(1, 2)
    sc = (qh @ kh.transpose(-1, -2)) / math.sqrt(hd)
    if kpm is not None:
        sc = sc.masked_fill(kpm[:, None, None, :], float("-inf"))
    mx = sc.amax(-1)
    inv = 1.0 / (sc - mx[..., None]).exp().sum(-1)
    st = stats.double().cpu().view(B, H, Lq, 4)
    assert (st[..., 0] - mx).abs().max().item() < 2e-3 * max(1.0, mx.abs().max().item())
    assert ((st[..., 1] - inv).abs() / inv).max().item() < 2e-2


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(3, 8, 300, 300), (2, 8, 500, 500), (2, 8, 500, 200), (2, 8, 60, 700)], ids=lambda s: "x".join(map(str, s)))
def test_streaming_lean_dropout_mask_is_the_probs_path_mask(shape):
    """Probability dropout on: the streaming kernels (64-bit index) against td_mha_fwd / td_mha_bwd on the same seed (the resident
    kernels' 32-bit index up to Lk = 512, the chunked kernels' 64-bit one at 700).  Below 2^32 elements both draw the same mask,
    so they agree to bf16 rounding; a different mask would differ by the dropout noise itself, which is checked to be far larger."""
    from tubedetr_amd import ops

    B, H, Lq, Lk = shape
    q, k, v, do, kpm = _inputs(B, H, Lq, Lk, True, seed=5)
    p, seed = 0.1, 1234
    out_a, _, ga = _lean(q, k, v, do, kpm, H, p, seed)
    out_0, _, _ = _lean(q, k, v, do, kpm, H)
    qd, kd, vd, dod = (t.to(dev()) for t in (q, k, v, do))
    scale = 1 / math.sqrt(32)
    out_b, probs_b, _ = ops.mha_fwd(qd, kd, vd, kpm.to(dev()), H, scale, dropout_p=p, seed=seed)
    gb = ops.mha_bwd(qd, kd, vd, dod, probs_b, None, H, scale, torch.empty_like(qd), torch.empty_like(kd), torch.empty_like(vd), dropout_p=p, seed=seed)
    assert rel_err(out_a, out_0) > 10 * TOL  # the dropout noise
    assert rel_err(out_a, out_b) < TOL
    for name, a, b in zip(("dq", "dk", "dv"), ga, gb):
        assert rel_err(a, b) < TOL, name


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(2, 8, 600, 600), (4, 8, 1, 700), (2, 8, 37, 900)], ids=lambda s: "x".join(map(str, s)))
def test_streaming_lean_is_bit_reproducible(shape):
    """No float atomics: two runs of forward + backward (dropout on, key padding) are bitwise equal."""
    B, H, Lq, Lk = shape
    q, k, v, do, kpm = _inputs(B, H, Lq, Lk, True, seed=7)
    runs = [_lean(q, k, v, do, kpm, H, 0.1, 99) for _ in range(2)]
    (o1, s1, g1), (o2, s2, g2) = runs
    assert torch.equal(o1, o2) and torch.equal(s1[:, :3], s2[:, :3])  # (column 3 of the statistics is unused, never written)
    for a, b in zip(g1, g2):
        assert torch.equal(a, b)


@pytest.mark.gpu
def test_streaming_lean_dropout_index_beyond_2_32():
    """B = 129, H = 8, Lq = Lk = 2048: B*H*Lq*Lk = 129 * 2^25 elements, so batch elements 0 and 128 are exactly 2^32 apart in
    the flat index.  Given identical inputs, they must draw different masks (a 32-bit index would give them the same one),
    and the keep rate must stay 1 - p on both sides of 2^32.
    Inputs: q = k = 0 (uniform probabilities 1/Lk), v = 1 in channel 0 of every head (output there = kept keys / Lk / (1 - p):
    the keep rate) and random elsewhere (output sensitive to every mask bit)."""
    from tubedetr_amd import ops

    B, H, L, E, p = 129, 8, 2048, 256, 0.1
    g = torch.Generator().manual_seed(3)
    q = torch.zeros(B, L, E, dtype=torch.bfloat16, device=dev())
    v1 = torch.randn(L, H, 32, generator=g)
    v1[:, :, 0] = 1.0
    v = torch.zeros(B, L, E, dtype=torch.bfloat16, device=dev())
    v[0] = v1.reshape(L, E).to(dev(), torch.bfloat16)
    v[128] = v[0]
    v[1:128] = v[0]  # (also below 2^32: more samples of the keep rate)
    out, stats, _ = ops.mha_lean_fwd(q, q, v, None, H, 1 / math.sqrt(32), dropout_p=p, seed=4321)
    torch.cuda.synchronize()
    o = out.float().view(B, L, H, 32)
    assert torch.isfinite(o).all()
    assert not torch.equal(o[0], o[128])
    noise = (o[0, :, :, 1:] - v1[:, :, 1:].to(dev()).mean(0)).abs().mean().item()  # dropout noise around the undropped mean
    assert (o[0, :, :, 1:] - o[128, :, :, 1:]).abs().mean().item() > 0.5 * noise
    keep = o[..., 0].double() * (1 - p)  # kept fraction of each row's keys (P = 1 exactly; bf16(1/(1-p)) is 0.16 % low)
    for part in (keep[:128], keep[128]):
        assert abs(part.mean().item() - (1 - p)) < 0.005 * (1 - p), part.mean().item()


PROBS_SHAPES = [(2, 8, 37, 513), (3, 8, 1, 700), (1, 8, 700, 700), (2, 8, 45, 1100)]  # (1, 8, 700, 700): dK / dV over query chunks too


@pytest.mark.gpu
@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("shape", PROBS_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_probs_path_beyond_512_keys_matches_fp64_reference(shape, dt):
    """td_mha_fwd / td_mha_bwd past the resident kernels (Lk > 512, Lq > 640): the chunked kernels, with the head-averaged
    weights and their gradient (need_wavg / dwavg, as nn.MultiheadAttention returns them) and key padding, against fp64 torch."""
    from tubedetr_amd import ops

    B, H, Lq, Lk = shape
    q, k, v, do, kpm = _inputs(B, H, Lq, Lk, True, seed=23)
    g = torch.Generator().manual_seed(29)
    dw = torch.randn(B, Lq, Lk, generator=g)
    hd = 32
    qr, kr, vr = (t.to(dev(), torch.float64).requires_grad_(True) for t in (q, k, v))
    qh, kh, vh = (t.view(B, -1, H, hd).transpose(1, 2) for t in (qr, kr, vr))
    sc = ((qh @ kh.transpose(-1, -2)) / math.sqrt(hd)).masked_fill(kpm.to(dev())[:, None, None, :], float("-inf"))
    pr = sc.softmax(-1)
    out_ref = (pr @ vh).transpose(1, 2).reshape(B, Lq, H * hd)
    wavg_ref = pr.mean(1)
    ((out_ref * do.to(dev(), torch.float64)).sum() + (wavg_ref * dw.to(dev(), torch.float64)).sum()).backward()
    qd, kd, vd = (t.to(dev(), dt) for t in (q, k, v))
    out, probs, wavg = ops.mha_fwd(qd, kd, vd, kpm.to(dev()), H, 1 / math.sqrt(hd), need_wavg=True)
    tol = 5e-5 if dt == torch.float32 else TOL
    assert rel_err(out, out_ref) < tol
    assert rel_err(probs, pr) < 1e-5 and rel_err(wavg, wavg_ref) < 1e-5  # fp32 probabilities in both dtypes
    dq, dk, dv = ops.mha_bwd(qd, kd, vd, do.to(dev(), dt), probs, dw.to(dev()), H, 1 / math.sqrt(hd), torch.empty_like(qd), torch.empty_like(kd),
                             torch.empty_like(vd))
    for name, got, ref in (("dq", dq, qr.grad), ("dk", dk, kr.grad), ("dv", dv, vr.grad)):
        assert rel_err(got, ref) < tol, name


@pytest.mark.gpu
def test_probs_path_dropout_is_bit_reproducible_and_shares_the_mask():
    """Chunked probabilities kernels with dropout: two runs (output, probabilities, head-averaged weights, gradients) are bitwise
    equal, and the output agrees with the streaming lean kernels' on the same seed (the same mask)."""
    from tubedetr_amd import ops

    B, H, Lq, Lk = 2, 8, 40, 700
    q, k, v, do, kpm = _inputs(B, H, Lq, Lk, True, seed=31)
    qd, kd, vd, dod = (t.to(dev()) for t in (q, k, v, do))
    runs = []
    for _ in range(2):
        out, probs, wavg = ops.mha_fwd(qd, kd, vd, kpm.to(dev()), H, 1 / math.sqrt(32), need_wavg=True, dropout_p=0.1, seed=77)
        grads = ops.mha_bwd(qd, kd, vd, dod, probs, None, H, 1 / math.sqrt(32), torch.empty_like(qd), torch.empty_like(kd), torch.empty_like(vd),
                            dropout_p=0.1, seed=77)
        runs.append((out, probs, wavg) + tuple(grads))
    for a, b in zip(*runs):
        assert torch.equal(a, b)
    out_l, _, _ = _lean(q, k, v, do, kpm, H, 0.1, 77)
    assert rel_err(out_l, runs[0][0]) < TOL
