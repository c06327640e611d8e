"""The decoder's query-side cross-attention (functional.CrossQ1Fn, csrc/cross_attn.hip) beyond the resident frame-core kernels:
S > 320 memory rows per frame run on the streaming instances, which walk the frame in chunks of CHUNK rows twice and keep only
per-head statistics between the passes.  Shapes are small (3 to 5 frames); the token counts are the ones at which the code
changes path: just above the resident limit (321, 337), a whole number of chunks and one row more (384, 385), 391 / 553 (608 x 608
and 736 x 736 frames) and 1 080 (800-resolution 16:9 video).  Tolerances are those of tests/test_ops_gpu.py and
tests/test_highres_model_gpu.py."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

CHUNK = 128  # csrc/cross_attn.hip CQ_CHUNK: rows per chunk of the streaming kernels
E, H = 256, 8


def dev():
    return torch.device("cuda:0")


def rel_err(got, ref):
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    return ((got - ref).abs().max() / ref.abs().max().clamp_min(1e-30)).item()


def _cross_attention_fp64(tgt, qpos, mem, pos, W_in, b_in, W_out, b_out, key_pad, F_, S):
    """nn.MultiheadAttention's arithmetic for one query per frame (tests/test_ops_gpu.py _torch_cross_attention) in float64."""
    tgt, qpos, mem, pos, W_in, b_in, W_out, b_out = (x.double() for x in (tgt, qpos, mem, pos, W_in, b_in, W_out, b_out))
    hd = E // H
    q = (tgt + qpos) @ W_in[:E].t() + b_in[:E]
    k = ((mem + pos) @ W_in[E : 2 * E].t() + b_in[E : 2 * E]).view(F_, S, H, hd)
    v = (mem @ W_in[2 * E :].t() + b_in[2 * E :]).view(F_, S, H, hd)
    sc = torch.einsum("fhd,fshd->fhs", q.view(F_, H, hd) / math.sqrt(hd), k)
    sc = sc.masked_fill(key_pad[:, None, :], float("-inf"))
    pr = sc.softmax(-1)
    ctxv = torch.einsum("fhs,fshd->fhd", pr, v).reshape(F_, E)
    return ctxv @ W_out.t() + b_out, pr.mean(1).view(F_, 1, S)


def _check_against_fp64(F_, S, dt, key_pad, seed):
    """Three layers over one shared memory, a loss on the outputs and on the returned weights: the loss and the gradients of the
    query, the memory and every parameter against the float64 reference (test_cross_attention_with_query_side_projections' bounds)."""
    from tubedetr_amd import functional as Fk

    nl = 3
    g = torch.Generator().manual_seed(seed)
    r = lambda *sh, s=1.0: (torch.randn(*sh, generator=g) * s).to(dt).float().to(dev())
    tgt, qpos, mem, pos = r(F_, E), r(F_, E), r(F_ * S, E), r(F_ * S, E)
    params = [[r(3 * E, E, s=1 / 16), r(3 * E, s=0.5), r(E, E, s=1 / 16), r(E, s=0.5)] for _ in range(nl)]
    wo, ww = r(nl, F_, E), r(nl, F_, 1, S)

    def run(fn, leafs_dtype):
        t_, m_ = tgt.clone().requires_grad_(True), mem.clone().requires_grad_(True)
        ps = [[p.clone().requires_grad_(True) for p in layer] for layer in params]
        loss = fn(t_.to(leafs_dtype), m_.to(leafs_dtype), ps)
        loss.backward()
        return loss.detach(), [t_.grad, m_.grad] + [p.grad for layer in ps for p in layer]

    mag = [0.0]

    def ref(t_, m_, ps):
        loss = 0.0
        x = t_
        for l in range(nl):
            o, w = _cross_attention_fp64(x, qpos, m_.view(F_ * S, E), pos, *ps[l], key_pad, F_, S)
            loss = loss + (o * wo[l]).sum() + (w * ww[l]).sum() * 30
            mag[0] += ((o * wo[l]).abs().sum() + (w * ww[l]).abs().sum() * 30).item()
            x = t_ + 0.1 * o
        return loss

    def new(t_, m_, ps):
        loss = 0.0
        anchor = Fk.cross_q1_memory(m_, pos.to(dt))
        x = t_
        for l in range(nl):
            o, w = Fk.multihead_attention_q1(x, anchor, *ps[l], key_pad, F_, S, H, need_weights=True, q_pos=qpos.to(dt))
            assert w.shape == (F_, 1, S)
            loss = loss + (o.float() * wo[l]).sum() + (w * ww[l]).sum() * 30
            x = t_ + (0.1 * o.float()).to(dt)
        return loss

    l_ref, g_ref = run(ref, torch.float64)
    l_new, g_new = run(new, dt)
    tol = 2e-4 if dt == torch.float32 else 3e-2
    names = ["tgt", "mem"] + [f"layer{l}.{n}" for l in range(nl) for n in ("in_proj_weight", "in_proj_bias", "out_proj.weight", "out_proj.bias")]
    errs = {n: rel_err(a, b) for n, a, b in zip(names, g_new, g_ref)}
    print(f"S={S} {dt}: loss err / magnitude {abs(l_new.double() - l_ref).item() / mag[0]:.2e}, worst gradient {max(errs.values()):.2e}")
    assert abs(l_new.double() - l_ref).item() <= (2e-5 if dt == torch.float32 else 2e-3) * mag[0]
    for n, a in zip(names, g_new):
        assert torch.isfinite(a).all(), n
        if n.endswith("in_proj_bias"):  # the key bias shifts every score of a row equally: zero gradient
            assert a[E : 2 * E].abs().max().item() == 0.0
        assert errs[n] < tol, (n, errs[n])


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("F_,S", [(5, 321), (4, 337), (3, 3 * CHUNK), (3, 3 * CHUNK + 1), (3, 553), (3, 1080)])
def test_query_side_cross_attention_above_the_resident_limit_matches_fp64(F_, S, dt):
    g = torch.Generator().manual_seed(900 + S)
    key_pad = (torch.rand(F_, S, generator=g) < 0.2).to(dev())
    key_pad[:, 0] = False
    _check_against_fp64(F_, S, dt, key_pad, 5 + S)


def _chunk_masks(S):
    """Frame 0: every row >= 300 masked (the last chunks see nothing); frame 1: rows 1 .. 299 masked (a fully masked chunk between
    live ones); frame 2: no mask; frame 3: rows < 300 masked (the running maximum is still -inf when the first live row arrives)."""
    kp = torch.zeros(4, S, dtype=torch.bool)
    kp[0, 300:] = True
    kp[1, 1:300] = True
    kp[3, :300] = True
    return kp.to(dev())


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16])
def test_fully_masked_chunks(dt):
    from tubedetr_amd import ops

    F_, S = 4, 553
    key_pad = _chunk_masks(S)
    _check_against_fp64(F_, S, dt, key_pad, 31)
    g = torch.Generator().manual_seed(32)
    r = lambda *sh, s=1.0: (torch.randn(*sh, generator=g) * s).to(dt).to(dev())
    u, mem, pos = r(F_, H * E, s=0.2), r(F_ * S, E), r(F_ * S, E)
    probs, wavg, zext = ops.cross_q1_fwd(u, mem, pos, key_pad, F_, S, H, need_wavg=True)
    probs = probs.view(F_, H, S)
    assert torch.isfinite(probs).all() and torch.isfinite(wavg).all() and torch.isfinite(zext.float()).all()
    assert (probs[key_pad[:, None, :].expand(F_, H, S)] == 0).all()  # exactly zero on masked rows
    assert (probs.sum(-1) - 1).abs().max().item() < 1e-5
    assert wavg.view(F_, S)[key_pad].abs().max().item() == 0.0


@pytest.mark.parametrize("S", [391, 553])
def test_same_dropout_mask_as_the_projected_path_beyond_one_chunk(S):
    """test_cross_attention_query_side_draws_the_same_dropout_mask_as_the_projected_path beyond one chunk: the dropout key stays
    (seed, (f * 8 + h) * S + s), td_mha_fwd's at Lq = 1."""
    from tubedetr_amd import functional as Fk

    F_ = 4
    g = torch.Generator().manual_seed(11 + S)
    r = lambda *sh, s=1.0: (torch.randn(*sh, generator=g) * s).to(dev())
    tgt, mem = r(F_, E), r(F_ * S, E)
    W_in, b_in, W_out, b_out = r(3 * E, E, s=1 / 16), r(3 * E, s=0.5), r(E, E, s=1 / 16), r(E, s=0.5)
    key_pad = (torch.rand(F_, S, generator=g) < 0.2).to(dev())
    key_pad[:, 0] = False
    wo, ww = r(F_, E), r(F_, 1, S)
    res = []
    for which in ("q1", "projected"):
        torch.manual_seed(77)  # both paths draw their dropout seeds from the generator keyed by torch's seed
        Fk._SEED_STATE["torch_seed"] = None
        t_, m_ = tgt.clone().requires_grad_(True), mem.clone().requires_grad_(True)
        ps = [p.clone().requires_grad_(True) for p in (W_in, b_in, W_out, b_out)]
        Fk.set_wgrad_deferral(which != "q1")
        try:
            if which == "q1":
                o, w = Fk.multihead_attention_q1(t_, Fk.cross_q1_memory(m_, None), *ps, key_pad, F_, S, H, need_weights=True, attn_dropout=0.3, training=True)
            else:
                o, w = Fk.multihead_attention(t_, m_, m_, *ps, key_pad, F_, 1, S, H, True, attn_dropout=0.3, training=True)
            ((o * wo).sum() + (w * ww).sum() * 30).backward()
        finally:
            Fk.set_wgrad_deferral(True)
        res.append([o.detach(), w.detach(), t_.grad, m_.grad] + [p.grad for p in ps])
    dropped = (res[0][1] == 0).float().mean().item()
    print(f"S={S}: dropped fraction {dropped:.3f}, weights rel err {rel_err(res[0][1], res[1][1]):.2e}, worst {max(rel_err(a, b) for a, b in zip(res[0], res[1])):.2e}")
    assert dropped < 0.35 and rel_err(res[0][1], res[1][1]) < 1e-4  # same dropped entries
    for a, b in zip(res[0], res[1]):
        assert rel_err(a, b) < 5e-4


@pytest.mark.parametrize("F_,S,nl", [(4, 391, 6), (3, 553, 2)])
def test_deferred_memory_gradient_beyond_one_chunk(F_, S, nl):
    """test_cross_attention_deferred_memory_gradient on the streaming kernels: td_cross_q1_bwd_coef (matrix pipe) + one td_cross_q1_dmem
    against td_cross_q1_bwd's fp32 accumulation (VALU family), dropout and key padding on."""
    from tubedetr_amd import ops

    dt = torch.bfloat16
    g = torch.Generator().manual_seed(100 + S)
    r = lambda *sh, s=1.0: (torch.randn(*sh, generator=g) * s).to(dt).to(dev())
    mem, pos = r(F_ * S, E), r(F_ * S, E)
    key_pad = (torch.rand(F_, S, generator=g) < 0.2).to(dev())
    key_pad[:, 0] = False
    ran = [l for l in range(nl) if not (nl == 6 and l == 4)]  # (layer 4 of the six never runs its backward)
    KP = (16 * nl + 31) // 32 * 32
    coef = torch.zeros((F_ * S, KP), dtype=dt, device=dev())
    dmem_ref, layers, first = torch.empty((F_ * S, E), dtype=torch.float32, device=dev()), [None] * nl, True
    for l in ran:
        u = r(F_, H * E, s=0.2)
        seed = 1234 + l
        probs, _wavg, _zext = ops.cross_q1_fwd(u, mem, pos, key_pad, F_, S, H, need_wavg=True, dropout_p=0.1, seed=seed)
        d_zext = r(F_, H * E + H, s=0.5)
        dwa = (torch.randn(F_, S, generator=g) * 0.3).to(dev())
        du_ref = ops.cross_q1_bwd(u, mem, pos, probs, d_zext, dwa, dmem_ref, not first, F_, S, H, dropout_p=0.1, seed=seed)
        du_new = ops.cross_q1_bwd_coef(u, mem, pos, probs, d_zext, dwa, coef, 16 * l, F_, S, H, dropout_p=0.1, seed=seed)
        print(f"S={S} layer {l}: d_u rel err {rel_err(du_new, du_ref):.2e}")
        assert rel_err(du_new, du_ref) < 1e-2
        layers[l] = (u, d_zext)
        first = False
    dmem = ops.cross_q1_dmem(coef, layers, F_, S, H, E)
    assert dmem.dtype == dt and dmem.shape == (F_ * S, E) and torch.isfinite(dmem.float()).all()
    num = (dmem.float() - dmem_ref).norm(dim=1)
    den = dmem_ref.norm(dim=1).clamp_min(1e-3 * dmem_ref.norm(dim=1).max())
    print(f"S={S}: d_mem rel err {rel_err(dmem, dmem_ref):.2e}, worst row {(num / den).max().item():.2e}")
    assert rel_err(dmem, dmem_ref) < 1e-2
    assert (num / den).max().item() < 2e-2


def test_memory_without_gradient_and_accumulation():
    """S = 391, fp32.  d_mem = NULL (memory.requires_grad = False): the query / parameter gradients are those of the run that does
    differentiate the memory, bit for bit.  accumulate: two layers added into one buffer = the sum of two separate calls."""
    from tubedetr_amd import functional as Fk
    from tubedetr_amd import ops

    F_, S = 4, 391
    g = torch.Generator().manual_seed(9)
    r = lambda *sh, s=1.0: (torch.randn(*sh, generator=g) * s).to(dev())
    tgt, qpos, mem, pos = r(F_, E), r(F_, E), r(F_ * S, E), r(F_ * S, E)
    ps0 = [r(3 * E, E, s=1 / 16), r(3 * E, s=0.5), r(E, E, s=1 / 16), r(E, s=0.5)]
    wo = r(F_, E)
    out = []
    for mem_grad in (True, False):
        t_ = tgt.clone().requires_grad_(True)
        m_ = mem.clone().requires_grad_(mem_grad)
        ps = [p.clone().requires_grad_(True) for p in ps0]
        anchor = Fk.cross_q1_memory(m_, pos)
        x = t_
        loss = 0.0
        for _ in range(2):
            o, _w = Fk.multihead_attention_q1(x, anchor, *ps, None, F_, S, H, need_weights=False, q_pos=qpos)
            loss = loss + (o * wo).sum()
            x = t_ + 0.1 * o
        loss.backward()
        out.append(([t_.grad] + [p.grad for p in ps], m_.grad))
    (g1, mg1), (g0, mg0) = out
    assert mg1 is not None and torch.isfinite(mg1).all() and mg0 is None
    for a, b in zip(g0, g1):
        assert torch.equal(a, b)

    key_pad = (torch.rand(F_, S, generator=g) < 0.2).to(dev())
    key_pad[:, 0] = False
    calls = []
    for l in range(2):
        u, d_zext, dwa = r(F_, H * E, s=0.2), r(F_, H * E + H, s=0.5), r(F_, S, s=0.3)
        probs, _wavg, _zext = ops.cross_q1_fwd(u, mem, pos, key_pad, F_, S, H, need_wavg=True, dropout_p=0.1, seed=50 + l)
        calls.append((u, probs, d_zext, dwa, 50 + l))
    acc = torch.empty((F_ * S, E), dtype=torch.float32, device=dev())
    sep, dus = [], []
    for l, (u, probs, d_zext, dwa, seed) in enumerate(calls):
        du_a = ops.cross_q1_bwd(u, mem, pos, probs, d_zext, dwa, acc, l > 0, F_, S, H, dropout_p=0.1, seed=seed)
        one = torch.empty_like(acc)
        du_s = ops.cross_q1_bwd(u, mem, pos, probs, d_zext, dwa, one, False, F_, S, H, dropout_p=0.1, seed=seed)
        assert torch.equal(du_a, du_s)
        sep.append(one)
    assert rel_err(acc, sep[0] + sep[1]) < 1e-6


def test_streaming_kernels_are_bit_reproducible():
    """The same forward + backward twice at S = 553 in bf16: no atomics, fixed reduction orders - every output is identical."""
    from tubedetr_amd import ops

    F_, S, dt = 4, 553, torch.bfloat16
    g = torch.Generator().manual_seed(77)
    r = lambda *sh, s=1.0: (torch.randn(*sh, generator=g) * s).to(dt).to(dev())
    u, mem, pos, d_zext = r(F_, H * E, s=0.2), r(F_ * S, E), r(F_ * S, E), r(F_, H * E + H, s=0.5)
    dwa = (torch.randn(F_, S, generator=g) * 0.3).to(dev())
    key_pad = (torch.rand(F_, S, generator=g) < 0.2).to(dev())
    key_pad[:, 0] = False
    runs = []
    for _ in range(2):
        probs, wavg, zext = ops.cross_q1_fwd(u, mem, pos, key_pad, F_, S, H, need_wavg=True, dropout_p=0.1, seed=5)
        coef = torch.zeros((F_ * S, 32), dtype=dt, device=dev())
        du_c = ops.cross_q1_bwd_coef(u, mem, pos, probs, d_zext, dwa, coef, 16, F_, S, H, dropout_p=0.1, seed=5)
        dmem = torch.empty((F_ * S, E), dtype=torch.float32, device=dev())
        du_m = ops.cross_q1_bwd(u, mem, pos, probs, d_zext, dwa, dmem, False, F_, S, H, dropout_p=0.1, seed=5)
        runs.append((probs, wavg, zext, coef, du_c, dmem, du_m))
    assert (runs[0][0] == 0).any() and torch.isfinite(runs[0][5]).all()
    for a, b in zip(*runs):
        assert torch.equal(a, b)


def _step(model, criterion, weight_dict, b_dev, params):
    from tubedetr_amd.harness import forward_step

    for p in params:
        p.grad = None
    loss, _, out, _ = forward_step(model, criterion, weight_dict, b_dev)
    loss.backward()
    torch.cuda.synchronize()
    grads = [None if p.grad is None else p.grad.detach().double().flatten().clone() for p in params]
    return loss.item(), out["pred_boxes"].float().clone(), out["pred_sted"].float().clone(), grads


def test_bf16_model_takes_the_query_side_path_at_391_tokens_and_follows_the_projected_path(monkeypatch):
    """608 x 608 frames, S = 19 x 19 + 30 = 391 (test_bf16_model_on_streaming_encoder_attention_follows_probs_path's setup): the decoder
    runs td_cross_q1_fwd at S = 391 by default and not at all under TD_CROSS_Q1=0; the two bf16 steps agree to bf16 rounding and the
    default one stays as close to the exact-fp32 step as the projected one."""
    import tubedetr_amd
    from oracle.tubedetr_oracle import OracleConfig
    from oracle.weights import fill_state, state_spec, synthetic_batch
    from tubedetr_amd import ops
    from tubedetr_amd.harness import FixedTokenizer, batch_to
    from tubedetr_amd.models import build_model

    T, k, L, res, S = 8, 4, 30, 608, 391
    cfg = OracleConfig(stride=k)
    sd = fill_state(state_spec(cfg), 17)
    batch = synthetic_batch(T=T, res=res, k=k, L=L, seed=77, pad_w=40)
    model, criterion, weight_dict = build_model(tubedetr_amd.default_args(stride=k, compute_dtype=torch.bfloat16))
    model.load_state_dict(sd, strict=True)
    model.to(dev()).eval()
    model.transformer.tokenizer = FixedTokenizer(batch["input_ids"], batch["attention_mask"])
    b_dev = batch_to(batch, dev())
    params = [p for p in model.parameters() if p.requires_grad]

    seen = []
    q1_fwd = ops.cross_q1_fwd

    def counting(u, mem, pos, key_pad, F_, S_, *a, **kw):
        seen.append(S_)
        return q1_fwd(u, mem, pos, key_pad, F_, S_, *a, **kw)

    monkeypatch.setattr(ops, "cross_q1_fwd", counting)
    new = _step(model, criterion, weight_dict, b_dev, params)
    assert seen and set(seen) == {S}, sorted(set(seen))
    monkeypatch.setenv("TD_CROSS_Q1", "0")
    n_before = len(seen)
    old = _step(model, criterion, weight_dict, b_dev, params)
    assert len(seen) == n_before  # the A/B run took the projected path
    monkeypatch.delenv("TD_CROSS_Q1")
    model.set_compute_dtype(torch.float32)
    ref = _step(model, criterion, weight_dict, b_dev, params)

    (l_x, b_x, s_x, _), (l_y, b_y, s_y, _) = new, old
    print("loss", l_x, l_y, "boxes", (b_x - b_y).abs().max().item(), "sted", (s_x - s_y).abs().max().item(), "of", s_y.abs().max().item())
    assert abs(l_x - l_y) < 0.02 * abs(l_y), (l_x, l_y)
    assert (b_x - b_y).abs().max().item() < 0.05
    assert (s_x - s_y).abs().max().item() < 0.1 * max(1.0, s_y.abs().max().item())

    def compare(x, y):
        g_x, g_y = x[3], y[3]
        dot = n_x = n_y = 0.0
        for a, b in zip(g_x, g_y):
            assert (a is None) == (b is None)
            if a is None:
                continue
            assert torch.isfinite(a).all()
            dot += (a @ b).item()
            n_x += (a @ a).item()
            n_y += (b @ b).item()
        return dot / (n_x * n_y) ** 0.5, (n_x / n_y) ** 0.5

    cos_ab, nr_ab = compare(new, old)
    cos_new, nr_new = compare(new, ref)
    cos_old, nr_old = compare(old, ref)
    rec = dict(new_vs_old=(cos_ab, nr_ab), new_vs_fp32=(cos_new, nr_new), old_vs_fp32=(cos_old, nr_old))
    print("gradients:", rec)
    assert cos_ab >= 0.97 and abs(nr_ab - 1.0) <= 0.13, rec
    assert cos_new >= cos_old - 0.01, rec
