"""td_grad_norm_clip and td_adamw_ema_step through the C ABI, element by element against tests/optim_ref.py: the float64
restatement of the arithmetic documented in include/tubedetr_hip.h, under ``bound`` = 15 * 2^-24 * (the magnitudes added or
subtracted to form each output).  tests/test_optim_cpu.py proves that every plausible mistake in the step leaves that bound
by a factor of 10 somewhere in these very cases.  Every buffer carries 64 sentinel elements behind ``n`` that must survive.

Worst err/bound measured on an MI355X (printed by each test; the bound is 1.0):
    small layouts, all hyper-parameter sets and steps:  param 0.23, exp_avg 0.11, exp_avg_sq 0.24, ema 0.12
    big layout (8 389 633 elements):                   param 0.23, exp_avg 0.11, exp_avg_sq 0.13, ema 0.13
    three consecutive steps (from 0 and from 999):     param 0.20, exp_avg 0.12, exp_avg_sq 0.23, ema 0.12
    FusedAdamWEMA on the small module, three steps:    param 0.10, exp_avg 0.19, exp_avg_sq 0.40, ema 0.10
(The last line is against torch's float64 AdamW, whose clip coefficient is not rounded to fp32 first.)
"""
import copy

import numpy as np
import pytest
import torch

import optim_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
PAD = 64
SENTINEL = 0x7FC5A5A5  # a NaN payload no kernel arithmetic produces
OUTS = ("param", "exp_avg", "exp_avg_sq", "ema")


def _hip():
    from tubedetr_amd import _hip

    return _hip


def buf(x):
    """Device copy of a 1-d numpy array with PAD sentinel elements behind it; 16-byte aligned."""
    x = np.ascontiguousarray(x)
    assert x.dtype.itemsize == 4
    t = torch.empty(len(x) + PAD, dtype=torch.int32, device=DEV)
    t[: len(x)] = torch.from_numpy(x.view(np.int32)).to(DEV)
    t[len(x):] = SENTINEL
    assert t.data_ptr() % 16 == 0
    return t


def host(t, n, dtype=np.float32):
    return t[:n].cpu().numpy().view(dtype)


def tail_intact(t, n):
    return bool((t[n:] == SENTINEL).all().item())


def seg_array(segs):
    H = _hip()
    arr = (H.OptimSegment * len(segs))()
    for s, (b, e, g, a) in zip(arr, segs):
        s.begin, s.end, s.group, s.active = b, e, g, a
    return arr


class Run:
    """One set of device buffers for a layout; norm() and step() call the two entry points."""

    def __init__(self, n, segs, p, g, m, v, ema, step0=0):
        H = _hip()
        self.n, self.segs, self.arr = n, segs, seg_array(segs)
        self.p, self.g, self.m, self.v = buf(p), buf(g), buf(m), buf(v)
        self.ema = None if ema is None else buf(ema)
        self.lr = buf(np.zeros(4, np.float32))
        self.nc = buf(np.array([-7.0, -7.0], np.float32))
        self.step = buf(np.array([step0], np.int32))
        self.ws_bytes = H.lib().td_grad_norm_ws_bytes()
        self.ws = torch.zeros(self.ws_bytes + 4 * PAD, dtype=torch.uint8, device=DEV)

    def buffers(self):
        return [b for b in (self.p, self.g, self.m, self.v, self.ema, self.lr, self.nc, self.step, self.ws) if b is not None]

    def set_lrs(self, lrs):
        self.lr[:4] = torch.from_numpy(np.asarray(lrs, np.float32).view(np.int32)).to(DEV)

    def norm(self, max_norm, use_step=True, grad_ptr=None, segs=None, n=None, ws_bytes=None):
        H = _hip()
        arr = self.arr if segs is None else seg_array(segs)
        return H.lib().td_grad_norm_clip(self.g.data_ptr() if grad_ptr is None else grad_ptr, self.n if n is None else n, arr, len(arr), max_norm,
                                         self.ws.data_ptr(), self.ws_bytes if ws_bytes is None else ws_bytes, self.nc.data_ptr(),
                                         self.step.data_ptr() if use_step else None, H.stream_ptr())

    def adam(self, hp, use_clip=True, use_ema=True, segs=None, n=None, ptrs=None):
        H = _hip()
        arr = self.arr if segs is None else seg_array(segs)
        a = {"param": self.p.data_ptr(), "grad": self.g.data_ptr(), "exp_avg": self.m.data_ptr(), "exp_avg_sq": self.v.data_ptr(),
             "ema": self.ema.data_ptr() if (use_ema and self.ema is not None) else None}
        a.update(ptrs or {})
        return H.lib().td_adamw_ema_step(a["param"], a["grad"], a["exp_avg"], a["exp_avg_sq"], a["ema"], self.n if n is None else n, arr, len(arr),
                                         self.lr.data_ptr(), self.nc.data_ptr() if use_clip else None, self.step.data_ptr(), hp.b1, hp.b2, hp.eps,
                                         hp.wd, hp.decay, H.stream_ptr())

    def read(self):
        torch.cuda.synchronize()
        out = {"param": host(self.p, self.n), "exp_avg": host(self.m, self.n), "exp_avg_sq": host(self.v, self.n),
               "ema": None if self.ema is None else host(self.ema, self.n)}
        nc = host(self.nc, 2)
        return out, float(nc[0]), np.float32(nc[1]), int(host(self.step, 1, np.int32)[0])

    def intact(self):
        return all(tail_intact(b, self.n) for b in (self.p, self.g, self.m, self.v) + (() if self.ema is None else (self.ema,))) and \
            tail_intact(self.lr, 4) and tail_intact(self.nc, 2) and tail_intact(self.step, 1) and not self.ws[self.ws_bytes:].any().item()


def compare(out, inputs, segs, lrs, clip, step, hp, worst, what):
    """Element-wise check of one step's outputs against the float64 reference under ``bound``; inactive elements of
    param / exp_avg / exp_avg_sq must be bit-identical to the inputs.  Updates ``worst`` (err/bound per output)."""
    p, g, m, v, ema = inputs
    a = (p, g, m, v, ema, segs, lrs, clip, step, hp)
    ref, bnd = R.adamw_ema_ref64(*a), R.bound(*a)
    _, act = R.seg_arrays(len(p), segs)
    for k, x in zip(OUTS[:3], (p, m, v)):
        assert np.array_equal(out[k][~act].view(np.int32), x[~act].view(np.int32)), (what, k, "an inactive element changed")
    for k in OUTS:
        if ref[k] is None:
            continue
        assert np.isfinite(out[k]).all(), (what, k)
        err = np.abs(out[k].astype(np.float64) - ref[k])
        ratio = R.worst_ratio(out[k], ref[k], bnd[k] / R.U)
        worst[k] = max(worst.get(k, 0.0), ratio)
        bad = np.nonzero(~(err <= bnd[k]))[0]
        assert len(bad) == 0, (what, k, "first bad element", int(bad[0]), float(err[bad[0]]), float(bnd[k][bad[0]]), "err/bound", ratio)


def one_step(layout, hp, step, use_ema=True):
    n, segs = R.LAYOUTS[layout]
    inputs = R.make_state(layout, step)
    r = Run(n, segs, *inputs[:4], inputs[4] if use_ema else None, step0=step - 1)
    r.set_lrs(hp.lrs)
    H = _hip()
    H.check(r.norm(hp.max_norm), "td_grad_norm_clip")
    H.check(r.adam(hp), "td_adamw_ema_step")
    out, norm, clip, step_now = r.read()
    assert r.intact(), "a sentinel behind a buffer was overwritten"
    want_norm, want_clip = R.norm_clip_ref64(inputs[1], segs, hp.max_norm)
    assert np.isfinite(norm) and abs(norm - want_norm) <= 1e-6 * want_norm, (norm, want_norm)
    assert abs(float(clip) - want_clip) <= 4 * R.U * want_clip, (clip, want_clip)
    assert step_now == step
    assert np.array_equal(host(r.g, n).view(np.int32), inputs[1].view(np.int32))  # the gradient is read-only
    return out, inputs, segs, clip


@pytest.mark.parametrize("hp_name", list(R.HYPERS))
@pytest.mark.parametrize("layout", R.SMALL_LAYOUTS)
def test_step_matches_float64_reference(layout, hp_name):
    hp = R.HYPERS[hp_name]
    worst = {}
    for step in R.STEPS:
        out, inputs, segs, clip = one_step(layout, hp, step)
        compare(out, inputs, segs, hp.lrs, clip, step, hp, worst, (layout, hp_name, step))
    print(f"{layout} {hp_name}: worst err/bound", {k: round(x, 3) for k, x in worst.items()})


def test_past_the_grid_caps():
    """8192*256*4 + 1025 elements: every workgroup of td_adamw_ema_step's capped grid sweeps twice, the norm kernel's five
    times, the scalar tail holds one element; three segments whose boundaries are no multiple of 4."""
    hp, worst = R.RESOLVING, {}
    out, inputs, segs, clip = one_step("big", hp, 3)
    compare(out, inputs, segs, hp.lrs, clip, 3, hp, worst, "big")
    print("big: worst err/bound", {k: round(x, 3) for k, x in worst.items()})


def test_null_norm_clip_is_coefficient_one_and_null_ema_changes_nothing_else():
    hp = R.RESOLVING
    for layout in ("straddle", "n3", "n5"):
        n, segs = R.LAYOUTS[layout]
        inputs = R.make_state(layout, 3)
        outs = []
        for use_clip, use_ema in ((True, True), (False, True), (True, False)):
            r = Run(n, segs, *inputs, step0=3)
            r.set_lrs(hp.lrs)
            r.nc[:2] = torch.from_numpy(np.array([123.0, 1.0], np.float32).view(np.int32)).to(DEV)  # coefficient exactly 1
            ema_before = host(r.ema, n).copy()
            assert r.adam(hp, use_clip=use_clip, use_ema=use_ema) == 0
            out = r.read()[0]
            assert r.intact()
            if not use_ema:
                assert np.array_equal(out["ema"].view(np.int32), ema_before.view(np.int32))  # a NULL ema: the buffer was not passed
            outs.append(out)
        for k in OUTS:
            assert np.array_equal(outs[0][k].view(np.int32), outs[1][k].view(np.int32)), (layout, k, "norm_clip == NULL")
        for k in OUTS[:3]:
            assert np.array_equal(outs[0][k].view(np.int32), outs[2][k].view(np.int32)), (layout, k, "ema == NULL")
        compare(outs[0], inputs, segs, hp.lrs, np.float32(1), 3, hp, {}, (layout, "clip 1"))


def _norm_of(g, segs, max_norm, use_step=True, step0=5):
    n = len(g)
    z = np.zeros(n, np.float32)
    r = Run(n, segs, z, g, z, z, None, step0=step0)
    assert r.norm(max_norm, use_step=use_step) == 0
    _, norm, clip, step = r.read()
    assert r.intact()
    return norm, clip, step, r


def test_norm_edges():
    n, segs = R.LAYOUTS["straddle"]
    _, act = R.seg_arrays(n, segs)
    rng = np.random.default_rng(3)
    stale = R.make_state("straddle", 3)[1]
    base = rng.standard_normal(n).astype(np.float32)

    def scaled(mag):
        return np.where(act, base * np.float32(mag), stale).astype(np.float32)

    # squares overflow fp32 (1e50) or underflow it (1e-60): the sum is taken in double
    for mag in (1e25, 1e-30):
        g = scaled(mag)
        want, _ = R.norm_clip_ref64(g, segs, 0.1)
        norm, clip, step, _ = _norm_of(g, segs, 0.1)
        assert np.isfinite(norm) and abs(norm - want) <= 1e-6 * want, (mag, norm, want)
        assert abs(float(clip) - min(1.0, float(R.f32(0.1)) / (want + 1e-6))) <= 4 * R.U * float(clip) and step == 6
    # all zeros: norm 0, coefficient exactly 1; the step then only decays param, m = v = 0 and denom = eps
    g0 = scaled(0.0)
    norm, clip, _, r = _norm_of(g0, segs, 0.1)
    assert norm == 0.0 and clip == np.float32(1)
    hp = R.RESOLVING
    p, _, m, v, ema = R.make_state("straddle", 1)
    r = Run(n, segs, p, g0, m, v, ema, step0=0)
    r.set_lrs(hp.lrs)
    assert r.norm(hp.max_norm) == 0 and r.adam(hp) == 0
    out, norm, clip, step = r.read()
    assert norm == 0.0 and clip == np.float32(1) and step == 1 and not out["exp_avg"].any() and not out["exp_avg_sq"].any()
    compare(out, (p, g0, m, v, ema), segs, hp.lrs, clip, 1, hp, {}, "zero gradient")
    group, _ = R.seg_arrays(n, segs)
    decayed = p.astype(np.float64) * (1 - R.f32(hp.lrs)[group] * float(R.f32(hp.wd)))
    assert (np.abs(out["param"][act] - decayed[act]) <= 2 * R.U * np.abs(decayed[act])).all()
    # norm just below / just above max_norm: coefficient exactly 1.0f below, < 1 above; max_norm <= 0 never clips
    g = scaled(1.0)
    want, _ = R.norm_clip_ref64(g, segs, 1.0)
    below, above = np.float32(want * (1 + 1e-5) + 2e-6), np.float32(want * (1 - 1e-5))
    assert _norm_of(g, segs, float(below))[1] == np.float32(1)
    c_above = _norm_of(g, segs, float(above))[1]
    assert c_above < np.float32(1) and abs(float(c_above) - float(above) / (want + 1e-6)) <= 8 * R.U
    for mx in (0.0, -1.0):
        assert _norm_of(g, segs, mx)[1] == np.float32(1)
    # step == NULL: the counter is left alone; with a pointer it advances by exactly one per call
    assert _norm_of(g, segs, 0.1, use_step=False, step0=41)[2] == 41
    norm, clip, step, r = _norm_of(g, segs, 0.1, step0=41)
    assert step == 42 and r.norm(0.1) == 0 and r.read()[3] == 43


@pytest.mark.parametrize("step0", [0, 999])
def test_three_steps_with_a_rate_change(step0):
    """Each step is compared with the reference started from the kernel's own previous outputs (no drift builds up)."""
    hp = R.RESOLVING
    worst = {}
    for layout in ("straddle", "seg32"):
        n, segs = R.LAYOUTS[layout]
        _, act = R.seg_arrays(n, segs)
        p, _, m, v, ema = R.make_state(layout, 1 if step0 == 0 else 1000)
        r = Run(n, segs, p, np.zeros(n, np.float32), m, v, ema, step0=step0)
        lrs = hp.lrs
        for i in range(3):
            if i == 2:
                lrs = tuple(x * f for x, f in zip(hp.lrs, (0.1, 0.5, 0.25, 2.0)))
            r.set_lrs(lrs)
            g = R.make_state(layout, 3, seed=10 + i)[1]
            r.g[:n] = torch.from_numpy(g.view(np.int32)).to(DEV)
            before = r.read()[0]
            assert r.norm(hp.max_norm) == 0 and r.adam(hp) == 0
            out, norm, clip, step = r.read()
            assert step == step0 + i + 1 and r.intact()
            want_norm, want_clip = R.norm_clip_ref64(g, segs, hp.max_norm)
            assert abs(norm - want_norm) <= 1e-6 * want_norm and abs(float(clip) - want_clip) <= 4 * R.U * want_clip
            compare(out, (before["param"], g, before["exp_avg"], before["exp_avg_sq"], before["ema"]), segs, lrs, clip, step, hp, worst,
                    (layout, step0, i))
    print(f"three steps from {step0}: worst err/bound", {k: round(x, 3) for k, x in worst.items()})


# --------------------------------------------------------------------------------------------------- host-side rejections
def _snapshot(r):
    torch.cuda.synchronize()
    return [b.clone() for b in r.buffers()]


def _unchanged(r, snap):
    torch.cuda.synchronize()
    return all(torch.equal(a, b) for a, b in zip(r.buffers(), snap))


BAD_SEGS = {
    "33 segments": (33, [(i, i + 1, 0, 1) for i in range(33)]),
    "gap": (10, [(0, 4, 0, 1), (5, 10, 1, 1)]),
    "overlap": (10, [(0, 6, 0, 1), (5, 10, 1, 1)]),
    "end == begin": (10, [(0, 4, 0, 1), (4, 4, 1, 1), (4, 10, 2, 1)]),
    "end < begin": (10, [(0, 4, 0, 1), (4, 3, 1, 1), (3, 10, 2, 1)]),
    "last end short of n": (10, [(0, 4, 0, 1), (4, 9, 1, 1)]),
    "last end past n": (10, [(0, 4, 0, 1), (4, 11, 1, 1)]),
    "group 4": (10, [(0, 4, 0, 1), (4, 10, 4, 1)]),
    "group -1": (10, [(0, 4, -1, 1), (4, 10, 1, 1)]),
}


def _reject_run(n=40):
    rng = np.random.default_rng(0)
    p, g, m, v, ema = (rng.standard_normal(n).astype(np.float32) for _ in range(5))
    r = Run(n, [(0, n, 0, 1)], p, g, m, np.abs(v), ema, step0=7)
    r.set_lrs(R.RESOLVING.lrs)
    return r


@pytest.mark.parametrize("what", list(BAD_SEGS))
def test_bad_segments_are_rejected_on_the_host(what):
    H = _hip()
    n, segs = BAD_SEGS[what]
    r = _reject_run()
    snap = _snapshot(r)
    assert r.norm(0.1, segs=segs, n=n) == -1 and b"td_grad_norm_clip" in H.lib().td_last_error()
    assert r.adam(R.RESOLVING, segs=segs, n=n) == -1 and b"td_adamw_ema_step" in H.lib().td_last_error()
    assert _unchanged(r, snap)


def test_bad_buffers_are_rejected_on_the_host():
    H = _hip()
    r = _reject_run()
    snap = _snapshot(r)
    assert r.norm(0.1, ws_bytes=r.ws_bytes - 1) == -1 and b"workspace" in H.lib().td_last_error()
    assert r.norm(0.1, grad_ptr=r.g.data_ptr() + 4) == -1 and b"aligned" in H.lib().td_last_error()
    for name, t in (("param", r.p), ("grad", r.g), ("exp_avg", r.m), ("exp_avg_sq", r.v), ("ema", r.ema)):
        assert r.adam(R.RESOLVING, ptrs={name: t.data_ptr() + 4}) == -1 and b"aligned" in H.lib().td_last_error(), name
    assert r.norm(0.1, n=0, segs=[(0, 1, 0, 1)]) == -1 and r.adam(R.RESOLVING, n=0, segs=[(0, 1, 0, 1)]) == -1  # n = 0
    assert _unchanged(r, snap)
    # ... and the same buffers are accepted when nothing is wrong
    assert r.norm(0.1) == 0 and r.adam(R.RESOLVING) == 0 and not _unchanged(r, snap) and r.intact()


# ----------------------------------------------------------------------------------------- FusedAdamWEMA on a small module
ORDER = [("backbone.a", 5), ("text_encoder.pooler.w", 3), ("head.b", 2), ("text_encoder.x", 7), ("backbone.c", 258), ("head.d", 1)]


class _Bag(torch.nn.Module):
    pass


class Tiny(torch.nn.Module):
    """Parameters whose names select all three groups and whose sizes put every later one at a misaligned offset;
    named_parameters() yields them in ``order`` (a model's registration order, which nested modules alone cannot interleave)."""

    def __init__(self, order, seed=0):
        super().__init__()
        self.order = [n for n, _ in order]
        gen = torch.Generator().manual_seed(seed)
        for name, numel in order:
            mod, parts = self, name.split(".")
            for part in parts[:-1]:
                if not hasattr(mod, part):
                    setattr(mod, part, _Bag())
                mod = getattr(mod, part)
            scale = torch.tensor([0.0, 1e-3, 1.0])[torch.arange(numel) % 3]  # exact zeros, ~1e-3 and ~1: see optim_ref.make_state
            mod.register_parameter(parts[-1], torch.nn.Parameter(torch.randn(numel, generator=gen) * scale))

    def named_parameters(self, *args, **kwargs):
        named = dict(super().named_parameters(*args, **kwargs))
        for n in self.order:
            yield n, named[n]


def _ref_update_ema(model, model_ema, decay):  # util/optim.py:8-25
    with torch.no_grad():
        msd = model.state_dict()
        for k, ema_v in model_ema.state_dict().items():
            ema_v.copy_(ema_v * decay + (1.0 - decay) * msd[k].detach())


def _grad_for(name, numel, gen):
    mag = 10.0 ** (torch.rand(numel, generator=gen) * 8 - 8)
    return (torch.randn(numel, generator=gen).sign() * mag).float()


def test_fused_optimizer_on_a_small_module_matches_torch_float64():
    from tubedetr_amd.optim import FusedAdamWEMA

    hp = R.RESOLVING
    w = lambda x: float(R.f32(x))  # the float32 values the kernels receive, widened: torch's float64 AdamW gets the same numbers
    model = Tiny(ORDER).to(DEV)
    ema_model = copy.deepcopy(model)
    with torch.no_grad():
        for p in ema_model.parameters():
            p.add_(0.25)  # "loaded from checkpoint['model_ema']"
    ref, ema_ref = copy.deepcopy(model).cpu().double(), copy.deepcopy(ema_model).cpu().double()
    p_ref, p_new = dict(ref.named_parameters()), dict(model.named_parameters())
    groups = [{"params": [p for n, p in ref.named_parameters() if "backbone" not in n and "text_encoder" not in n], "lr": w(hp.lrs[0])},
              {"params": [p for n, p in ref.named_parameters() if "backbone" in n], "lr": w(hp.lrs[1])},
              {"params": [p for n, p in ref.named_parameters() if "text_encoder" in n], "lr": w(hp.lrs[2])}]
    opt_ref = torch.optim.AdamW(groups, lr=w(hp.lrs[0]), betas=(w(hp.b1), w(hp.b2)), eps=w(hp.eps), weight_decay=w(hp.wd))
    opt = FusedAdamWEMA(model, lr=hp.lrs[0], lr_backbone=hp.lrs[1], text_encoder_lr=hp.lrs[2], weight_decay=hp.wd, betas=(hp.b1, hp.b2), eps=hp.eps,
                        max_norm=hp.max_norm, ema_model=ema_model, ema_decay=hp.decay)
    assert opt.offsets == [0, 5, 8, 10, 17, 275] and opt.group_of == [1, 2, 0, 2, 1, 0] and opt.numel == 276
    segs = [(0, 5, 1, 1), (5, 8, 2, 0), (8, 10, 0, 1), (10, 17, 2, 1), (17, 275, 1, 1), (275, 276, 0, 1)]
    names = [n for n, _ in ORDER]
    e_ref = dict(ema_ref.named_parameters())
    gen = torch.Generator().manual_seed(4)
    flat = lambda named, dt: np.concatenate([named[n].detach().cpu().numpy().astype(dt).ravel() for n in names])
    worst = {}
    for i in range(3):
        lrs = [w(x) for x in hp.lrs[:3]] if i < 2 else [w(hp.lrs[0] * 0.1), w(hp.lrs[1] * 0.5), w(hp.lrs[2] * 0.25)]
        for o in (opt_ref, opt):
            for gr, lr in zip(o.param_groups, lrs):
                gr["lr"] = lr
        gflat = np.full(276, np.nan, np.float32)
        for (n, numel), off in zip(ORDER, opt.offsets):
            if "pooler" in n:  # never reached by the loss
                p_ref[n].grad = p_new[n].grad = None
                continue
            gr = _grad_for(n, numel, gen)
            p_ref[n].grad, p_new[n].grad = gr.double(), gr.to(DEV)
            gflat[off : off + numel] = gr.numpy()
        inputs = (opt.flat_p.cpu().numpy(), gflat, opt.exp_avg.cpu().numpy(), opt.exp_avg_sq.cpu().numpy(), opt.ema.cpu().numpy())
        total = torch.nn.utils.clip_grad_norm_(list(ref.parameters()), w(hp.max_norm))
        opt_ref.step()
        _ref_update_ema(ref, ema_ref, w(hp.decay))
        opt.step()
        torch.cuda.synchronize()
        assert [(s.begin, s.end, s.group, s.active) for s in opt._segs] == segs
        assert abs(opt.norm_clip[0].item() - total.item()) <= 1e-6 * total.item() and opt.step_dev.item() == i + 1
        clip = np.float32(opt.norm_clip[1].item())
        assert abs(float(clip) - min(1.0, w(hp.max_norm) / (total.item() + 1e-6))) <= 4 * R.U and clip < 1
        # torch's own float64 result is the reference; ``bound`` is evaluated at the step's inputs
        a = (*inputs, segs, tuple(lrs) + (0.0,), clip, i + 1, hp)
        bnd = R.bound(*a)
        st = {k: np.zeros(276) for k in ("exp_avg", "exp_avg_sq")}
        for (n, numel), off in zip(ORDER, opt.offsets):
            for k in st:
                st[k][off : off + numel] = opt_ref.state[p_ref[n]][k].numpy() if p_ref[n] in opt_ref.state else 0.0
        want = {"param": flat(p_ref, np.float64), "ema": flat(e_ref, np.float64), **st}
        got = {"param": opt.flat_p.cpu().numpy(), "ema": opt.ema.cpu().numpy(), "exp_avg": opt.exp_avg.cpu().numpy(), "exp_avg_sq": opt.exp_avg_sq.cpu().numpy()}
        mine = R.adamw_ema_ref64(*a)
        for k in OUTS:
            assert (np.abs(mine[k] - want[k]) <= 0.25 * bnd[k] + 1e-300).all(), (k, "optim_ref disagrees with torch")  # the two references agree (torch's clip is not rounded to fp32)
            ratio = R.worst_ratio(got[k], want[k], bnd[k] / R.U)
            worst[k] = max(worst.get(k, 0.0), ratio)
            assert (np.abs(got[k].astype(np.float64) - want[k]) <= bnd[k]).all(), (i, k, ratio)
        # the pooler: parameter and moments untouched, EMA moved as update_ema moves it
        assert np.array_equal(got["param"][5:8], inputs[0][5:8]) and not got["exp_avg"][5:8].any() and not got["exp_avg_sq"][5:8].any()
        assert (np.abs(got["ema"][5:8] - inputs[4][5:8]) > 1e-3).all()
        # next step: the reference starts from the device's state
        with torch.no_grad():
            for (n, numel), off in zip(ORDER, opt.offsets):
                p_ref[n].copy_(torch.from_numpy(got["param"][off : off + numel].astype(np.float64)))
                e_ref[n].copy_(torch.from_numpy(got["ema"][off : off + numel].astype(np.float64)))
                if p_ref[n] in opt_ref.state:
                    for k in st:
                        opt_ref.state[p_ref[n]][k].copy_(torch.from_numpy(got[k][off : off + numel].astype(np.float64)))
    print("small module, three steps: worst err/bound", {k: round(x, 3) for k, x in worst.items()})


def test_a_parameter_that_starts_receiving_a_gradient_rebuilds_the_segments():
    from tubedetr_amd.optim import FusedAdamWEMA

    hp = R.RESOLVING
    model = Tiny(ORDER, seed=1).to(DEV)
    opt = FusedAdamWEMA(model, lr=hp.lrs[0], lr_backbone=hp.lrs[1], text_encoder_lr=hp.lrs[2], weight_decay=hp.wd, eps=hp.eps, max_norm=hp.max_norm)
    gen = torch.Generator().manual_seed(9)
    named = dict(model.named_parameters())
    for i in range(2):
        gflat = np.full(276, np.nan, np.float32)
        for (n, numel), off in zip(ORDER, opt.offsets):
            if "pooler" in n and i == 0:
                named[n].grad = None
                continue
            gr = _grad_for(n, numel, gen)
            named[n].grad = gr.to(DEV)
            gflat[off : off + numel] = gr.numpy()
        inputs = (opt.flat_p.cpu().numpy(), gflat, opt.exp_avg.cpu().numpy(), opt.exp_avg_sq.cpu().numpy(), None)
        opt.step()
        torch.cuda.synchronize()
        segs = [(s.begin, s.end, s.group, s.active) for s in opt._segs]
        assert segs[1] == (5, 8, 2, i), segs
        clip = np.float32(opt.norm_clip[1].item())
        got = {"param": opt.flat_p.cpu().numpy(), "exp_avg": opt.exp_avg.cpu().numpy(), "exp_avg_sq": opt.exp_avg_sq.cpu().numpy(), "ema": None}
        compare(got, inputs, segs, tuple(hp.lrs[:3]) + (0.0,), clip, i + 1, hp, {}, ("late gradient", i))  # (one step counter: t = 2 for the pooler too)
        assert (got["exp_avg"][5:8] != 0).all() == bool(i)


def test_more_than_32_runs_raises():
    from tubedetr_amd.optim import FusedAdamWEMA

    order = [((("backbone." if i % 2 else "head.") + f"p{i}"), 3) for i in range(33)]
    model = Tiny(order).to(DEV)
    opt = FusedAdamWEMA(model)
    before = opt.flat_p.clone()
    for p in model.parameters():
        p.grad = torch.ones_like(p)
    with pytest.raises(RuntimeError, match="33 optimizer segments"):
        opt.step()
    torch.cuda.synchronize()
    assert torch.equal(opt.flat_p, before) and opt.step_dev.item() == 0
