"""td_grad_norm_clip_guarded and td_adamw_ema_step_guarded through the C ABI, and FusedAdamWEMA(skip_nonfinite=True): the
cases of tests/optim_guard_ref.py on the kernels.  tests/test_optim_guard_cpu.py proves that every plausible mistake in the
guard's rules changes the outcome of one of these cases.  What is bit-exact is compared bit for bit: the guarded pair against
the unguarded pair on a finite buffer, and every buffer of a skipped step against its state before.  Every buffer - the guard
block and the workspace included - carries 64 sentinel elements behind its end that must survive."""
import copy
import functools

import numpy as np
import pytest
import torch

import optim_guard_ref as G
import optim_ref as R
from test_optim_kernels_gpu import DEV, OUTS, PAD, buf, compare, host, seg_array, tail_intact

pytestmark = pytest.mark.gpu


def _hip():
    from tubedetr_amd import _hip

    return _hip


def bits(x):
    return np.ascontiguousarray(x).view(np.int32)


class GRun:
    """One set of device buffers for a layout, with a guard block of ``history`` records; the guarded and the unguarded entry
    points run on the same buffers (the workspace has the guarded size, which the unguarded call accepts)."""

    def __init__(self, n, segs, p, g, m, v, ema, step0=0, history=8):
        H = _hip()
        L = H.lib()
        self.n, self.segs, self.arr, self.history = n, segs, seg_array(segs), history
        self.p, self.g, self.m, self.v = buf(p), buf(g), buf(m), buf(v)
        self.ema = None if ema is None else buf(ema)
        self.lr = buf(np.zeros(4, np.float32))
        self.nc = buf(np.array([-7.0, -7.0], np.float32))
        self.step = buf(np.array([step0], np.int32))
        self.loss = buf(np.array([-3.0], np.float32))
        self.guard_ints = L.td_guard_bytes(history) // 4
        assert self.guard_ints == 4 + 10 * history
        self.guard = buf(np.zeros(self.guard_ints, np.int32))  # zero-filled once by the caller
        self.ws_bytes = L.td_grad_norm_guard_ws_bytes()
        self.ws = torch.zeros(self.ws_bytes + 4 * PAD, dtype=torch.uint8, device=DEV)

    def state(self):
        return [b for b in (self.p, self.m, self.v, self.ema, self.step) if b is not None]

    def set_lrs(self, lrs):
        self.lr[:4] = torch.from_numpy(np.asarray(lrs, np.float32).view(np.int32)).to(DEV)

    def set_grad(self, g):
        self.g[: self.n] = torch.from_numpy(bits(g)).to(DEV)

    def set_loss(self, x):
        self.loss[:1] = torch.from_numpy(bits(np.array([x], np.float32))).to(DEV)

    def norm(self, max_norm, loss=None, write_loss=True):
        """The guarded norm; ``loss``: None -> a NULL pointer, a float -> the device scalar is handed over (and written first,
        unless ``write_loss`` is False)."""
        H = _hip()
        if loss is not None and write_loss:
            self.set_loss(loss)
        return H.lib().td_grad_norm_clip_guarded(self.g.data_ptr(), self.n, self.arr, len(self.arr), max_norm, self.ws.data_ptr(), self.ws_bytes,
                                                 self.nc.data_ptr(), self.step.data_ptr(), None if loss is None else self.loss.data_ptr(),
                                                 self.guard.data_ptr(), self.history, H.stream_ptr())

    def adam(self, hp):
        H = _hip()
        return H.lib().td_adamw_ema_step_guarded(self.p.data_ptr(), self.g.data_ptr(), self.m.data_ptr(), self.v.data_ptr(),
                                                 None if self.ema is None else self.ema.data_ptr(), self.n, self.arr, len(self.arr), self.lr.data_ptr(),
                                                 self.nc.data_ptr(), self.step.data_ptr(), hp.b1, hp.b2, hp.eps, hp.wd, hp.decay, self.guard.data_ptr(),
                                                 H.stream_ptr())

    def norm_unguarded(self, max_norm):
        H = _hip()
        return H.lib().td_grad_norm_clip(self.g.data_ptr(), self.n, self.arr, len(self.arr), max_norm, self.ws.data_ptr(), self.ws_bytes,
                                         self.nc.data_ptr(), self.step.data_ptr(), H.stream_ptr())

    def adam_unguarded(self, hp):
        H = _hip()
        return H.lib().td_adamw_ema_step(self.p.data_ptr(), self.g.data_ptr(), self.m.data_ptr(), self.v.data_ptr(),
                                         None if self.ema is None else self.ema.data_ptr(), self.n, self.arr, len(self.arr), self.lr.data_ptr(),
                                         self.nc.data_ptr(), self.step.data_ptr(), hp.b1, hp.b2, hp.eps, hp.wd, hp.decay, H.stream_ptr())

    def attempt(self, g, loss, hp):
        self.set_grad(g)
        assert self.norm(hp.max_norm, loss) == 0 and self.adam(hp) == 0

    def read(self):
        torch.cuda.synchronize()
        out = {"param": host(self.p, self.n), "exp_avg": host(self.m, self.n), "exp_avg_sq": host(self.v, self.n),
               "ema": None if self.ema is None else host(self.ema, self.n)}
        return out, host(self.nc, 2), int(host(self.step, 1, np.int32)[0])

    def header(self):
        """-> (attempts, skipped, consecutive_skipped, applied_now)."""
        torch.cuda.synchronize()
        return tuple(int(x) for x in host(self.guard, 4, np.int32))

    def ring(self):
        """The ring as it lies in memory -> one record dict per slot (a slot never written is all zeros: attempt 0)."""
        H = _hip()
        torch.cuda.synchronize()
        raw = host(self.guard, self.guard_ints, np.int32)[4:].tobytes()
        recs = (H.StepRecord * self.history).from_buffer_copy(raw) if self.history else ()
        return [{"attempt": r.attempt, "step": r.step, "applied": r.applied, "norm": r.norm, "clip": r.clip, "loss": r.loss,
                 "group_norm": list(r.group_norm)} for r in recs]

    def intact(self):
        return all(tail_intact(b, self.n) for b in (self.p, self.g, self.m, self.v) + (() if self.ema is None else (self.ema,))) and \
            tail_intact(self.lr, 4) and tail_intact(self.nc, 2) and tail_intact(self.step, 1) and tail_intact(self.loss, 1) and \
            tail_intact(self.guard, self.guard_ints) and not self.ws[self.ws_bytes:].any().item()


def same_bits(a, b, what):
    for k in OUTS:
        if a[k] is None:
            assert b[k] is None
            continue
        assert np.array_equal(bits(a[k]), bits(b[k])), (what, k)


def check_ring(got_ring, want_ring, what):
    assert len(got_ring) == len(want_ring)
    for i, (got, want) in enumerate(zip(got_ring, want_ring)):
        if want is None:
            assert got["attempt"] == 0 and got["step"] == 0 and got["norm"] == 0, (what, i, "a slot that no attempt reached was written")
            continue
        assert G.record_mismatch(got, want) is None, (what, i, G.record_mismatch(got, want), got, want)


# ------------------------------------------------------------------------------------------------------ 1. finite buffers
@pytest.mark.parametrize("hp_name", list(R.HYPERS))
@pytest.mark.parametrize("layout", R.SMALL_LAYOUTS)
def test_finite_buffer_is_bit_identical_to_the_unguarded_pair(layout, hp_name):
    """make_state plants NaN / Inf in the inactive slots, so this also pins that inactive slots do not count."""
    hp = R.HYPERS[hp_name]
    n, segs = R.LAYOUTS[layout]
    for step in R.STEPS:
        p, g, m, v, ema = R.make_state(layout, step)
        a, b = (GRun(n, segs, p, g, m, v, ema, step0=step - 1, history=4) for _ in range(2))
        for r in (a, b):
            r.set_lrs(hp.lrs)
        assert a.norm_unguarded(hp.max_norm) == 0 and a.adam_unguarded(hp) == 0
        assert b.norm(hp.max_norm) == 0 and b.adam(hp) == 0
        (out_a, nc_a, step_a), (out_b, nc_b, step_b) = a.read(), b.read()
        what = (layout, hp_name, step)
        assert np.array_equal(bits(nc_a), bits(nc_b)) and np.isfinite(nc_b).all() and step_a == step_b == step, what
        same_bits(out_a, out_b, what)
        assert not np.array_equal(bits(out_b["ema"]), bits(ema)), what  # (the step did run)
        assert a.intact() and b.intact(), what
        assert b.header() == (1, 0, 0, 1), what
        assert a.header() == (0, 0, 0, 0), "the unguarded pair touched a guard block"
        want = G.run(segs, (p, m, v, ema), [(g, None)], hp.lrs, hp, step0=step - 1, history=4)
        ring = b.ring()
        check_ring(ring, want["ring"], what)
        assert bits(np.float32(ring[0]["norm"])) == bits(nc_b[0]) and bits(np.float32(ring[0]["clip"])) == bits(nc_b[1]), what


# --------------------------------------------------------------------------------------------------- 2. one bad element
def _expect_skipped(r, before, what, attempts=1):
    """All four buffers and the step counter bit-unchanged, sentinels intact, coefficient 0, header (attempts, k, k, 0)."""
    torch.cuda.synchronize()
    assert all(torch.equal(x, y) for x, y in zip(r.state(), before)), (what, "a buffer or the step counter changed on a skipped step")
    assert r.intact(), what
    nc = host(r.nc, 2)
    assert not np.isfinite(nc[0]) and bits(nc[1]) == bits(np.float32(0)), (what, nc)
    assert r.header() == (attempts, attempts, attempts, 0), (what, r.header())


@pytest.mark.parametrize("value", list(G.BAD_VALUES))
@pytest.mark.parametrize("layout,index", G.BAD_POSITIONS_SMALL)
def test_one_bad_element_skips_the_step(layout, index, value):
    hp = R.RESOLVING
    n, segs = R.LAYOUTS[layout]
    p, _, m, v, ema = R.make_state(layout, 3)
    g = G.bad_gradient(layout, index, G.BAD_VALUES[value])
    r = GRun(n, segs, p, g, m, v, ema, step0=2, history=4)
    r.set_lrs(hp.lrs)
    before = [x.clone() for x in r.state()]
    assert r.norm(hp.max_norm) == 0 and r.adam(hp) == 0
    _expect_skipped(r, before, (layout, index, value))
    want = G.run(segs, (p, m, v, ema), [(g, None)], hp.lrs, hp, step0=2, history=4)
    assert (want["skipped"], want["step"]) == (1, 2)
    check_ring(r.ring(), want["ring"], (layout, index, value))


@functools.lru_cache(maxsize=1)
def _big_state():
    return R.make_state("big", 3)


def test_big_layout_bad_elements_and_group_norms():
    """The one use of the 8 389 633-element layout: a bad value in its last element (the scalar tail, workgroup 0) and in an
    element that workgroup 5 sums; then a finite attempt whose norm must be td_grad_norm_clip's bit for bit and whose group
    norms - summed over 2048 workgroups' partials - must be within one fp32 ulp of the float64 reference."""
    hp = R.RESOLVING
    n, segs = R.LAYOUTS["big"]
    p, g, m, v, ema = _big_state()
    r = GRun(n, segs, p, g, m, v, ema, step0=2, history=8)
    r.set_lrs(hp.lrs)
    before = [x.clone() for x in r.state()]
    attempts = 0
    for index in G.big_positions():
        for name, value in G.BAD_VALUES.items():
            keep = r.g[index].clone()
            r.g[index] = int(bits(np.array([value], np.float32))[0])
            assert r.norm(hp.max_norm) == 0 and r.adam(hp) == 0
            attempts += 1
            _expect_skipped(r, before, ("big", index, name), attempts)
            r.g[index] = keep
    assert r.norm_unguarded(hp.max_norm) == 0
    _, nc_u, step_u = r.read()
    nc_u = nc_u.copy()
    assert step_u == 3
    r.step[:1] = 2
    assert r.norm(hp.max_norm) == 0
    _, nc_g, step_g = r.read()
    assert np.array_equal(bits(nc_u), bits(nc_g)) and step_g == 3 and r.header() == (7, 6, 0, 1) and r.intact()
    total, group_norm = G.norms64(g, segs)
    rec = r.ring()[6]
    want = {"attempt": 7, "step": 3, "applied": 1, "norm": total, "clip": min(1.0, float(R.f32(hp.max_norm)) / (total + float(R.f32(1e-6)))),
            "loss": float("nan"), "group_norm": group_norm}
    assert G.record_mismatch(rec, want) is None, (G.record_mismatch(rec, want), rec, want)
    assert group_norm[0] == 0 and rec["group_norm"][0] == 0 and group_norm[1] > 0 and group_norm[3] > 0  # (group 2 is inactive here: 0 too)


# -------------------------------------------------------------------------------------------------- 3. fp32 norm overflow
def test_finite_elements_whose_fp32_norm_overflows_are_skipped():
    hp = R.RESOLVING
    n, segs = R.LAYOUTS["straddle"]
    p, _, m, v, ema = R.make_state("straddle", 3)
    g = G.overflow_gradient()
    _, act = R.seg_arrays(n, segs)
    assert np.isfinite(g[act]).all() and np.isfinite(G.norms64(g, segs)[0])
    r = GRun(n, segs, p, g, m, v, ema, step0=2, history=4)
    r.set_lrs(hp.lrs)
    before = [x.clone() for x in r.state()]
    assert r.norm(hp.max_norm) == 0 and r.adam(hp) == 0
    _expect_skipped(r, before, "overflow")
    assert host(r.nc, 2)[0] == np.float32(np.inf)
    check_ring(r.ring(), G.run(segs, (p, m, v, ema), [(g, None)], hp.lrs, hp, step0=2, history=4)["ring"], "overflow")


# ------------------------------------------------------------------------------ 4. applied, skipped, skipped, applied
def test_sequence_applied_skipped_skipped_applied():
    hp = R.RESOLVING
    layout = "straddle"
    n, segs = R.LAYOUTS[layout]
    p, _, m, v, ema = R.make_state(layout, 1)
    attempts = G.sequence_attempts(layout)
    r = GRun(n, segs, p, attempts[0][0], m, v, ema, step0=0, history=8)
    u = GRun(n, segs, p, attempts[0][0], m, v, ema, step0=0, history=0)  # the unguarded pair sees the two finite gradients only
    for x in (r, u):
        x.set_lrs(hp.lrs)
    headers = []
    for i, (g, loss) in enumerate(attempts):
        prev, _, _ = r.read()
        prev = {k: x.copy() for k, x in prev.items()}
        r.attempt(g, loss, hp)
        out, nc, step = r.read()
        headers.append(r.header())
        if i in (0, 3):
            u.set_grad(g)
            assert u.norm_unguarded(hp.max_norm) == 0 and u.adam_unguarded(hp) == 0
            out_u, nc_u, step_u = u.read()
            same_bits(out, out_u, ("attempt", i + 1))
            assert np.array_equal(bits(nc), bits(nc_u)) and step == step_u == (1 if i == 0 else 2)
            # ... and equals the reference AT THAT VALUE of the step counter, from the state the kernel itself left before
            compare(out, (prev["param"], g, prev["exp_avg"], prev["exp_avg_sq"], prev["ema"]), segs, hp.lrs, nc[1], step, hp, {}, ("attempt", i + 1))
        else:
            same_bits(out, prev, ("attempt", i + 1))
            assert step == 1
    assert headers == [(1, 0, 0, 1), (2, 1, 1, 0), (3, 2, 2, 0), (4, 2, 0, 1)]
    assert r.intact() and u.intact()
    want = G.run(segs, (p, m, v, ema), attempts, hp.lrs, hp, step0=0, history=8)
    assert (want["attempts"], want["skipped"], want["consecutive_skipped"], want["step"]) == (4, 2, 0, 2)
    ring = r.ring()
    check_ring(ring, want["ring"], "sequence")
    assert ring[0]["loss"] == 2.5 and np.isnan(ring[1]["loss"]) and np.isnan(ring[2]["loss"]) and ring[3]["loss"] == float("inf")
    assert [x["applied"] for x in ring[:4]] == [1, 0, 0, 1] and [x["step"] for x in ring[:4]] == [1, 1, 1, 2]


# ------------------------------------------------------------------------------------------------------------ 5. the ring
def test_ring_wraps_and_history_zero_writes_nothing_past_the_header():
    hp = R.RESOLVING
    layout = "n5"
    n, segs = R.LAYOUTS[layout]
    p, _, m, v, ema = R.make_state(layout, 1)
    attempts = G.wrap_attempts(layout)
    want = G.run(segs, (p, m, v, ema), attempts, hp.lrs, hp, step0=0, history=4)
    for history in (4, 0):
        r = GRun(n, segs, p, attempts[0][0], m, v, ema, step0=0, history=history)
        r.set_lrs(hp.lrs)
        for g, loss in attempts:
            r.attempt(g, loss, hp)
        _, _, step = r.read()
        assert r.header() == (6, 2, 0, 1) and step == 4 == want["step"]
        assert r.intact(), "history = %d: something was written past the guard block" % history  # history 0: the block IS the header
        if history:
            ring = r.ring()
            assert [x["attempt"] for x in ring] == [5, 6, 3, 4]
            check_ring(ring, want["ring"], "wrap")
        else:
            assert r.guard_ints == 4 and r.ring() == []


# --------------------------------------------------------------------------------------------------------- 6. graph capture
def test_captured_pair_replays_like_the_eager_sequence():
    """One linear graph (three kernel nodes, no forks) captured on a side stream and replayed three times over a gradient
    buffer rewritten in between: finite, NaN, finite.  Nothing in the pair reads from the host, so the replay decides anew."""
    hp = R.RESOLVING
    layout = "seg32"
    n, segs = R.LAYOUTS[layout]
    p, _, m, v, ema = R.make_state(layout, 1)
    grads = [R.make_state(layout, 3, seed=41)[1], G.bad_gradient(layout, G.first_active(layout), G.BAD_VALUES["nan"]), R.make_state(layout, 3, seed=43)[1]]
    losses = [0.75, float("nan"), 1.25]
    eager, graphed = (GRun(n, segs, p, grads[0], m, v, ema, step0=0, history=8) for _ in range(2))
    for r in (eager, graphed):
        r.set_lrs(hp.lrs)
        r.set_loss(0.0)
    for g, loss in zip(grads, losses):
        eager.attempt(g, loss, hp)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        rc1 = graphed.norm(hp.max_norm, loss=0.0, write_loss=False)  # the loss POINTER is captured; the scalar is rewritten between replays
        rc2 = graphed.adam(hp)
    assert rc1 == 0 and rc2 == 0
    torch.cuda.synchronize()
    assert graphed.header() == (0, 0, 0, 0), "capturing must not run the kernels"
    for g, loss in zip(grads, losses):
        graphed.set_grad(g)
        graphed.set_loss(loss)
        graph.replay()
    (out_e, nc_e, step_e), (out_g, nc_g, step_g) = eager.read(), graphed.read()
    same_bits(out_e, out_g, "graph")
    assert np.array_equal(bits(nc_e), bits(nc_g)) and step_e == step_g == 2
    assert eager.header() == graphed.header() == (3, 1, 0, 1)
    assert torch.equal(eager.guard, graphed.guard), "the guard blocks (counters and records) differ"
    assert eager.intact() and graphed.intact()


# ------------------------------------------------------------------------------- 7. FusedAdamWEMA(skip_nonfinite=True)
SMALL_ORDER = [("backbone.a", 5), ("text_encoder.pooler.w", 3), ("head.b", 2), ("text_encoder.x", 7), ("backbone.c", 258), ("head.d", 1)]


class _Bag(torch.nn.Module):
    pass


class Small(torch.nn.Module):
    """Parameters whose names select all three groups, at misaligned offsets, yielded by named_parameters() in ``order``;
    the pooler never receives a gradient."""

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
            mod.register_parameter(parts[-1], torch.nn.Parameter(torch.randn(numel, generator=gen)))

    def named_parameters(self, *args, **kwargs):
        named = dict(super().named_parameters(*args, **kwargs))
        for n in self.order:
            yield n, named[n]


def _set_grads(model, seed, nan_in=None):
    gen = torch.Generator().manual_seed(seed)
    for name, p in model.named_parameters():
        if "pooler" in name:
            p.grad = None
            continue
        g = torch.randn(p.numel(), generator=gen) * 0.1
        if name == nan_in:
            g[p.numel() // 2] = float("nan")
        p.grad = g.to(DEV)


def _make_opt(model, ema_model, **kw):
    from tubedetr_amd.optim import FusedAdamWEMA

    hp = R.RESOLVING
    return FusedAdamWEMA(model, lr=hp.lrs[0], lr_backbone=hp.lrs[1], text_encoder_lr=hp.lrs[2], weight_decay=hp.wd, betas=(hp.b1, hp.b2), eps=hp.eps,
                         max_norm=hp.max_norm, ema_model=ema_model, ema_decay=hp.decay, **kw)


def _same_snapshot(a, b):
    return repr(a) == repr(b)  # (nan prints as nan: the dicts hold ints, bools, floats and lists of them)


class _Spy:
    def __init__(self, lib):
        self._lib, self.calls = lib, []

    def __getattr__(self, name):
        self.calls.append(name)
        return getattr(self._lib, name)


def test_fused_optimizer_skips_a_nan_step_and_reports_it(monkeypatch):
    from tubedetr_amd.optim import NonFiniteStepError

    H = _hip()
    model = Small(SMALL_ORDER).to(DEV)
    ema_model = copy.deepcopy(model)
    with torch.no_grad():
        for p in ema_model.parameters():
            p.add_(0.25)
    opt = _make_opt(model, ema_model, skip_nonfinite=True, history=8)
    assert opt._guard is not None and opt._guard.numel() == 16 + 40 * 8 and opt._ws.numel() == H.lib().td_grad_norm_guard_ws_bytes()
    assert opt.group_of == [1, 2, 0, 2, 1, 0]
    assert opt.poll() is None  # before the first copy has completed
    torch.cuda.synchronize()

    # a finite step first: the optimizer state exists and its step is 1
    _set_grads(model, 1)
    spy = _Spy(H.lib())
    monkeypatch.setattr(H, "lib", lambda: spy)
    opt.step(loss=torch.tensor(0.5, device=DEV))
    monkeypatch.undo()
    assert [c for c in spy.calls if c.startswith("td_")] == ["td_grad_norm_clip_guarded", "td_adamw_ema_step_guarded"]
    torch.cuda.synchronize()
    assert opt.step_dev.item() == 1

    def everything():
        torch.cuda.synchronize()
        sd = opt.state_dict()["state"]
        return ([p.detach().clone() for p in model.parameters()] + [p.detach().clone() for p in ema_model.parameters()] +
                [opt.flat_p.clone(), opt.ema.clone(), opt.exp_avg.clone(), opt.exp_avg_sq.clone(), opt.step_dev.clone()] +
                [sd[i][k].clone() for i in sorted(sd) for k in ("step", "exp_avg", "exp_avg_sq")])

    before = everything()
    assert len(opt.state_dict()["state"]) == 5 and all(float(s["step"]) == 1.0 for s in opt.state_dict()["state"].values())
    # the NaN step: nothing moves
    _set_grads(model, 2, nan_in="backbone.c")
    opt.step(loss=torch.tensor(float("nan"), device=DEV))
    after = everything()
    assert len(before) == len(after) and all(torch.equal(x, y) for x, y in zip(before, after)), "a skipped step changed something"
    assert opt.norm_clip[1].item() == 0 and not np.isfinite(opt.norm_clip[0].item())
    opt.poll()  # enqueues a copy behind the NaN step
    torch.cuda.current_stream().synchronize()
    snap = opt.guard_snapshot()
    assert (snap["attempts"], snap["skipped"], snap["consecutive_skipped"]) == (2, 1, 1)
    assert [r["applied"] for r in snap["history"]] == [True, False] and snap["last"]["step"] == 1 and snap["history"][0]["loss"] == 0.5
    assert np.isnan(snap["last"]["loss"]) and np.isnan(snap["last"]["norm"]) and snap["last"]["clip"] == 0
    assert np.isnan(snap["last"]["group_norm"][1]) and np.isfinite(snap["last"]["group_norm"][0]) and snap["last"]["group_norm"][3] == 0
    polled = opt.poll()  # the copy enqueued above has completed: one query, no waiting loop
    assert polled is not None and _same_snapshot(polled, snap), (polled, snap)
    with pytest.raises(NonFiniteStepError, match="1 optimizer steps in a row") as err:
        opt.raise_if_stuck(1)
    assert "'applied': False" in str(err.value) and "'attempt': 2" in str(err.value)
    opt.raise_if_stuck(2)  # one skipped step is not two

    # the following finite step equals a fresh UNGUARDED optimizer's step from the same state
    model2, ema2 = Small(SMALL_ORDER).to(DEV), Small(SMALL_ORDER).to(DEV)
    with torch.no_grad():
        for dst, src in ((model2, model), (ema2, ema_model)):
            for (_, a), (_, b) in zip(dst.named_parameters(), src.named_parameters()):
                a.copy_(b)
    opt2 = _make_opt(model2, ema2)
    assert opt2._guard is None and opt2.skip_nonfinite is False and opt2._ws.numel() == H.lib().td_grad_norm_ws_bytes()
    with pytest.raises(RuntimeError, match="skip_nonfinite"):
        opt2.guard_snapshot()
    with pytest.raises(ValueError, match="skip_nonfinite"):
        opt2.step(loss=torch.tensor(0.5, device=DEV))
    opt2.load_state_dict(opt.state_dict())
    assert torch.equal(opt2.flat_p, opt.flat_p) and torch.equal(opt2.ema, opt.ema) and torch.equal(opt2.exp_avg, opt.exp_avg) and \
        torch.equal(opt2.exp_avg_sq, opt.exp_avg_sq) and opt2.step_dev.item() == 1
    _set_grads(model, 3)
    _set_grads(model2, 3)
    opt.step()
    spy = _Spy(H.lib())
    monkeypatch.setattr(H, "lib", lambda: spy)
    opt2.step()
    monkeypatch.undo()
    assert [c for c in spy.calls if c.startswith("td_")] == ["td_grad_norm_clip", "td_adamw_ema_step"]
    torch.cuda.synchronize()
    for k in ("flat_p", "ema", "exp_avg", "exp_avg_sq", "step_dev", "norm_clip"):
        assert torch.equal(getattr(opt, k), getattr(opt2, k)), k
    assert opt.step_dev.item() == 2 and not torch.equal(opt.flat_p, before[2 * len(SMALL_ORDER)])
    opt.poll()
    torch.cuda.current_stream().synchronize()
    opt.raise_if_stuck(1)  # the finite step reset the run of skipped steps
    snap = opt.guard_snapshot()
    assert (snap["attempts"], snap["skipped"], snap["consecutive_skipped"]) == (3, 1, 0) and np.isnan(snap["last"]["loss"]) and snap["last"]["applied"]
    assert _same_snapshot(opt.poll(), snap)
    # a resume: torch's layout, applied updates only; the counters start again at zero
    sd = opt.state_dict()
    assert set(sd) == {"state", "param_groups"} and all(float(s["step"]) == 2.0 and set(s) == {"step", "exp_avg", "exp_avg_sq"} for s in sd["state"].values())
    opt.load_state_dict(sd)
    assert opt.guard_snapshot()["attempts"] == 0 and opt.poll() is None and opt.step_dev.item() == 2
