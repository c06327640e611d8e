"""The flat kernels of tubedetr_amd/csrc/elementwise.hip through the C ABI against tests/elementwise_ref.py, at the sizes
where a 16-byte vector body, a scalar tail and a capped grid with a grid-stride loop go wrong: n = 1, VEC-1, VEC, VEC+1,
257*VEC+3 and one vector plus three elements past the 4096-workgroup cap.  Every buffer carries 64 sentinel elements behind
its payload that must survive.  td_add, td_relu_bwd and td_dropout are compared bit for bit; GELU, colsum and LayerNorm
under bounds derived from the number formats (tests/test_elementwise_cpu.py shows what those bounds exclude).

Worst err/bound measured on an MI355X (printed by the tests; the bound is 1.0):
    td_gelu_fwd  fp32 0.29, bf16 1.00      td_gelu_bwd  fp32 0.28, bf16 1.00
    td_colsum    fp32 0.40, bf16 0.10
    td_add_layernorm_fwd / _bwd, err / (row scale * TOL): fp32 0.011, bf16 0.32
The bf16 GELU figures sit at 1.00 by construction: the bound is the fp32 part (what the fp32 line measures) plus half a bf16
ulp of the result, and round-to-nearest reaches exactly half an ulp wherever the fp32 value falls on a tie; a truncating
store, at up to a whole ulp, would be at 2.
"""
import itertools

import numpy as np
import pytest
import torch

import elementwise_ref as E

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
PAD = 64
DT = {"f32": torch.float32, "bf16": torch.bfloat16}
INT = {"f32": torch.int32, "bf16": torch.int16}
SENT = {"f32": 0x7FC5A5A5, "bf16": 0x7FA5}  # NaN payloads no kernel arithmetic produces
DTYPES = ["f32", "bf16"]


def _hip():
    from tubedetr_amd import _hip

    return _hip


def code(dt):
    return _hip().dtype_code(DT[dt])


def sentinel_buf(n, dt, lead=0):
    """Integer-typed device buffer of lead + n + PAD elements, all sentinel; 16-byte aligned."""
    t = torch.full((lead + n + PAD,), SENT[dt], dtype=INT[dt], device=DEV)
    assert t.data_ptr() % 16 == 0
    return t


def dev(x, dt, lead=0):
    """float32 array of ``dt`` values -> sentinel-padded device buffer holding exactly those bit patterns behind ``lead``
    sentinel elements."""
    b = E.bits(np.ravel(x), dt)
    t = sentinel_buf(b.size, dt, lead)
    t[lead : lead + b.size] = torch.from_numpy(b.view(np.int32 if dt == "f32" else np.int16)).to(DEV)
    return t


def ptr(t, lead=0):
    return None if t is None else t.data_ptr() + lead * t.element_size()


def got_bits(t, n, dt, lead=0):
    torch.cuda.synchronize()
    return t[lead : lead + n].cpu().numpy().view(np.uint32 if dt == "f32" else np.uint16)


def got_f32(t, n, dt, lead=0):
    b = got_bits(t, n, dt, lead)
    return b.view(np.float32) if dt == "f32" else E.bf16_bits_to_f32(b)


def intact(t, n, dt, lead=0):
    return bool((t[:lead] == SENT[dt]).all().item() and (t[lead + n:] == SENT[dt]).all().item())


def ok(rc, what):
    _hip().check(rc, what)


def rand(n, dt, seed):
    rng = np.random.default_rng(seed)
    return E.round_to(rng.standard_normal(n) * 10.0 ** rng.integers(-3, 3, n), dt)


# ---------------------------------------------------------------------------------------------------- single roundings
@pytest.mark.parametrize("dt", DTYPES)
def test_add_is_bit_exact(dt):
    H = _hip()
    for n in E.sizes(dt):
        a, b = rand(n, dt, 1), rand(n, dt, 2)
        da, db = dev(a, dt), dev(b, dt)
        for with_b in (True, False):
            y = sentinel_buf(n, dt)
            ok(H.lib().td_add(ptr(da), ptr(db) if with_b else None, ptr(y), n, code(dt), H.stream_ptr()), "td_add")
            want = E.add_ref(a, b if with_b else None, dt)
            assert np.array_equal(got_bits(y, n, dt), want), (n, with_b)  # b = NULL: a copy
            assert intact(y, n, dt) and np.array_equal(got_bits(da, n, dt), E.bits(a, dt)), n


@pytest.mark.parametrize("dt", DTYPES)
def test_relu_bwd_is_bit_exact(dt):
    """The mask is y > 0: NaN, +0 and -0 block the gradient, the smallest positive subnormal passes it."""
    H = _hip()
    for n in E.sizes(dt):
        dy, y = E.relu_cases(n, dt)
        ddy, dy_ = dev(dy, dt), dev(y, dt)
        for scale in (1.0, 0.5, 1 / 0.9):
            g = sentinel_buf(n, dt)
            ok(H.lib().td_relu_bwd(ptr(ddy), ptr(dy_), ptr(g), n, scale, code(dt), H.stream_ptr()), "td_relu_bwd")
            out, want = got_bits(g, n, dt), E.relu_bwd_ref(dy, y, scale, dt)
            bad = np.nonzero(out != want)[0]
            assert len(bad) == 0, (n, scale, int(bad[0]), float(y[bad[0]]), float(dy[bad[0]]), hex(int(out[bad[0]])), hex(int(want[bad[0]])))
            assert intact(g, n, dt)


def _counter(value):
    return torch.tensor([value - (1 << 32) if value >= 1 << 31 else value], dtype=torch.int32, device=DEV)


@pytest.mark.parametrize("dt", DTYPES)
def test_dropout_p0_is_a_copy(dt):
    from tubedetr_amd import ops

    H = _hip()
    ops.set_dropout_counter(_counter(5))
    try:
        for n in E.sizes(dt):
            x = rand(n, dt, 3)
            dx, y = dev(x, dt), sentinel_buf(n, dt)
            ok(H.lib().td_dropout(ptr(dx), ptr(y), n, 0.0, 77, ops._ctr(), code(dt), H.stream_ptr()), "td_dropout")
            assert np.array_equal(got_bits(y, n, dt), E.bits(x, dt)) and intact(y, n, dt), n
        small = torch.from_numpy(rand(100, "f32", 4)).to(DEV).to(DT[dt])
        assert torch.equal(ops.dropout(small, 0.0, 77), small)
    finally:
        ops.set_dropout_counter(None)


P_DROP = (1e-10, 0.1, 0.5, 0.999)
SEEDS = (0, 1234, 0xFFFFFFFF)
COUNTERS = (None, 0, 1, 0xFFFFFFFF)


@pytest.mark.parametrize("dt", DTYPES)
def test_dropout_mask_is_the_documented_hash(dt):
    """keep(i) = hash32(i * golden + effective seed) >= uint32(p * 2^32) (at least 1), restated on the host in numpy uint32;
    kept values are x * float32(1 / (1 - p)), bit for bit.  Every (p, seed, counter) at the small sizes; four (seed, counter)
    pairs x every p past the grid cap."""
    from tubedetr_amd import ops

    H = _hip()
    sizes = E.sizes(dt)
    big = sizes[-1]
    ones_big = dev(np.ones(big, np.float32), dt)  # a prefix of it serves every size
    big_pairs = {(0, None), (1234, 0), (0xFFFFFFFF, 1), (1234, 0xFFFFFFFF)}
    try:
        for seed, ctr in itertools.product(SEEDS, COUNTERS):
            ops.set_dropout_counter(None if ctr is None else _counter(ctr))
            nmax = big if (seed, ctr) in big_pairs else sizes[-2]
            h = torch.from_numpy(E.hash32(E.effective_seed(seed, ctr), nmax).astype(np.int64)).to(DEV)
            for p in P_DROP:
                kept = torch.from_numpy(E.bits(np.ones(1, np.float32) * E.dropout_scale(p), dt).astype(np.int64)).to(DEV).to(INT[dt])
                keep = h >= E.threshold(p)
                for n in sizes:
                    if n > nmax:
                        continue
                    y = sentinel_buf(n, dt)
                    ok(H.lib().td_dropout(ptr(ones_big), ptr(y), n, p, seed, ops._ctr(), code(dt), H.stream_ptr()), "td_dropout")
                    want = torch.where(keep[:n], kept, torch.zeros_like(kept))
                    same = torch.equal(y[:n], want)
                    assert same, (p, seed, ctr, n, "first mismatch at", int((y[:n] != want).nonzero()[0]))
                    assert intact(y, n, dt)
                if p == 1e-10:
                    assert keep.sum().item() >= nmax - 1  # the threshold clamps to 1: only a hash of exactly 0 is dropped
        # the wrapper hands the counter on (and scales a non-trivial x)
        ops.set_dropout_counter(_counter(1))
        x = rand(2059, dt, 6)
        y = ops.dropout(torch.from_numpy(x).to(DEV).to(DT[dt]), 0.5, 1234)
        keep = E.dropout_keep(2059, 0.5, 1234, 1)
        want = E.bits(np.where(keep, x * E.dropout_scale(0.5), np.float32(0)).astype(np.float32), dt)
        assert np.array_equal(y.view(INT[dt]).cpu().numpy().view(want.dtype), want)
    finally:
        ops.set_dropout_counter(None)


# ----------------------------------------------------------------------------------------------------------------- GELU
@pytest.mark.parametrize("dt", DTYPES)
def test_gelu_fwd_bwd_against_float64_erf_form(dt):
    H = _hip()
    worst_f = worst_b = 0.0
    for n in E.sizes(dt):
        x, dy = E.gelu_inputs(dt, n)
        dx_, ddy = dev(x, dt), dev(dy, dt)
        y, g = sentinel_buf(n, dt), sentinel_buf(n, dt)
        ok(H.lib().td_gelu_fwd(ptr(dx_), ptr(y), n, code(dt), H.stream_ptr()), "td_gelu_fwd")
        ok(H.lib().td_gelu_bwd(ptr(ddy), ptr(dx_), ptr(g), n, code(dt), H.stream_ptr()), "td_gelu_bwd")
        out_f, out_b = got_f32(y, n, dt).astype(np.float64), got_f32(g, n, dt).astype(np.float64)
        assert intact(y, n, dt) and intact(g, n, dt) and np.isfinite(out_f).all() and np.isfinite(out_b).all(), n
        x64, dy64 = x.astype(np.float64), dy.astype(np.float64)
        for name, out, ref, bnd in (("fwd", out_f, E.gelu64(x64), E.gelu_fwd_bound(x, dt)), ("bwd", out_b, dy64 * E.gelu_grad64(x64), E.gelu_bwd_bound(dy, x, dt))):
            err = np.abs(out - ref)
            with np.errstate(divide="ignore", invalid="ignore"):
                ratio = np.where(err == 0, 0.0, err / bnd)
            i = int(ratio.argmax())
            if name == "fwd":
                worst_f = max(worst_f, float(ratio[i]))
            else:
                worst_b = max(worst_b, float(ratio[i]))
            assert ratio[i] <= 1.0, (name, n, "x", float(x[i]), "dy", float(dy[i]), "got", float(out[i]), "want", float(ref[i]), "err/bound", float(ratio[i]))
    print(f"gelu {dt}: worst err/bound forward {worst_f:.3f}, backward {worst_b:.3f}")


# --------------------------------------------------------------------------------------------------------------- colsum
def _colsum(g_dev, out, rows, cols, ld, dt):
    H = _hip()
    ok(H.lib().td_colsum(ptr(g_dev), ptr(out), rows, cols, ld, code(dt), H.stream_ptr()), "td_colsum")


@pytest.mark.parametrize("dt", DTYPES)
def test_colsum_routes_and_row_strides(dt):
    worst = 0.0
    for route, rows, cols, ld in E.colsum_shapes(dt):
        assert E.colsum_route(cols, ld, dt) == route
        g, want, bnd = E.colsum_case(rows, cols, ld, dt)
        gd = dev(g, dt)
        pre = (np.arange(cols) % 5 - 2).astype(np.float32) * 0.75
        for start in (np.zeros(cols, np.float32), pre):  # the sum is ADDED to what out holds
            out = dev(start, "f32")
            _colsum(gd, out, rows, cols, ld, dt)
            res = got_f32(out, cols, "f32").astype(np.float64)
            b = bnd if not start.any() else (rows + 1) * E.U * (np.abs(start) + bnd / (rows * E.U))  # one more operand per column
            err = np.abs(res - (want + start))
            worst = max(worst, float((err / b).max()))
            assert (err <= b).all(), (route, rows, cols, ld, float((err / b).max()))
            assert intact(out, cols, "f32")
    print(f"colsum {dt}: worst err/bound {worst:.3f}")


@pytest.mark.parametrize("dt", DTYPES)
def test_colsum_empty_and_deterministic(dt):
    import tubedetr_amd

    v = E.VEC[dt]
    g, _, _ = E.colsum_case(4, v, v, dt)
    gd = dev(g, dt)
    start = np.array([1.5, -2.0, 3.25] + [0.5] * (v - 3), np.float32)
    for rows, cols in ((0, v), (4, 0), (0, 0)):
        out = dev(start, "f32")
        _colsum(gd, out, rows, cols, v, dt)
        assert np.array_equal(got_f32(out, v, "f32"), start) and intact(out, v, "f32")
    was = tubedetr_amd.is_deterministic()
    try:
        tubedetr_amd.set_deterministic(True)
        for rows, cols, ld in ((129, 33 * v, 33 * v), (1000, 3 * v, 3 * v), (130, 7, 7), (65, 7, 9)):
            g, want, bnd = E.colsum_case(rows, cols, ld, dt, seed=1)
            gd = dev(g, dt)
            runs = []
            for _ in range(2):
                out = dev(np.zeros(cols, np.float32), "f32")
                _colsum(gd, out, rows, cols, ld, dt)
                runs.append(got_bits(out, cols, "f32"))
            assert np.array_equal(runs[0], runs[1]), (rows, cols, ld)
            assert (np.abs(runs[0].view(np.float32).astype(np.float64) - want) <= bnd).all()
    finally:
        tubedetr_amd.set_deterministic(was)


# ------------------------------------------------------------------------------------------------------------ LayerNorm
EPS = 1e-5


class LN:
    """Device buffers of one LayerNorm case; every tensor of the compute dtype sits ``lead`` elements into its allocation."""

    def __init__(self, x, r, gamma, beta, dy, extra, dt, lead=0):
        self.dt, self.lead, (self.rows, self.cols) = dt, lead, x.shape
        n = x.size
        self.n = n
        self.x, self.r = dev(x, dt, lead), None if r is None else dev(r, dt, lead)
        self.dy, self.extra = dev(dy, dt, lead), None if extra is None else dev(extra, dt, lead)
        self.gamma, self.beta = dev(gamma, "f32"), dev(beta, "f32")
        self.y, self.s, self.ds = sentinel_buf(n, dt, lead), sentinel_buf(n, dt, lead), sentinel_buf(n, dt, lead)
        self.mean, self.rstd = sentinel_buf(self.rows, "f32"), sentinel_buf(self.rows, "f32")

    def fwd(self, save=True):
        H, L = _hip(), self.lead
        ok(H.lib().td_add_layernorm_fwd(ptr(self.x, L), ptr(self.r, L), ptr(self.gamma), ptr(self.beta), ptr(self.y, L),
                                        ptr(self.s, L) if (save and self.r is not None) else None, ptr(self.mean) if save else None,
                                        ptr(self.rstd) if save else None, self.rows, self.cols, EPS, code(self.dt), H.stream_ptr()), "td_add_layernorm_fwd")
        f = lambda t: got_f32(t, self.n, self.dt, L).reshape(self.rows, self.cols)
        assert all(intact(t, self.n, self.dt, L) for t in (self.y, self.s)) and intact(self.mean, self.rows, "f32") and intact(self.rstd, self.rows, "f32")
        return f(self.y), f(self.s), got_f32(self.mean, self.rows, "f32"), got_f32(self.rstd, self.rows, "f32")

    def bwd(self, s_dev, dgamma=None, dbeta=None, want_dg=True, want_db=True):
        """s_dev: the device buffer holding the saved sum (self.s, or self.x when there was no residual)."""
        H, L = _hip(), self.lead
        dg = dev(np.zeros(self.cols, np.float32) if dgamma is None else dgamma, "f32")
        db = dev(np.zeros(self.cols, np.float32) if dbeta is None else dbeta, "f32")
        ok(H.lib().td_add_layernorm_bwd(ptr(self.dy, L), ptr(s_dev, L), ptr(self.mean), ptr(self.rstd), ptr(self.gamma), ptr(self.extra, L), ptr(self.ds, L),
                                        ptr(dg) if want_dg else None, ptr(db) if want_db else None, self.rows, self.cols, code(self.dt), H.stream_ptr()),
           "td_add_layernorm_bwd")
        assert intact(self.ds, self.n, self.dt, L) and intact(dg, self.cols, "f32") and intact(db, self.cols, "f32")
        return got_f32(self.ds, self.n, self.dt, L).reshape(self.rows, self.cols), got_f32(dg, self.cols, "f32"), got_f32(db, self.cols, "f32")


def _check_ln(case, dt, worst, what, with_r=True, with_extra=True):
    """Forward and backward of one case against float64, per element relative to the row's scale."""
    x, r, gamma, beta, dy, extra = case
    ln = LN(x, r if with_r else None, gamma, beta, dy, extra if with_extra else None, dt)
    tol = E.LN_TOL[dt]
    y, s, mean, rstd = ln.fwd()
    y64, s64, mean64, rstd64 = E.ln_fwd64(x, r if with_r else None, gamma, beta, EPS)
    errs = {"y": E.row_rel_err(y, y64), "mean": float(np.abs(mean - mean64).max() / np.abs(s64).max()), "rstd": float((np.abs(rstd - rstd64) / rstd64).max())}
    if with_r:
        errs["s"] = E.row_rel_err(s, s64)
    # the backward is checked on its own inputs: the saved sum as the device stored it, and the device's mean / rstd
    s_in = s if with_r else x
    ds, dgamma, dbeta = ln.bwd(ln.s if with_r else ln.x)
    ds64, dg64, db64 = E.ln_bwd64(dy, s_in, mean.astype(np.float64), rstd.astype(np.float64), gamma, extra if with_extra else None)
    errs.update(ds=E.row_rel_err(ds, ds64), dgamma=E.row_rel_err(dgamma, dg64), dbeta=E.row_rel_err(dbeta, db64))
    for k, e in errs.items():
        t = E.LN_TOL["f32"] if k in ("mean", "rstd") else tol  # mean / rstd are fp32 in both modes
        worst[0] = max(worst[0], e / t)
        assert e <= t, (what, k, e, t)
    return ln, (y, s, mean, rstd, ds, dgamma, dbeta)


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("cols", E.LN_COLS)
def test_add_layernorm_against_float64(cols, dt):
    worst = [0.0]
    for rows in E.LN_ROWS:
        _check_ln(E.ln_case(rows, cols, dt), dt, worst, (rows, cols, dt))
    print(f"layernorm {dt} cols {cols} ({E.ln_route(cols, dt)}): worst err / (row scale * TOL) {worst[0]:.3f}")


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("cols", [65, 256])
def test_add_layernorm_optional_arguments(cols, dt):
    H = _hip()
    case = E.ln_case(5, cols, dt, seed=3)
    x, r, gamma, beta, dy, extra = case
    worst = [0.0]
    base, (y0, s0, mean0, rstd0, ds0, dg0, db0) = _check_ln(case, dt, worst, "all present")
    _check_ln(case, dt, worst, "r = None", with_r=False)
    _check_ln(case, dt, worst, "extra = None", with_extra=False)
    # save = False: mean, rstd and s_out NULL - y is the same, nothing else is written
    ln = LN(*case, dt)
    y, s, mean, rstd = ln.fwd(save=False)
    assert np.array_equal(E.bits(y, dt), E.bits(y0, dt))
    assert (ln.s == SENT[dt]).all().item() and (ln.mean == SENT["f32"]).all().item() and (ln.rstd == SENT["f32"]).all().item()
    # dgamma / dbeta NULL: ds is the same; pre-filled: the kernel adds to them
    ds, _, _ = base.bwd(base.s, want_dg=False, want_db=False)
    assert np.array_equal(E.bits(ds, dt), E.bits(ds0, dt))
    ds, dg, _ = base.bwd(base.s, want_db=False)
    assert np.array_equal(E.bits(ds, dt), E.bits(ds0, dt)) and E.row_rel_err(dg, dg0.astype(np.float64)) <= E.LN_TOL["f32"]
    pre_g, pre_b = np.linspace(-3, 3, cols).astype(np.float32), np.linspace(5, -5, cols).astype(np.float32)
    _, dg, db = base.bwd(base.s, dgamma=pre_g, dbeta=pre_b)
    for got, pre, zero_based in ((dg, pre_g, dg0), (db, pre_b, db0)):
        want = pre.astype(np.float64) + zero_based
        assert E.row_rel_err(got, want) <= E.LN_TOL["f32"], (cols, dt)
    # cols = 1025 is rejected on the host; rows = 0 is a no-op
    before = [t.clone() for t in (base.y, base.s, base.ds, base.mean, base.rstd)]
    L = H.lib()
    if base.n >= 1025:  # (the buffers would hold the row even if the check were missing)
        assert L.td_add_layernorm_fwd(ptr(base.x), ptr(base.r), ptr(base.gamma), ptr(base.beta), ptr(base.y), ptr(base.s), ptr(base.mean), ptr(base.rstd), 1,
                                      1025, EPS, code(dt), H.stream_ptr()) == -1
        assert L.td_add_layernorm_bwd(ptr(base.dy), ptr(base.s), ptr(base.mean), ptr(base.rstd), ptr(base.gamma), None, ptr(base.ds), None, None, 1, 1025,
                                      code(dt), H.stream_ptr()) == -1
    ok(L.td_add_layernorm_fwd(ptr(base.x), ptr(base.r), ptr(base.gamma), ptr(base.beta), ptr(base.y), ptr(base.s), ptr(base.mean), ptr(base.rstd), 0, cols, EPS,
                              code(dt), H.stream_ptr()), "rows = 0")
    ok(L.td_add_layernorm_bwd(ptr(base.dy), ptr(base.s), ptr(base.mean), ptr(base.rstd), ptr(base.gamma), None, ptr(base.ds), None, None, 0, cols, code(dt),
                              H.stream_ptr()), "rows = 0")
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(before, (base.y, base.s, base.ds, base.mean, base.rstd)))


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("cols", [65, 768, 1000])
def test_add_layernorm_constant_rows(cols, dt):
    """Variance 0: rstd = 1 / sqrt(eps), y = beta, and the backward's x_hat is 0 up to the rounding of the mean (0.5, 2 and
    -1.25 sum exactly in fp32; the vector route multiplies by a rounded 1 / cols, so its mean may be one ulp off)."""
    rows = 3
    x, r, gamma, beta, dy, extra = E.ln_case(rows, cols, dt, seed=5)
    x = np.repeat(np.array([[0.5], [2.0], [-1.25]], np.float32), cols, axis=1)
    ln = LN(x, None, gamma, beta, dy, extra, dt)
    y, _, mean, rstd = ln.fwd()
    assert (np.abs(mean - x[:, 0]) <= 2 * E.U * np.abs(x[:, 0])).all() and (np.abs(rstd - 1 / np.sqrt(EPS)) <= 2e-5 / np.sqrt(EPS)).all()
    if E.ln_route(cols, dt) == "generic":
        assert np.array_equal(mean, x[:, 0]) and np.array_equal(E.bits(y, dt), E.bits(np.broadcast_to(beta, x.shape).copy(), dt))
    assert E.row_rel_err(y, np.broadcast_to(beta.astype(np.float64), x.shape)) <= E.LN_TOL[dt]
    ds, dgamma, dbeta = ln.bwd(ln.x)
    ds64, dg64, db64 = E.ln_bwd64(dy, x, mean.astype(np.float64), rstd.astype(np.float64), gamma, extra)
    xh_max = float(np.abs((x - mean[:, None].astype(np.float64)) * rstd[:, None]).max())
    assert np.abs(dgamma - dg64).max() <= E.LN_TOL["f32"] * max(1e-30, np.abs(dy).sum(0).max() * xh_max)  # exactly 0 where the mean is exact
    # (ds = rstd * (dy*gamma - its row mean) + extra is a difference of terms 316 x larger than a typical element)
    scale = (rstd[:, None] * np.abs(dy * gamma)).max(axis=1, keepdims=True) + np.abs(extra).max(axis=1, keepdims=True)
    assert (np.abs(ds - ds64) <= E.LN_TOL[dt] * scale).all() and E.row_rel_err(dbeta, db64) <= E.LN_TOL["f32"]


def _ulp_bf16(a):
    return 2.0 * E.half_ulp_bf16(a)


@pytest.mark.parametrize("det", [False, True])
def test_add_layernorm_bf16_misaligned_storage_takes_the_generic_kernel(det):
    """256-column bf16 tensors that start one element (2 bytes) into their allocation are not 8-byte aligned: the launch must
    fall back to the generic kernel, which only makes 2-byte accesses, and agree with the vector route on the same values
    within one bf16 ulp.  (gamma, beta, mean and rstd stay aligned: the vector route reads them 16 bytes at a time.)  In
    deterministic mode both routes are bit-reproducible."""
    import tubedetr_amd

    case = E.ln_case(33, 256, "bf16", seed=7)
    was = tubedetr_amd.is_deterministic()
    try:
        tubedetr_amd.set_deterministic(det)
        outs = {}
        for lead in (0, 1):
            rep = []
            for _ in range(2):
                ln = LN(*case, "bf16", lead=lead)
                assert (ptr(ln.x, lead) % 8 == 0) == (lead == 0) and ptr(ln.x, lead) % 2 == 0
                y, s, mean, rstd = ln.fwd()
                ds, dg, db = ln.bwd(ln.s)
                rep.append((y, s, mean, rstd, ds, dg, db))
            if det:
                assert all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(*rep)), ("not bit-reproducible", lead)
            outs[lead] = rep[0]
        for name, a, b in zip(("y", "s", "mean", "rstd", "ds", "dgamma", "dbeta"), outs[0], outs[1]):
            a64, b64 = a.astype(np.float64), b.astype(np.float64)
            if name in ("y", "s", "ds"):
                assert (np.abs(a64 - b64) <= _ulp_bf16(np.maximum(np.abs(a64), np.abs(b64)))).all(), name
            else:
                assert E.row_rel_err(b, a64) <= E.LN_TOL["f32"], name
    finally:
        tubedetr_amd.set_deterministic(was)


@pytest.mark.parametrize("dt", DTYPES)
def test_add_layernorm_deterministic_generic_route(dt):
    import tubedetr_amd

    case = E.ln_case(33, 65, dt, seed=8)
    was = tubedetr_amd.is_deterministic()
    try:
        tubedetr_amd.set_deterministic(True)
        rep = []
        for _ in range(2):
            ln = LN(*case, dt)
            ln.fwd()
            rep.append(ln.bwd(ln.s))
        assert all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(*rep))
    finally:
        tubedetr_amd.set_deterministic(was)
