"""The cases of tests/elementwise_ref.py are well posed (no GPU): the host restatement of the dropout hash behaves like a
mask generator, the GELU bounds hold for a float32 implementation and exclude the tanh approximation and a backward that
lacks x*phi(x), the colsum / LayerNorm shapes take the routes they are meant to take, and the Python wrappers refuse a
strided view before anything reaches the device."""
import numpy as np
import pytest
import torch

import elementwise_ref as E


def test_sizes_cover_the_paths():
    for dt, v in E.VEC.items():
        s = E.sizes(dt)
        assert s[:4] == [1, v - 1, v, v + 1] and s[4] % v == 3 and s[4] // v > 256
        assert s[5] // v == E.GRID_CAP * 256 + 1 and s[5] % v == 3  # one vector and a 3-element tail past the capped grid


def test_bf16_rounding_is_nearest_even():
    x = np.array([1.0, 1.00390625, 1.01171875, -1.00390625, 3.0e38, np.inf, -0.0], np.float32)  # ties at 1 + 2^-8, 1 + 3*2^-8
    want = torch.from_numpy(x).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)
    assert np.array_equal(E.f32_to_bf16_bits(x), want)
    rnd = np.random.default_rng(0).standard_normal(4096).astype(np.float32)
    assert np.array_equal(E.f32_to_bf16_bits(rnd), torch.from_numpy(rnd).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16))
    assert np.isnan(E.bf16_bits_to_f32(E.f32_to_bf16_bits(np.array([np.nan], np.float32))))[0]
    assert E.half_ulp_bf16(np.array([1.0, 1.5, 2.0]))[0] == 2.0 ** -8 and E.half_ulp_bf16(np.array([2.0]))[0] == 2.0 ** -7


def test_relu_cases_hold_the_specials():
    for dt in E.VEC:
        dy, y = E.relu_cases(100, dt)
        b = E.bits(y, dt)
        top = 31 if dt == "f32" else 15
        assert (b == 0).any() and (b == (1 << top)).any() and (b == 1).any() and np.isnan(y).any() and (y < 0).any() and (y > 1).any()
        out = E.relu_bwd_ref(dy, y, 0.5, dt)
        blocked = ~(y > 0)
        assert (out[blocked] == 0).all() and blocked[np.isnan(y)].all() and not blocked[b == 1].any()


def test_dropout_restatement():
    """What the host restatement can show on its own: the keep-rate, and that counters 0 and 1 draw unrelated masks."""
    n = 1 << 20
    for p in (0.1, 0.5, 0.999):
        for seed, ctr in ((0, None), (1234, 0), (0xFFFFFFFF, 1), (1234, 0xFFFFFFFF)):
            keep = E.dropout_keep(n, p, seed, ctr).mean()
            sigma = np.sqrt(p * (1 - p) / n)
            assert abs(keep - (1 - p)) <= 4 * sigma, (p, seed, ctr, keep)
    assert E.threshold(1e-10) == 1 and E.threshold(0.0) == 0 and E.threshold(0.5) == 1 << 31 and E.threshold(0.999) < 1 << 32
    assert E.dropout_keep(n, 1e-10, 7).all() or (~E.dropout_keep(n, 1e-10, 7)).sum() <= 1  # only a hash of exactly 0 is dropped
    m0, m1 = E.dropout_keep(n, 0.5, 1234, 0), E.dropout_keep(n, 0.5, 1234, 1)
    assert not np.array_equal(m0, m1) and abs((m0 == m1).mean() - 0.5) < 4 * 0.5 / np.sqrt(n)
    for shift in range(1, 65):  # ... nor a shift of one another (what a counter ADDED to the seed would give)
        agree = (m0[shift:] == m1[:-shift]).mean(), (m1[shift:] == m0[:-shift]).mean()
        assert max(abs(a - 0.5) for a in agree) < 5 * 0.5 / np.sqrt(n - shift), shift
    assert E.effective_seed(5, None) == 5 and E.effective_seed(5, 0) != 5
    assert E.dropout_scale(0.1) == np.float32(1) / np.float32(0.9)


def _gelu_ratios(dt):
    x, dy = E.gelu_inputs(dt, 3 * 4811)
    x64, dy64 = x.astype(np.float64), dy.astype(np.float64)
    ef = np.abs(E.gelu_emul32(x).astype(np.float64) - E.gelu64(x64))
    eb = np.abs(E.gelu_grad_emul32(dy, x).astype(np.float64) - dy64 * E.gelu_grad64(x64))
    with np.errstate(divide="ignore", invalid="ignore"):
        rf = np.where(ef == 0, 0.0, ef / (E.U * np.abs(x64)))
        rb = np.where(eb == 0, 0.0, eb / (E.U * np.abs(dy64) * (1 + np.abs(x64))))
    return float(rf.max()), float(rb.max())


def test_gelu_constants_come_from_the_float32_emulation():
    rf, rb = (max(a) for a in zip(_gelu_ratios("f32"), _gelu_ratios("bf16")))
    print(f"float32 emulation against float64: forward {rf:.2f} units of 2^-24 |x|, backward {rb:.2f} units of 2^-24 |dy| (1 + |x|)")
    assert abs(rf - E.GELU_FWD_MEASURED) < 0.05 and abs(rb - E.GELU_BWD_MEASURED) < 0.05, "update the measured ratios in elementwise_ref.py"
    assert 4 * rf <= E.C_GELU_FWD <= 4 * E.GELU_FWD_MEASURED + 0.2 and E.C_GELU_FWD <= 64
    assert 4 * rb <= E.C_GELU_BWD <= 4 * E.GELU_BWD_MEASURED + 0.2 and E.C_GELU_BWD <= 64


@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_gelu_cases_are_well_posed(dt):
    x, dy = E.gelu_inputs(dt, 3 * 4811)
    assert (E.bits(x, "f32") == 0).any() and (E.bits(x, "f32") == 1 << 31).any() and (np.abs(x) == np.float32(E.BF16_MAX)).any()
    assert ((np.abs(x) > 4e-5) & (np.abs(x) < 3e-4)).sum() >= 6 and x.min() == -np.float32(E.BF16_MAX) and np.abs(dy).max() / np.abs(dy).min() > 1e6
    x64, dy64 = x.astype(np.float64), dy.astype(np.float64)
    # a float32 implementation (rounded to bf16 where the kernel stores bf16) is inside the bound
    fwd, bwd = E.round_to(E.gelu_emul32(x), dt), E.round_to(E.gelu_grad_emul32(dy, x), dt)
    assert (np.abs(fwd.astype(np.float64) - E.gelu64(x64)) <= E.gelu_fwd_bound(x, dt)).all()
    assert (np.abs(bwd.astype(np.float64) - dy64 * E.gelu_grad64(x64)) <= E.gelu_bwd_bound(dy, x, dt)).all()
    # the tanh approximation and a backward without x*phi(x) are more than 10 x the bound away somewhere
    far_f = np.abs(E.gelu_tanh64(x64) - E.gelu64(x64)) / E.gelu_fwd_bound(x, dt).clip(1e-300)
    far_b = np.abs(dy64 * (E.gelu_grad_no_pdf64(x64) - E.gelu_grad64(x64))) / E.gelu_bwd_bound(dy, x, dt).clip(1e-300)
    print(f"{dt}: tanh approximation up to {far_f.max():.0f} x the bound, backward without x*phi(x) up to {far_b.max():.0f} x")
    assert far_f.max() > 10 and far_b.max() > 10


def test_colsum_and_layernorm_cases_take_their_routes():
    for dt in E.VEC:
        for route, rows, cols, ld in E.colsum_shapes(dt):
            assert E.colsum_route(cols, ld, dt) == route and ld >= cols, (dt, route, rows, cols, ld)
        shapes = E.colsum_shapes(dt)
        assert {r for r, *_ in shapes} == {"vector", "generic"} and any(ld > c for _, _, c, ld in shapes)
        # a partial last group of 32 column vectors, several row lanes, and more than one 64-row workgroup
        assert any(r == "vector" and (c // E.VEC[dt]) % 32 for r, _, c, _ in shapes) and any(rows > 64 for _, rows, _, _ in shapes)
    g, want, bnd = E.colsum_case(65, 16, 40, "bf16")
    assert g.shape == (65, 40) and (g[:, 16:] == 777.0).all() and want.shape == (16,) and (bnd > 0).all()
    assert [E.ln_route(c, "bf16") for c in E.LN_COLS] == ["generic"] * 4 + ["vector"] * 2 + ["generic"] * 2
    assert all(E.ln_route(c, "f32") == "generic" for c in E.LN_COLS) and max(E.LN_COLS) == 1024
    x, r, gamma, beta, dy, extra = E.ln_case(3, 65, "f32")
    y, s, mean, rstd = E.ln_fwd64(x, r, gamma, beta, 1e-5)
    t = torch.from_numpy(s).requires_grad_(True)
    gm = torch.from_numpy(gamma.astype(np.float64)).requires_grad_(True)
    bt = torch.from_numpy(beta.astype(np.float64)).requires_grad_(True)
    yt = torch.nn.functional.layer_norm(t, (65,), gm, bt, 1e-5)
    yt.backward(torch.from_numpy(dy.astype(np.float64)))
    ds, dgamma, dbeta = E.ln_bwd64(dy, s, mean, rstd, gamma, extra)
    assert np.allclose(y, yt.detach().numpy(), rtol=0, atol=1e-12) and np.allclose(ds - extra, t.grad.numpy(), rtol=0, atol=1e-12)
    assert np.allclose(dgamma, gm.grad.numpy(), rtol=0, atol=1e-12) and np.allclose(dbeta, bt.grad.numpy(), rtol=0, atol=1e-12)


def test_wrappers_refuse_a_transposed_view():
    """The flat wrappers pass numel() / shape and a raw pointer: a strided view must raise before any launch (the check
    comes first, so it is visible without a device)."""
    from tubedetr_amd import ops

    a = torch.randn(8, 16)
    t = torch.randn(16, 8).t()  # same shape, not contiguous
    v = torch.randn(16)
    assert not t.is_contiguous() and t.shape == a.shape
    calls = [lambda: ops.add(t, a), lambda: ops.add(a, t), lambda: ops.relu_bwd(t, a), lambda: ops.relu_bwd(a, t), lambda: ops.gelu_fwd(t),
             lambda: ops.gelu_bwd(t, a), lambda: ops.gelu_bwd(a, t), lambda: ops.dropout(t, 0.1, 1), lambda: ops.colsum(t),
             lambda: ops.colsum(a, torch.randn(32)[::2]), lambda: ops.add_layernorm_fwd(t, a, v, v, 1e-5), lambda: ops.add_layernorm_fwd(a, t, v, v, 1e-5),
             lambda: ops.add_layernorm_fwd(a, a, torch.randn(32)[::2], v, 1e-5), lambda: ops.add_layernorm_fwd(a, a, v, torch.randn(32)[::2], 1e-5),
             lambda: ops.add_layernorm_bwd(t, a, v[:8], v[:8], v), lambda: ops.add_layernorm_bwd(a, t, v[:8], v[:8], v),
             lambda: ops.add_layernorm_bwd(a, a, v[::2], v[:8], v), lambda: ops.add_layernorm_bwd(a, a, v[:8], v[::2], v),
             lambda: ops.add_layernorm_bwd(a, a, v[:8], v[:8], torch.randn(32)[::2]), lambda: ops.add_layernorm_bwd(a, a, v[:8], v[:8], v, t)]
    for i, call in enumerate(calls):
        with pytest.raises(AssertionError, match="contiguous"):
            call()
