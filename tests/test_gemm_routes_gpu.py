"""Every dispatch route of td_conv_gemm / td_linear_ex (planned by csrc/gemm_route.h, launched by launch_route of csrc/gemm_conv.hip) at the
smallest shapes that reach it on 256 CUs, standing on each threshold from both sides (the cases: tests/gemm_route_cases.py).  Every case
asserts three things:

  route   td_prof_enable / td_prof_dump record (family, dtype, M, N, K, R, stride, mode) of every launch: the case names the launches
          it expects, so a moved threshold shows up as a changed family instead of silently testing another kernel.  The record does
          not tell the 256- from the 128-wide instance of the 256-row tiles (it follows from Nc % 256) nor two from three stages of the
          tiled kernel (three when the 64x128 grid has at most 512 workgroups and K >= 1024): td_conv_gemm_route / td_linear_ex_route
          return the plan the launch runs - its rows must equal the recorded ones, its stages / walk / bn what the case states
          (tests/test_gemm_routes_cpu.py asserts the same plans without a GPU).
  value   operands are bf16-rounded (or fp32) values, identical on both sides; the reference is the same operation in fp64 on the
          device.  PER ELEMENT  |got - ref| <= u_out |ref| + (K + 4) 2^-24 A,  A = the same product of absolute values
          (|x| @ |w|^T + |bias| + |res|) in fp64: output rounding (u_out = 2^-8 for bf16, the project's figure; 2^-23 for fp32) plus
          the worst-case fp32 accumulation bound.  ReLU, the ReLU mask and dropout are selections: an element they drop must be an
          exact zero (for ReLU wherever the reference lies further below zero than the accumulation bound).  Sigmoid cases use the
          max|err| / max|ref| metric of test_ops_gpu.py (the error of the fast exponential is not derivable).
  guard   the launch writes into a view [M, Nc] of a sentinel-filled buffer [M + 300, ldc]: rows M.. and, with ldc > Nc, columns
          Nc.. must still hold the sentinel.  The first case of each route runs at ldc == Nc and at ldc == Nc + 64 (residual and mask
          share the pitch).

Dropout epilogues key their mask on the OUTPUT OFFSET m * ldc + n: the cases compare with ops.dropout over the full-pitch [M, ldc]
buffer of the same seed; at ldc = Nc + 64 (where m * ldc + n and m * Nc + n differ) this pins the rule on the persistent instance, all three
tile shapes of the tiled kernel (vector and scalar epilogue) and td_linear_ex - the 256-row tiles hand dropout to the tiled kernel."""
import contextlib
import math
import os

import pytest
import torch
import torch.nn.functional as F

from gemm_route_cases import BF16, BIG_POINTWISE, BIG_TAP_UNIFORM, F32, FAMILY, LINEAR_EX, OFFSET_EDGE, PERSISTENT, STRIDE2_GRAD, TILED, TILED_FP32

pytestmark = pytest.mark.gpu

# thresholds below are derived for 256 CUs, and the dispatcher reads its A/B knobs once per process
if torch.cuda.is_available():
    _cus = torch.cuda.get_device_properties(0).multi_processor_count
    if _cus != 256:
        pytest.skip(f"route shapes are sized for 256 CUs, this device has {_cus}", allow_module_level=True)
_knobs = sorted(k for k in os.environ if k.startswith("TD_PW_PERSIST") or k.startswith("TD_CONV_") or k == "TD_DGRAD_S2_PARITY")
if _knobs:
    pytest.skip(f"dispatch knobs set in the environment ({', '.join(_knobs)}): the routes asserted here are the default ones", allow_module_level=True)

SENTINEL = 7.0
TOL = {F32: 2e-5, BF16: 1.2e-2}  # max|err| / max|ref| (test_ops_gpu.py): sigmoid cases only


def dev():
    return torch.device("cuda:0")


@contextlib.contextmanager
def recorded_routes(tmp_path):
    """rows (family, dtype, M, N, K, R, stride, mode) of every launch made inside the block, filled when it ends"""
    from tubedetr_amd import _hip

    lib = _hip.lib()
    rows = []
    _hip.check(lib.td_prof_enable(1), "td_prof_enable")
    try:
        yield rows
        path = str(tmp_path / "routes.csv")
        _hip.check(lib.td_prof_dump(path.encode()), "td_prof_dump")
        with open(path) as f:
            lines = f.read().split()
        assert lines[0] == "family,dtype,M,N,K,R,stride,mode,ms"
        rows.extend(tuple(int(v) for v in ln.split(",")[:8]) for ln in lines[1:])
    finally:
        lib.td_prof_enable(0)


def _show(rows):
    return [(FAMILY.get(r[0], r[0]),) + tuple(r[1:]) for r in rows]


def _planned_rows(routes):
    return [(r.family, r.dtype, r.M, r.N, r.K, r.R, r.stride, r.mode) for r in routes]


def _rand(shape, g, dt, scale=1.0):
    return (torch.randn(shape, generator=g, device=dev(), dtype=torch.float32) * scale).to(dt)


def _pitched(rows, cols, ldc, dt, g=None, extra=0):
    """a [rows, cols] view of a [rows + extra, ldc] buffer: sentinel-filled (g None) or random"""
    if g is None:
        buf = torch.full((rows + extra, ldc), SENTINEL, dtype=dt, device=dev())
    else:
        buf = _rand((rows + extra, ldc), g, dt)
    return buf, buf[:rows, :cols]


def check_values(got, pre, A, K, dt, *, relu=False, mask=None, keep=None, drop_scale=1.0, what=None):
    """got [m, n] against the fp64 pre-selection reference `pre` and its absolute-value companion A (see the module docstring)"""
    got = got.double()
    acc = (K + 4) * 2.0**-24 * A * drop_scale
    ref = pre
    if relu:
        ref = ref.clamp_min(0.0)
        must_zero = pre < -acc / drop_scale
        assert bool((got[must_zero] == 0).all()), (what, "ReLU let a negative value through", int((got[must_zero] != 0).sum()))
    if mask is not None:
        ref = ref * mask
        assert bool((got[~mask] == 0).all()), (what, "masked elements are not exact zeros", int((got[~mask] != 0).sum()))
    if keep is not None:
        ref = ref * keep * drop_scale
        assert bool((got[~keep] == 0).all()), (what, "dropped elements are not exact zeros", int((got[~keep] != 0).sum()))
    u_out = 2.0**-8 if dt == BF16 else 2.0**-23
    bound = u_out * ref.abs() + acc
    err = (got - ref).abs()
    bad = err > bound
    ratio = float((err / bound.clamp_min(1e-300)).max())
    print(f"  {what}: max err/bound {ratio:.3f}")
    assert not bool(bad.any()), (what, "elements out of bound", int(bad.sum()), "max err/bound", ratio, "first", [int(i) for i in bad.nonzero()[0]])


def _row_ranges(M, limit_rows):
    if M <= limit_rows:
        return [(0, M)]
    n = 256
    mid = (M // 2) // 128 * 128 + 37  # an interior tile, not aligned to it
    return [(0, n), (mid, mid + n), (M - n, M)]  # first tile, an interior one, the ragged last one


def run_conv(tmp_path, expect, *, dt=BF16, N=1, H=None, W=1, M=None, C, Nc, R=1, S=1, stride=1, pad=0, mode=0, bias=True, res=False, mask=False, relu=False,
             sigmoid=False, alpha=1.0, drop=0.0, pitch=0, inplace=False, seed=1, guard_rows=300, plan=None):
    """One td_conv_gemm launch.  mode 0: x [N, H, W, C] -> y [N, Ho, Wo, Nc].  mode 1 (input gradient of a forward conv Nc -> C channels):
    g [N, Hg, Wg, C] -> dx [N, H, W, Nc].  M = ... is the pointwise shorthand for N = 1, H = M, W = 1."""
    from tubedetr_amd import ops

    if M is not None:
        H, W = M, 1
    g = torch.Generator(device=dev()).manual_seed(seed)
    K = R * S * C
    if mode == 0:
        Hs, Ws = H, W
        Ho, Wo = ops.conv_out(H, R, stride, pad), ops.conv_out(W, S, stride, pad)
        w4 = _rand((Nc, C, R, S), g, dt, 1.0 / math.sqrt(K))
        wmat = w4.permute(0, 2, 3, 1).reshape(Nc, K).contiguous()  # [Co][r][s][ci]
    else:
        Ho, Wo = H, W
        Hs, Ws = ops.conv_out(H, R, stride, pad), ops.conv_out(W, S, stride, pad)
        w4 = _rand((C, Nc, R, S), g, dt, 1.0 / math.sqrt(K))
        wmat = w4.permute(1, 2, 3, 0).reshape(Nc, K).contiguous()  # [Ci][r][s][co]
    Mr = N * Ho * Wo
    ldc = Nc + pitch
    x = _rand((N, Hs, Ws, C), g, dt)
    b = torch.randn(Nc, generator=g, device=dev()) if bias else None
    res_buf, res_v = _pitched(Mr, Nc, ldc, dt, g) if res else (None, None)
    msk_buf, msk_v = _pitched(Mr, Nc, ldc, dt, g) if mask else (None, None)
    out_buf, out_v = _pitched(Mr, Nc, ldc, dt, extra=guard_rows)
    desc = ops._desc(N, Hs, Ws, C, Ho, Wo, R, S, stride, pad, mode, Nc, ldc)
    epi = ops._epi(b, res_v, msk_v, relu, sigmoid, drop, 4321, alpha)
    planned = ops.conv_gemm_route(desc, epi, dt, _cus)  # the query plans what the launch below runs
    with recorded_routes(tmp_path) as rows:
        ops.conv_gemm_raw(x, wmat, out_v, desc, epi)
    code = 1 if dt == BF16 else 0
    if isinstance(expect, int):
        expect = [(expect, code, Mr, Nc, K, R, stride, mode)]
    assert rows == expect, ("recorded", _show(rows), "expected", _show(expect))
    assert _planned_rows(planned) == rows, ("planned", _show(_planned_rows(planned)), "recorded", _show(rows))
    for key, want in (plan or {}).items():  # what the case states beyond the record (stages, walk, bn)
        assert [getattr(r, key) for r in planned] == [want], (key, [getattr(r, key) for r in planned], want)

    # guard region
    assert bool((out_buf[Mr:] == SENTINEL).all()), "rows past M were written"
    if pitch:
        assert bool((out_buf[:Mr, Nc:] == SENTINEL).all()), "columns past Nc were written"

    # reference in fp64 (whole launch, or row ranges of a pointwise launch above ~50 MB of output)
    pointwise = R == 1 and S == 1 and stride == 1 and pad == 0
    ranges = _row_ranges(Mr, 50e6 / (Nc * out_v.element_size())) if pointwise else [(0, Mr)]
    keep = None
    if drop > 0:
        keep = ops.dropout(torch.ones((Mr, ldc), dtype=dt, device=dev()), drop, 4321)[:, :Nc] != 0
        rate = 1.0 - keep.double().mean().item()
        assert abs(rate - drop) < 0.01, rate
    for a, e in ranges:
        if pointwise:
            x2, w2 = x.reshape(Mr, C)[a:e].double(), wmat.double()
            pre, A = x2 @ w2.t(), x2.abs() @ w2.abs().t()
        else:
            conv = (lambda t_, w_: F.conv2d(t_, w_, stride=stride, padding=pad)) if mode == 0 else \
                   (lambda t_, w_: F.conv_transpose2d(t_, w_, stride=stride, padding=pad,
                                                      output_padding=(Ho - ((Hs - 1) * stride - 2 * pad + R), Wo - ((Ws - 1) * stride - 2 * pad + S))))
            x4, w8 = x.double().permute(0, 3, 1, 2), w4.double()
            pre = conv(x4, w8).permute(0, 2, 3, 1).reshape(Mr, Nc)
            A = conv(x4.abs(), w8.abs()).permute(0, 2, 3, 1).reshape(Mr, Nc)
            del x4
        pre, A = pre * alpha, A * abs(alpha)
        if bias:
            pre, A = pre + b.double(), A + b.double().abs()
        if res:
            pre, A = pre + res_v[a:e].double(), A + res_v[a:e].double().abs()
        got = out_v[a:e]
        what = (FAMILY[expect[0][0]], Mr, Nc, K, a)
        if sigmoid:
            ref = torch.sigmoid(pre.clamp_min(0.0) if relu else pre)
            rel = ((got.double() - ref).abs().max() / ref.abs().max()).item()
            assert rel < TOL[dt], (what, rel)
        else:
            check_values(got, pre, A, K, dt, relu=relu, mask=(msk_v[a:e] > 0) if mask else None, keep=keep[a:e] if keep is not None else None,
                         drop_scale=1.0 / (1.0 - drop), what=what)
        del pre, A
    if inplace:  # in place on the residual (the input-gradient chain accumulates this way): bit-equal to out of place
        pad_cols = res_buf[:, Nc:].clone()
        with recorded_routes(tmp_path) as rows2:
            ops.conv_gemm_raw(x, wmat, res_v, desc, epi)
        assert rows2 == expect
        assert torch.equal(res_v, out_v), "in-place residual differs from out of place"
        assert torch.equal(res_buf[:, Nc:], pad_cols), "columns past Nc were written"
    return out_v


# ------------------------------------------------------------------------------------------------
# the case tables: tests/gemm_route_cases.py (tests/test_gemm_routes_cpu.py asserts the planned route of the same cases without a GPU)
@pytest.mark.parametrize("expect,kw,plan", PERSISTENT)
def test_persistent_route(expect, kw, plan, tmp_path):
    run_conv(tmp_path, expect, seed=11, plan=plan, **kw)


@pytest.mark.parametrize("expect,kw,plan", BIG_POINTWISE)
def test_256_row_pointwise_route(expect, kw, plan, tmp_path):
    run_conv(tmp_path, expect, seed=13, plan=plan, **kw)


@pytest.mark.parametrize("expect,kw,plan", BIG_TAP_UNIFORM)
def test_256_row_tap_uniform_route(expect, kw, plan, tmp_path):
    run_conv(tmp_path, expect, seed=17, plan=plan, **kw)


@pytest.mark.parametrize("expect,kw,plan", TILED + TILED_FP32)
def test_tiled_route(expect, kw, plan, tmp_path):
    run_conv(tmp_path, expect, seed=19, plan=plan, **kw)


@pytest.mark.parametrize("expect,kw,plan", OFFSET_EDGE)
def test_32_bit_output_offset_edge(expect, kw, plan, tmp_path):
    """(double)M * ldc < 2 147 483 000 admits the routes with 32-bit output offsets.  Nc = 2048, K = 64 is the persistent instance's shape:
    M = 1 048 575 (M * ldc = 2 147 481 600, byte offsets up to 2^32 - 4098) still runs on it, M = 1 048 600 (2 147 532 800) must be recorded
    as a tiled family, whose 64-bit offsets put the last rows where they belong.  First / interior / last 256 rows against fp64, guard rows
    untouched.  The file's largest allocations (4.3 GB of output): freed right after."""
    try:
        run_conv(tmp_path, expect, seed=23, plan=plan, **kw)
    finally:
        import gc

        gc.collect()
        torch.cuda.empty_cache()


# ------------------------------------------------------------------------------------------------
# input gradient of a 3x3 / stride 2 / pad 1 convolution: four parity-class launches on even extents, one gather otherwise
@pytest.mark.parametrize("pitch", [0, 64])
@pytest.mark.parametrize("expect,kw,plan", STRIDE2_GRAD)
def test_stride2_input_gradient_routes(expect, kw, plan, pitch, tmp_path):
    run_conv(tmp_path, expect, pitch=pitch, seed=29, plan=plan, **kw)


# ------------------------------------------------------------------------------------------------
# td_linear_ex (the GX instances of conv_gemm_kernel): K1 = K2 = 320
@pytest.mark.parametrize("dt", [BF16, F32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("variant", ["concat_maps_res_mask", "concat_maps_res_mask_pitch", "shared_maps_dropout_pitch", "concat_identity_rows"])
@pytest.mark.parametrize("shape", LINEAR_EX, ids=[s[0] for s in LINEAR_EX])
def test_linear_ex_routes(shape, variant, dt, tmp_path):
    """out[out_map[m]] = epilogue([a1[a1_map[m]] | a2[a2_map[m]]] @ w^T + bias + residual[res_map[m]]) on all three tile shapes: all four row
    maps, residual through res_map (own pitch), ReLU-mask and dropout epilogues (both keyed on the OUTPUT row), a shared weight; rows no
    index points at keep the sentinel."""
    from tubedetr_amd import ops

    _, family, M, Nn = shape
    K1 = 320
    shared = variant.startswith("shared")
    mapped = "maps" in variant
    use_mask = variant.startswith("concat_maps_res_mask")
    drop = 0.1 if shared else 0.0
    pitch = 64 if variant.endswith("pitch") else 0
    g = torch.Generator(device=dev()).manual_seed(31 + M + Nn)
    rows1, rows2, rows_r = (M // 3 + 5, M // 2 + 3, M // 4 + 7) if mapped else (M, M, M)
    out_rows = M + 17 if mapped else M
    a1, a2 = _rand((rows1, K1), g, dt), _rand((rows2, K1), g, dt)
    w = _rand((Nn, K1 if shared else 2 * K1), g, dt, 1.0 / math.sqrt(2 * K1))
    bias = torch.randn(Nn, generator=g, device=dev())
    res = _rand((rows_r, Nn + 8), g, dt)[:, :Nn]  # a pitch of its own (ldr != ldc)
    ldc = Nn + pitch
    ri = lambda hi: torch.randint(0, hi, (M,), generator=g, device=dev(), dtype=torch.int32)
    a1_map, a2_map, res_map = (ri(rows1), ri(rows2), ri(rows_r)) if mapped else (None, None, None)
    out_map = torch.randperm(out_rows, generator=g, device=dev())[:M].to(torch.int32) if mapped else None
    out_buf, out_v = _pitched(out_rows, Nn, ldc, dt, extra=300)
    msk_buf, msk_v = _pitched(out_rows, Nn, ldc, dt, g) if use_mask else (None, None)
    planned = ops.linear_ex_route(ops.linear_ex_desc(M, Nn, K1, K1, a1, a2, out_v, res, shared, a1_map, a2_map, out_map, res_map), True,
                                  ops._epi(bias, res, msk_v, True, False, drop, 4321), dt, _cus)
    with recorded_routes(tmp_path) as rows:
        ops.linear_ex(a1, w, bias, a2=a2, a1_map=a1_map, a2_map=a2_map, w_shared=shared, out=out_v, out_map=out_map, residual=res, res_map=res_map,
                      relu=True, mask_src=msk_v, dropout_p=drop, seed=4321)
    expect = [(family, 1 if dt == BF16 else 0, M, Nn, 2 * K1, 1, 1, 2)]
    assert rows == expect, ("recorded", _show(rows), "expected", _show(expect))
    assert _planned_rows(planned) == rows, ("planned", _show(_planned_rows(planned)), "recorded", _show(rows))

    orow = out_map.long() if mapped else torch.arange(M, device=dev())
    untouched = torch.ones(out_rows + 300, dtype=torch.bool, device=dev())
    untouched[orow] = False
    assert bool((out_buf[untouched] == SENTINEL).all()), "rows no index points at were written"
    if pitch:
        assert bool((out_buf[:, Nn:] == SENTINEL).all()), "columns past N were written"

    X1 = (a1[a1_map.long()] if mapped else a1).double()
    X2 = (a2[a2_map.long()] if mapped else a2).double()
    w1, w2 = (w.double(), w.double()) if shared else (w[:, :K1].double(), w[:, K1:].double())
    r_ = (res[res_map.long()] if mapped else res).double()
    pre = X1 @ w1.t() + X2 @ w2.t() + bias.double() + r_
    A = X1.abs() @ w1.abs().t() + X2.abs() @ w2.abs().t() + bias.double().abs() + r_.abs()
    keep = None
    if drop > 0:
        keep = (ops.dropout(torch.ones((out_rows, ldc), dtype=dt, device=dev()), drop, 4321)[:, :Nn] != 0)[orow]
    check_values(out_v[orow], pre, A, 2 * K1, dt, relu=True, mask=(msk_v[orow] > 0) if use_mask else None, keep=keep, drop_scale=1.0 / (1.0 - drop),
                 what=("td_linear_ex", FAMILY[family], variant))
