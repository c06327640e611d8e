"""Every dispatch route of td_conv_gemm / td_linear_ex (csrc/gemm_conv.hip, conv_gemm_launch) at the smallest shapes that reach it on
256 CUs, standing on each threshold from both sides.  Every case asserts three things:

  route   td_prof_enable / td_prof_dump record (family, dtype, M, N, K, R, stride, mode) of every launch: the case names the launches
          it expects, so a moved threshold shows up as a changed family instead of silently testing another kernel.  The record does
          not tell the 256- from the 128-wide instance of the 256-row tiles (it follows from Nc % 256) nor two from three stages of the
          tiled kernel (three when the 64x128 grid has at most 512 workgroups and K >= 1024): those pairs are run, not asserted.
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

pytestmark = pytest.mark.gpu

# thresholds below are derived for 256 CUs, and the dispatcher reads its A/B knobs once per process
if torch.cuda.is_available():
    _cus = torch.cuda.get_device_properties(0).multi_processor_count
    if _cus != 256:
        pytest.skip(f"route shapes are sized for 256 CUs, this device has {_cus}", allow_module_level=True)
_knobs = sorted(k for k in os.environ if k.startswith("TD_PW_PERSIST") or k.startswith("TD_CONV_") or k == "TD_DGRAD_S2_PARITY")
if _knobs:
    pytest.skip(f"dispatch knobs set in the environment ({', '.join(_knobs)}): the routes asserted here are the default ones", allow_module_level=True)

# TD_PROF_* of include/tubedetr_hip.h
T128, T128x64, T64, PERSIST, BIG, BIG_PW = 0, 1, 3, 4, 5, 6
FAMILY = {T128: "128x128", T128x64: "128x64", T64: "64x128", PERSIST: "persistent", BIG: "256-row", BIG_PW: "256-row pointwise"}
BF16, F32 = torch.bfloat16, torch.float32
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
             sigmoid=False, alpha=1.0, drop=0.0, pitch=0, inplace=False, seed=1, guard_rows=300):
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
    with recorded_routes(tmp_path) as rows:
        ops.conv_gemm_raw(x, wmat, out_v, desc, epi)
    code = 1 if dt == BF16 else 0
    if isinstance(expect, int):
        expect = [(expect, code, Mr, Nc, K, R, stride, mode)]
    assert rows == expect, ("recorded", _show(rows), "expected", _show(expect))

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


def case(id_, expect, **kw):
    return pytest.param(expect, kw, id=id_)


# ------------------------------------------------------------------------------------------------
# persistent weight-stationary instance (pw_resident2_kernel<NKT, RES, MSK>), bf16: needs cdiv(M, 64) >= 4 * 8 * (64 / (Nc / 128))
PERSISTENT = [
    case("Nc2048_K64_M8128_tiled", T64, M=8128, C=64, Nc=2048, relu=True),
    case("Nc2048_K64_M8129", PERSIST, M=8129, C=64, Nc=2048, relu=True),
    case("Nc2048_K64_M8129_pitch", PERSIST, M=8129, C=64, Nc=2048, relu=True, pitch=64),
    case("Nc1024_K128_M16320_res_tiled", T64, M=16320, C=128, Nc=1024, res=True, relu=True),
    case("Nc1024_K128_M16321_res", PERSIST, M=16321, C=128, Nc=1024, res=True, relu=True),
    case("Nc512_K192_M32704_mask_tiled", T64, M=32704, C=192, Nc=512, mask=True),
    case("Nc512_K192_M32705_mask", PERSIST, M=32705, C=192, Nc=512, mask=True),
    case("Nc512_K256_M32705_res_mask_pitch", PERSIST, M=32705, C=256, Nc=512, res=True, mask=True, pitch=64, inplace=True),
    case("strided_1x1_forward_odd_extent", PERSIST, N=3, H=105, W=105, C=128, Nc=2048, stride=2, relu=True),
    case("mode1_stride1_res_mask", PERSIST, M=8129, C=64, Nc=2048, mode=1, bias=False, res=True, mask=True),
    case("dropout", PERSIST, M=8129, C=128, Nc=2048, res=True, drop=0.1),
    case("dropout_pitch", PERSIST, M=8129, C=128, Nc=2048, res=True, drop=0.1, pitch=64),
    # refusals: the same row counts on the tiled kernel
    case("refuse_Nc384", T64, M=33000, C=64, Nc=384, res=True, relu=True),
    case("refuse_Nc768", T64, M=33000, C=64, Nc=768, mask=True),
    case("refuse_K320", T64, M=32705, C=320, Nc=512, res=True),
    case("refuse_alpha", T64, M=8129, C=64, Nc=2048, alpha=0.5),
    case("refuse_sigmoid", T64, M=8129, C=64, Nc=2048, sigmoid=True),
]


@pytest.mark.parametrize("expect,kw", PERSISTENT)
def test_persistent_route(expect, kw, tmp_path):
    run_conv(tmp_path, expect, seed=11, **kw)


# ------------------------------------------------------------------------------------------------
# 256-row tiles, pointwise (conv_gemm_big8_kernel<false, RES> at Nc % 256 == 0, conv_gemm_big8n_kernel<false> otherwise), bf16:
# needs 512 <= K <= 64 * 154 and cdiv(M, 256) * (Nc / (256 or 128)) >= 160
BIG_POINTWISE = [
    case("Nc2048_K512_M4864_tiled", T64, M=4864, C=512, Nc=2048, relu=True),
    case("Nc2048_K512_M4865", BIG_PW, M=4865, C=512, Nc=2048, relu=True),
    case("Nc2048_K512_M4865_pitch", BIG_PW, M=4865, C=512, Nc=2048, relu=True, pitch=64),
    case("Nc256_K512_M40704_res_tiled", T64, M=40704, C=512, Nc=256, res=True, relu=True),
    case("Nc256_K512_M40705_res_inplace", BIG_PW, M=40705, C=512, Nc=256, res=True, relu=True, inplace=True),
    case("Nc384_K576_M13568_res_tiled", T64, M=13568, C=576, Nc=384, res=True),
    case("Nc384_K576_M13569_res", BIG_PW, M=13569, C=576, Nc=384, res=True, pitch=64, inplace=True),  # 128 wide, three column tiles
    case("Nc128_K512_M40705_mask", BIG_PW, M=40705, C=512, Nc=128, mask=True),
    case("Nc2048_M4865_res_mask", BIG_PW, M=4865, C=640, Nc=2048, res=True, mask=True),
    case("K448_tiled", T64, M=4865, C=448, Nc=2048, relu=True),
    case("K9856_last_table_entry", BIG_PW, M=4865, C=9856, Nc=2048, relu=True),
    case("K9920_tiled_128x128", T128, M=4865, C=9920, Nc=2048, relu=True),
    case("dropout_falls_back_to_tiles", T64, M=4865, C=512, Nc=2048, drop=0.1),
    case("dropout_falls_back_to_tiles_pitch", T64, M=4865, C=512, Nc=2048, drop=0.1, pitch=64),
    case("dropout_falls_back_to_tiles_K576", T128, M=4865, C=576, Nc=2048, drop=0.1, pitch=64),
]


@pytest.mark.parametrize("expect,kw", BIG_POINTWISE)
def test_256_row_pointwise_route(expect, kw, tmp_path):
    run_conv(tmp_path, expect, seed=13, **kw)


# ------------------------------------------------------------------------------------------------
# 256-row tiles, tap-uniform walk (conv_gemm_big8_kernel<true, RES> / conv_gemm_big8n_kernel<true>): at most 32 taps, C % 64 == 0.
# Nc = 1024: four column tiles, cdiv(M, 256) >= 40 from M = 9985; Nc = 512: M >= 20225.  3 x 59 x 58 = 10266 rows, ragged last tile.
_OUT = dict(N=3, Nc=1024)
BIG_TAP_UNIFORM = [
    case("3x3_s1", BIG, N=5, H=65, W=63, C=64, Nc=512, R=3, S=3, pad=1, relu=True),
    case("3x3_s1_pitch", BIG, N=5, H=65, W=63, C=64, Nc=512, R=3, S=3, pad=1, relu=True, pitch=64),
    case("3x3_s2", BIG, H=117, W=115, C=64, R=3, S=3, stride=2, pad=1, relu=True, **_OUT),
    case("5x5", BIG, H=59, W=58, C=64, R=5, S=5, pad=2, relu=True, **_OUT),
    case("1x3", BIG, H=57, W=58, C=192, R=1, S=3, pad=1, **_OUT),
    case("3x1", BIG, H=59, W=56, C=192, R=3, S=1, pad=1, **_OUT),
    case("3x3_pad0", BIG, H=61, W=60, C=64, R=3, S=3, pad=0, **_OUT),
    case("3x3_pad2", BIG, H=57, W=56, C=64, R=3, S=3, pad=2, res=True, **_OUT),
    case("3x3_C1088_K9792", BIG, H=59, W=58, C=1088, R=3, S=3, pad=1, **_OUT),
    case("3x3_C1152_K10368_tiled", T128, H=59, W=58, C=1152, R=3, S=3, pad=1, **_OUT),
    case("3x3_rows_below_threshold_tiled", T128, H=59, W=56, C=64, R=3, S=3, pad=1, **_OUT),  # 9912 rows: 39 row tiles x 4 = 156 workgroups
    case("3x3_mode1_res_mask", BIG, H=59, W=58, C=64, R=3, S=3, pad=1, mode=1, bias=False, res=True, mask=True, **_OUT),
    case("5x5_mode1_res_mask", BIG, H=59, W=58, C=64, R=5, S=5, pad=2, mode=1, bias=False, res=True, mask=True, pitch=64, inplace=True, **_OUT),
    case("1x3_mode1_res_mask", BIG, H=59, W=58, C=192, R=1, S=3, pad=1, mode=1, bias=False, res=True, mask=True, **_OUT),
]


@pytest.mark.parametrize("expect,kw", BIG_TAP_UNIFORM)
def test_256_row_tap_uniform_route(expect, kw, tmp_path):
    run_conv(tmp_path, expect, seed=17, **kw)


# ------------------------------------------------------------------------------------------------
# tiled kernel (conv_gemm_kernel): 128x64 tiles at Nc <= 64; else 64x128 when cdiv(M, 128) * cdiv(Nc, 128) < 512 or K <= 512; else 128x128.
# Nc = 120 (one column tile, no multiple of 128: the persistent and 256-row routes refuse bf16 launches) stands on 511 / 512 tiles exactly:
# M = 65408 and 65409; Nc = 776 (seven column tiles) adds 73 x 7 = 511 against 74 x 7 = 518.
# Scalar epilogue (vec_ok false): ldc no multiple of 16 bytes (bf16: ldc % 8, fp32: ldc % 4) or a ragged last 16 bytes - bf16 Nc = 1, 2, 4, 100,
# 12 at ldc = 76, 65; fp32 Nc = 1, 2, 6, 101, 65 at ldc = 129 (fp32 Nc = 4, 12, 100 at ldc = Nc take the vector epilogue).
# Stage count (not recorded): three when the 64x128 grid 8 * cdiv(cdiv(M, 64), 8) * cdiv(Nc, 128) <= 512 and K >= 1024, bf16 only.  Nc = 128:
# grid 512 up to M = 32768 = 8 x 64 x 64, grid 520 at 8 x 64 x 65 rows; 128 / 130 workgroups of 256 rows stay below the 256-row route.
_SQ = dict(N=8, Nc=128)
TILED = [
    case("Nc64_narrow", T128x64, M=1000, C=128, Nc=64, res=True, relu=True),
    case("Nc64_narrow_pitch", T128x64, M=1000, C=128, Nc=64, res=True, relu=True, pitch=64),
    case("Nc65", T64, M=1000, C=128, Nc=65, res=True, relu=True),
    case("Nc1", T128x64, M=777, C=96, Nc=1, res=True, relu=True),
    case("Nc2", T128x64, M=777, C=96, Nc=2, mask=True),
    case("Nc4_sigmoid", T128x64, M=777, C=96, Nc=4, sigmoid=True),
    case("Nc4", T128x64, M=777, C=96, Nc=4, res=True, mask=True),
    case("Nc12", T128x64, M=777, C=96, Nc=12, res=True, relu=True, pitch=64),
    case("Nc100", T64, M=777, C=96, Nc=100, res=True, relu=True),
    case("Nc100_dropout", T64, M=777, C=96, Nc=100, drop=0.25),
    case("Nc100_dropout_pitch", T64, M=777, C=96, Nc=100, drop=0.25, pitch=64),  # scalar epilogue, key m * 164 + n
    case("Nc256_dropout_pitch", T64, M=777, C=96, Nc=256, res=True, drop=0.25, pitch=64),  # vector epilogue on 64x128 tiles
    case("Nc64_dropout_pitch", T128x64, M=1000, C=128, Nc=64, res=True, drop=0.25, pitch=64),  # 128x64 tiles
    case("tiles128_511_exact_K576", T64, M=65408, C=576, Nc=120, relu=True),
    case("tiles128_512_exact_K576", T128, M=65409, C=576, Nc=120, relu=True),
    case("tiles128_511_K576", T64, M=9344, C=576, Nc=776, relu=True),
    case("tiles128_518_K576", T128, M=9345, C=576, Nc=776, relu=True),
    case("tiles128_518_K576_pitch", T128, M=9345, C=576, Nc=776, res=True, mask=True, pitch=64),
    case("tiles128_518_K512", T64, M=9345, C=512, Nc=776, relu=True),
    # two against three stages: pointwise, tap-uniform, generic gather
    case("pw_K960_grid512", T64, M=32768, C=960, Nc=128, relu=True),
    case("pw_K1024_grid512_three_stages", T64, M=32768, C=1024, Nc=128, relu=True),
    case("pw_K1024_grid520", T64, M=32769, C=1024, Nc=128, relu=True),
    case("tu_3x5_K960_grid512", T64, H=64, W=66, C=64, R=3, S=5, pad=1, **_SQ),
    case("tu_4x4_K1024_grid512_three_stages", T64, H=65, W=65, C=64, R=4, S=4, pad=1, res=True, relu=True, **_SQ),
    case("tu_4x4_K1024_grid520", T64, H=65, W=66, C=64, R=4, S=4, pad=1, **_SQ),
    case("generic_3x3_C104_K936_grid512", T64, H=64, W=64, C=104, R=3, S=3, pad=1, **_SQ),
    case("generic_3x3_C120_K1080_grid512_three_stages", T64, H=64, W=64, C=120, R=3, S=3, pad=1, res=True, relu=True, **_SQ),
    case("generic_3x3_C120_K1080_grid520", T64, H=64, W=65, C=120, R=3, S=3, pad=1, **_SQ),
    case("generic_3x3_C120_mode1", T64, H=64, W=64, C=120, R=3, S=3, pad=1, mode=1, bias=False, res=True, mask=True, **_SQ),
    case("7x7_C64_49_taps_generic", T64, N=2, H=30, W=30, C=64, Nc=128, R=7, S=7, pad=3, relu=True),
    case("M1", T64, M=1, C=128, Nc=256, res=True),
    case("M63", T64, M=63, C=128, Nc=256, res=True, pitch=64),
    case("M65", T64, M=65, C=128, Nc=256, mask=True),
]
TILED_FP32 = [
    case("fp32_tap_uniform_C96", T64, dt=F32, N=2, H=20, W=21, C=96, Nc=128, R=3, S=3, pad=1, relu=True),
    case("fp32_tap_uniform_C96_s2", T64, dt=F32, N=2, H=21, W=23, C=96, Nc=128, R=3, S=3, stride=2, pad=1, res=True),
    case("fp32_Nc64_narrow", T128x64, dt=F32, M=1000, C=128, Nc=64, res=True, relu=True),
    case("fp32_Nc65", T64, dt=F32, M=1000, C=128, Nc=65, res=True, relu=True, pitch=64),
    case("fp32_Nc1", T128x64, dt=F32, M=777, C=100, Nc=1, res=True, relu=True),
    case("fp32_Nc2", T128x64, dt=F32, M=777, C=100, Nc=2, mask=True),
    case("fp32_Nc4", T128x64, dt=F32, M=777, C=100, Nc=4, res=True, mask=True),
    case("fp32_Nc12", T128x64, dt=F32, M=777, C=100, Nc=12, res=True, relu=True),
    case("fp32_Nc100", T64, dt=F32, M=777, C=100, Nc=100, res=True, relu=True),
    case("fp32_Nc6_scalar", T128x64, dt=F32, M=777, C=100, Nc=6, res=True, mask=True),
    case("fp32_Nc101_scalar", T64, dt=F32, M=777, C=100, Nc=101, res=True, relu=True),
    case("fp32_Nc101_scalar_dropout_pitch", T64, dt=F32, M=777, C=100, Nc=101, drop=0.25, pitch=64),
    case("fp32_tiles128_511_exact_K576", T64, dt=F32, M=65408, C=576, Nc=120, relu=True),
    case("fp32_tiles128_512_exact_K576", T128, dt=F32, M=65409, C=576, Nc=120, res=True, relu=True),
    case("fp32_tiles128_511_K576", T64, dt=F32, M=9344, C=576, Nc=776, relu=True),
    case("fp32_tiles128_518_K576", T128, dt=F32, M=9345, C=576, Nc=776, res=True, relu=True),
    case("fp32_tiles128_518_K512", T64, dt=F32, M=9345, C=512, Nc=776, relu=True),
    case("fp32_7x7_C64", T64, dt=F32, N=2, H=30, W=30, C=64, Nc=128, R=7, S=7, pad=3, relu=True),
    case("fp32_M1", T64, dt=F32, M=1, C=128, Nc=256, res=True),
    case("fp32_M63", T64, dt=F32, M=63, C=128, Nc=256, res=True),
    case("fp32_M65", T64, dt=F32, M=65, C=128, Nc=256, mask=True, pitch=64),
]


@pytest.mark.parametrize("expect,kw", TILED + TILED_FP32)
def test_tiled_route(expect, kw, tmp_path):
    run_conv(tmp_path, expect, seed=19, **kw)


@pytest.mark.parametrize("M,expect", [(1048575, PERSIST), (1048600, T64)], ids=["M1048575_below_persistent", "M1048600_above_tiled"])
def test_32_bit_output_offset_edge(M, expect, tmp_path):
    """(double)M * ldc < 2 147 483 000 admits the routes with 32-bit output offsets.  Nc = 2048, K = 64 is the persistent instance's shape:
    M = 1 048 575 (M * ldc = 2 147 481 600, byte offsets up to 2^32 - 4098) still runs on it, M = 1 048 600 (2 147 532 800) must be recorded
    as a tiled family, whose 64-bit offsets put the last rows where they belong.  First / interior / last 256 rows against fp64, guard rows
    untouched.  The file's largest allocations (4.3 GB of output): freed right after."""
    try:
        run_conv(tmp_path, expect, M=M, C=64, Nc=2048, relu=True, seed=23)
    finally:
        import gc

        gc.collect()
        torch.cuda.empty_cache()


# ------------------------------------------------------------------------------------------------
# input gradient of a 3x3 / stride 2 / pad 1 convolution: four parity-class launches on even extents, one gather otherwise
@pytest.mark.parametrize("pitch", [0, 64])
@pytest.mark.parametrize("even", [True, False], ids=["even_extent_four_launches", "odd_extent_one_launch"])
def test_stride2_input_gradient_routes(even, pitch, tmp_path):
    N, C, Nc = 3, 64, 128  # forward layer: Nc -> C channels; g [N, 12, 10, C] -> dx [N, H, W, Nc]
    H, W = (24, 20) if even else (23, 19)
    Mg = N * 12 * 10
    expect = [(T64, 1, Mg, Nc, taps * C, r, 1, 0) for r, taps in ((1, 1), (1, 2), (2, 2), (2, 4))] if even else [(T64, 1, N * H * W, Nc, 9 * C, 3, 2, 1)]
    run_conv(tmp_path, expect, N=N, H=H, W=W, C=C, Nc=Nc, R=3, S=3, stride=2, pad=1, mode=1, bias=False, res=True, mask=True, pitch=pitch, seed=29)


# ------------------------------------------------------------------------------------------------
# td_linear_ex (the GX instances of conv_gemm_kernel): K1 = K2 = 320
LINEAR_EX = [  # id, family, M, N
    ("128x128", T128, 8192, 1024),
    ("64x128", T64, 512, 1024),
    ("128x64", T128x64, 512, 48),
]


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
    with recorded_routes(tmp_path) as rows:
        ops.linear_ex(a1, w, bias, a2=a2, a1_map=a1_map, a2_map=a2_map, w_shared=shared, out=out_v, out_map=out_map, residual=res, res_map=res_map,
                      relu=True, mask_src=msk_v, dropout_p=drop, seed=4321)
    expect = [(family, 1 if dt == BF16 else 0, M, Nn, 2 * K1, 1, 1, 2)]
    assert rows == expect, ("recorded", _show(rows), "expected", _show(expect))

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
