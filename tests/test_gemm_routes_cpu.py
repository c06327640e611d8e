"""The route table of td_conv_gemm / td_linear_ex ("Which kernel a td_conv_gemm / td_linear_ex launch runs on") asserted without a
GPU: td_conv_gemm_route / td_linear_ex_route run the planner the launching calls run (csrc/gemm_route.h) and return the plan.  Every case of
tests/gemm_route_cases.py - the shapes tests/test_gemm_routes_gpu.py launches - is planned for 256 CUs and compared with

  record  the row (family, dtype, M, N, K, R, stride, mode) the profiler would record for each launch;
  plan    what the case states beyond the record: stages (2 / 3 of the tiled kernel), the operand walk, the 256- or 128-wide instance of
          the 256-row tiles - what the GPU test runs but cannot see;
  grid    workgroups and threads by DESIGN.md's formulas: tiled 8 cdiv(cdiv(M, bm), 8) cdiv(Nc, bn) x 256; persistent 2 n_cu x 256;
          256-row 8 cdiv(cdiv(M, 256), 8) (Nc / bn) x 512, the 256-wide instance capped at n_cu (persistent, one workgroup per CU).

Every argument check of the two entry points is reached once through the launching call (which returns before any launch) and through the
query: same code, same message.  (The planner's "weight-column subset" check guards the parity classes it builds itself; no argument of
td_conv_gemm reaches it.)"""
import ctypes
import os

import pytest

from gemm_route_cases import (BF16, BIG, BIG_POINTWISE, BIG_PW, BIG_TAP_UNIFORM, F32, FAMILY, GATHER, GX, LINEAR_EX, OFFSET_EDGE, PERSIST, PERSISTENT, PW,
                              STRIDE2_GRAD, T64, T128, T128x64, TILED, TILED_FP32, TU)

_knobs = sorted(k for k in os.environ if k.startswith("TD_PW_PERSIST") or k.startswith("TD_CONV_") or k == "TD_DGRAD_S2_PARITY")
if _knobs:
    pytest.skip(f"dispatch knobs set in the environment ({', '.join(_knobs)}): the routes asserted here are the default ones", allow_module_level=True)

N_CU = 256
TILE = {T128: (128, 128), T128x64: (128, 64), T64: (64, 128)}
KERNEL_TILED, KERNEL_PERSISTENT, KERNEL_BIG8, KERNEL_BIG8N = 0, 1, 2, 3
PTR = ctypes.c_void_p(16)  # stands for a device pointer: the query only tests it for NULL, the launching call returns before it is used


def cdiv(a, b):
    return -(-a // b)


@pytest.fixture(scope="module")
def lib():
    from tubedetr_amd import _hip
    from tubedetr_amd.build import build_lib

    build_lib(verbose=False)
    return _hip.lib()


def conv_args(dt=BF16, N=1, H=None, W=1, M=None, C=None, Nc=None, R=1, S=1, stride=1, pad=0, mode=0, bias=True, res=False, mask=False, relu=False,
              sigmoid=False, alpha=1.0, drop=0.0, pitch=0, inplace=False):
    """descriptor and epilogue of the launch run_conv (test_gemm_routes_gpu.py) makes from the same keywords"""
    from tubedetr_amd import _hip, ops

    if M is not None:
        H, W = M, 1
    if mode == 0:
        Hs, Ws, Ho, Wo = H, W, ops.conv_out(H, R, stride, pad), ops.conv_out(W, S, stride, pad)
    else:
        Ho, Wo, Hs, Ws = H, W, ops.conv_out(H, R, stride, pad), ops.conv_out(W, S, stride, pad)
    desc = ops._desc(N, Hs, Ws, C, Ho, Wo, R, S, stride, pad, mode, Nc, Nc + pitch)
    epi = _hip.Epilogue(PTR if bias else None, PTR if res else None, PTR if mask else None, int(relu), int(sigmoid), float(drop), 4321, float(alpha), None)
    return desc, epi, dt


def planned(routes):
    return [(r.family, r.dtype, r.M, r.N, r.K, r.R, r.stride, r.mode) for r in routes]


def check_grid(r):
    if r.kernel == KERNEL_TILED:
        bm, bn = TILE[r.family]
        assert (r.bm, r.bn) == (bm, bn)
        assert (r.grid, r.block) == (8 * cdiv(cdiv(r.M, bm), 8) * cdiv(r.N, bn), 256)
    elif r.kernel == KERNEL_PERSISTENT:
        assert r.family == PERSIST and (r.bm, r.bn, r.grid, r.block) == (64, 128, 2 * N_CU, 256)
    else:
        assert r.family in (BIG, BIG_PW) and r.bm == 256 and r.bn == (256 if r.kernel == KERNEL_BIG8 else 128) and r.N % r.bn == 0
        tiles = 8 * cdiv(cdiv(r.M, 256), 8) * (r.N // r.bn)
        assert (r.grid, r.block) == (min(tiles, N_CU) if r.kernel == KERNEL_BIG8 else tiles, 512)


ALL_CONV = PERSISTENT + BIG_POINTWISE + BIG_TAP_UNIFORM + TILED + TILED_FP32 + OFFSET_EDGE + STRIDE2_GRAD


@pytest.mark.parametrize("expect,kw,plan", ALL_CONV)
def test_conv_route(expect, kw, plan, lib):
    from tubedetr_amd import ops

    desc, epi, dt = conv_args(**kw)
    routes = ops.conv_gemm_route(desc, epi, dt, N_CU)
    if isinstance(expect, int):
        expect = [(expect, 1 if dt == BF16 else 0, desc.N * desc.Ho * desc.Wo, desc.Nc, desc.R * desc.S * desc.C, desc.R, desc.stride, desc.mode)]
    assert planned(routes) == expect, ("planned", planned(routes), "expected", expect)
    for r in routes:
        check_grid(r)
        tiled = r.family in TILE
        assert (r.kernel == KERNEL_TILED) == tiled and (r.kernel == KERNEL_PERSISTENT) == (r.family == PERSIST)
        assert r.stages in ((2, 3) if tiled else (0,))
        assert r.walk != GX
        assert r.family != PERSIST or r.walk == PW
        assert r.family != BIG_PW or r.walk == PW
        assert r.family != BIG or r.walk == TU
    if "stages" in plan:
        assert [r.stages for r in routes] == [plan["stages"]]
    if "walk" in plan:
        assert [r.walk for r in routes] == [plan["walk"]]
    if "bn" in plan:
        assert [(r.bm, r.bn, r.kernel) for r in routes] == [(256, plan["bn"], KERNEL_BIG8 if plan["bn"] == 256 else KERNEL_BIG8N)]


def test_every_tiled_case_states_its_stages_and_every_256_row_case_its_width():
    for p in ALL_CONV:
        expect, _, plan = p.values
        if isinstance(expect, int):
            assert ("stages" in plan) == (expect in TILE), p.id
            assert ("bn" in plan) == (expect in (BIG, BIG_PW)), p.id
    three = [p.id for p in ALL_CONV if p.values[2].get("stages") == 3]
    assert sorted(three) == ["7x7_C64_49_taps_generic", "generic_3x3_C120_K1080_grid512_three_stages", "generic_3x3_C120_mode1", "pw_K1024_grid512_three_stages",
                             "tu_4x4_K1024_grid512_three_stages"]


def test_stride2_gradient_classes(lib):
    """even extents: four forward-geometry launches, R = 1 / 1 / 2 / 2 with K = C, 2C, 2C, 4C, each on the tap-uniform walk that honours the tap ->
    column-block map (the one-tap class: a plain gather through its pointer offset); odd extents: one nine-tap gather"""
    from tubedetr_amd import ops

    for pitch in (0, 64):  # the GPU test's two pitches
        (even, odd) = [conv_args(**dict(p.values[1], pitch=pitch)) for p in STRIDE2_GRAD]
        routes = ops.conv_gemm_route(*even, N_CU)
        C = even[0].C
        assert [(r.R, r.K, r.stride, r.mode, r.walk, r.stages) for r in routes] == [(1, C, 1, 0, GATHER, 2), (1, 2 * C, 1, 0, TU, 2), (2, 2 * C, 1, 0, TU, 2), (2, 4 * C, 1, 0, TU, 2)]
        routes = ops.conv_gemm_route(*odd, N_CU)
        assert [(r.R, r.K, r.stride, r.mode, r.walk) for r in routes] == [(3, 9 * C, 2, 1, GATHER)]


def linear_ex_args(M, Nn, dt, variant):
    """descriptor and epilogue of test_linear_ex_routes (test_gemm_routes_gpu.py)"""
    from tubedetr_amd import _hip

    K1 = 320
    shared, mapped, pitch = variant.startswith("shared"), "maps" in variant, 64 if variant.endswith("pitch") else 0
    rows1, rows2 = (M // 3 + 5, M // 2 + 3) if mapped else (M, M)
    x = _hip.LinearExDesc()
    x.M, x.N, x.K1, x.K2 = M, Nn, K1, K1
    x.lda1, x.lda2, x.ldc, x.ldr = K1, K1, Nn + pitch, Nn + 8
    x.w_shared = int(shared)
    x.rows1, x.rows2 = rows1, rows2
    if mapped:
        x.a1_map = x.a2_map = x.out_map = x.res_map = 16
    epi = _hip.Epilogue(PTR, PTR, PTR if variant.startswith("concat_maps_res_mask") else None, 1, 0, 0.1 if shared else 0.0, 4321, 1.0, None)
    return x, epi


@pytest.mark.parametrize("dt", [BF16, F32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("variant", ["concat_maps_res_mask", "concat_maps_res_mask_pitch", "shared_maps_dropout_pitch", "concat_identity_rows"])
@pytest.mark.parametrize("shape", LINEAR_EX, ids=[s[0] for s in LINEAR_EX])
def test_linear_ex_route(shape, variant, dt, lib):
    from tubedetr_amd import ops

    _, family, M, Nn = shape
    x, epi = linear_ex_args(M, Nn, dt, variant)
    routes = ops.linear_ex_route(x, True, epi, dt, N_CU)
    assert planned(routes) == [(family, 1 if dt == BF16 else 0, M, Nn, 640, 1, 1, 2)]
    (r,) = routes
    assert (r.kernel, r.walk, r.stages) == (KERNEL_TILED, GX, 2)
    check_grid(r)


# ------------------------------------------------------------------------------------------------
# argument checks: (id, message, descriptor fields changed from a valid call, epilogue fields, dtype code)
_OK_CONV = dict(N=1, Hs=4, Ws=4, C=8, Ho=4, Wo=4, R=1, S=1, stride=1, pad=0, mode=0, Nc=8, ldc=8, out_sp=1)
CONV_ERRORS = [
    ("null_pointer", "td_conv_gemm: null pointer", None, {}, 1),
    ("dtype", "td_conv_gemm: bad dtype 7", {}, {}, 7),
    ("channels", "td_conv_gemm: source channels C=3 must be a multiple of 8 (pad them)", dict(C=3), {}, 1),  # test_abi.py's case
    ("geometry", "td_conv_gemm: bad geometry", dict(Wo=0), {}, 1),
    ("source_elements", "td_conv_gemm: source tensor exceeds 2^31 elements", dict(N=4096, Hs=1024, Ws=1024), {}, 1),
    ("aniso", "td_conv_gemm: anisotropic stride / padding is a forward-only geometry", dict(aniso=1, stride_w=1, mode=1), {}, 1),
    ("descriptor_range", "td_conv_gemm: operand exceeds the 4 GiB buffer-descriptor range", dict(Hs=32768, Ws=4096, C=12), {}, 0),  # 1.6e9 fp32 elements
    ("dropout_p", "td_conv_gemm: dropout_p must be < 1", {}, dict(dropout_p=1.0), 1),
    ("ldc", "td_conv_gemm: ldc < Nc", dict(ldc=4), {}, 1),
]
_OK_LIN = dict(M=64, N=64, K1=64, K2=64, lda1=64, lda2=64, ldc=64, ldr=0, w_shared=0, rows1=64, rows2=64)
LINEAR_ERRORS = [  # ..., has_a2
    ("null_pointer", "td_linear_ex: null pointer", None, {}, 1, True),
    ("dtype", "td_linear_ex: bad dtype 7", {}, {}, 7, True),
    ("sizes", "td_linear_ex: bad sizes", dict(M=0), {}, 1, True),
    ("multiples", "td_linear_ex: K1 / K2 / lda must be multiples of 8", dict(lda1=68), {}, 1, True),
    ("k_tile", "td_linear_ex: with a second source K1=72 must be a multiple of the K tile (64)", dict(K1=72, lda1=72), {}, 1, True),
    ("row_stride", "td_linear_ex: row stride smaller than the row", dict(ldc=56), {}, 1, True),
    ("rows", "td_linear_ex: source has fewer rows than M and no row map", dict(rows2=63), {}, 1, True),
    ("shared_weight", "td_linear_ex: a shared weight needs K2 == K1", dict(w_shared=1, K2=128, lda2=128), {}, 1, True),
    ("descriptor_range", "td_linear_ex: operand exceeds the 4 GiB buffer-descriptor range", dict(rows1=1 << 26), {}, 0, False),
    ("dropout_p", "td_linear_ex: dropout_p must be < 1", {}, dict(dropout_p=1.5), 1, False),
]


def _epilogue(fields):
    from tubedetr_amd import _hip

    e = _hip.Epilogue(None, None, None, 0, 0, 0.0, 0, 1.0, None)
    for k, v in fields.items():
        setattr(e, k, v)
    return e


@pytest.mark.parametrize("message,change,epi,code", [c[1:] for c in CONV_ERRORS], ids=[c[0] for c in CONV_ERRORS])
def test_conv_argument_errors_match_the_launching_call(message, change, epi, code, lib):
    from tubedetr_amd import _hip

    d = None if change is None else _hip.ConvDesc(**dict(_OK_CONV, **change))
    dp = None if d is None else ctypes.byref(d)
    e = ctypes.byref(_epilogue(epi))
    rc_launch = lib.td_conv_gemm(PTR, PTR, PTR, dp, e, code, None)
    msg_launch = lib.td_last_error()
    routes, n = (_hip.GemmRoute * 4)(), ctypes.c_int(0)
    rc_query = lib.td_conv_gemm_route(dp, e, code, N_CU, routes, ctypes.byref(n))
    assert rc_launch != 0 and rc_query == rc_launch
    assert lib.td_last_error() == msg_launch == message.encode()


@pytest.mark.parametrize("message,change,epi,code,has_a2", [c[1:] for c in LINEAR_ERRORS], ids=[c[0] for c in LINEAR_ERRORS])
def test_linear_ex_argument_errors_match_the_launching_call(message, change, epi, code, has_a2, lib):
    from tubedetr_amd import _hip

    x = None
    if change is not None:
        x = _hip.LinearExDesc()
        for k, v in dict(_OK_LIN, **change).items():
            setattr(x, k, v)
    xp = None if x is None else ctypes.byref(x)
    e = ctypes.byref(_epilogue(epi))
    rc_launch = lib.td_linear_ex(PTR, PTR if has_a2 else None, PTR, PTR, xp, e, code, None)
    msg_launch = lib.td_last_error()
    routes, n = (_hip.GemmRoute * 4)(), ctypes.c_int(0)
    rc_query = lib.td_linear_ex_route(xp, int(has_a2), e, code, N_CU, routes, ctypes.byref(n))
    assert rc_launch != 0 and rc_query == rc_launch
    assert lib.td_last_error() == msg_launch == message.encode()


def test_every_family_is_planned_by_some_case():
    seen = {p.values[0] for p in ALL_CONV if isinstance(p.values[0], int)}
    assert seen == set(FAMILY)
