"""The dispatch-route cases of td_conv_gemm / td_linear_ex: tests/test_gemm_routes_cpu.py asserts the planned route of each through
td_conv_gemm_route / td_linear_ex_route (no GPU), tests/test_gemm_routes_gpu.py launches each and asserts the recorded route, the
values and the guard region.  A case is (expected family or list of recorded rows, run_conv keywords, plan): `plan` holds what the case
expects of the launch beyond the profiler's record - stages=, walk=, bn= - stated per case, not derived from the rule under test."""
import pytest
import torch

# TD_PROF_* of include/tubedetr_hip.h
T128, T128x64, T64, PERSIST, BIG, BIG_PW = 0, 1, 3, 4, 5, 6
FAMILY = {T128: "128x128", T128x64: "128x64", T64: "64x128", PERSIST: "persistent", BIG: "256-row", BIG_PW: "256-row pointwise"}
BF16, F32 = torch.bfloat16, torch.float32
# TD_GEMM_WALK_* (the operand walk of the launch)
PW, TU, GATHER, GX = 0, 1, 2, 3


def case(id_, expect, stages=None, walk=None, bn=None, **kw):
    plan = {k: v for k, v in (("stages", stages), ("walk", walk), ("bn", bn)) if v is not None}
    return pytest.param(expect, kw, plan, id=id_)


# ------------------------------------------------------------------------------------------------
# persistent weight-stationary instance (pw_resident2_kernel<NKT, RES, MSK>), bf16: needs cdiv(M, 64) >= 4 * 8 * (64 / (Nc / 128))
PERSISTENT = [
    case("Nc2048_K64_M8128_tiled", T64, M=8128, C=64, Nc=2048, relu=True, stages=2),
    case("Nc2048_K64_M8129", PERSIST, M=8129, C=64, Nc=2048, relu=True),
    case("Nc2048_K64_M8129_pitch", PERSIST, M=8129, C=64, Nc=2048, relu=True, pitch=64),
    case("Nc1024_K128_M16320_res_tiled", T64, M=16320, C=128, Nc=1024, res=True, relu=True, stages=2),
    case("Nc1024_K128_M16321_res", PERSIST, M=16321, C=128, Nc=1024, res=True, relu=True),
    case("Nc512_K192_M32704_mask_tiled", T64, M=32704, C=192, Nc=512, mask=True, stages=2),
    case("Nc512_K192_M32705_mask", PERSIST, M=32705, C=192, Nc=512, mask=True),
    case("Nc512_K256_M32705_res_mask_pitch", PERSIST, M=32705, C=256, Nc=512, res=True, mask=True, pitch=64, inplace=True),
    case("strided_1x1_forward_odd_extent", PERSIST, N=3, H=105, W=105, C=128, Nc=2048, stride=2, relu=True),
    case("mode1_stride1_res_mask", PERSIST, M=8129, C=64, Nc=2048, mode=1, bias=False, res=True, mask=True),
    case("dropout", PERSIST, M=8129, C=128, Nc=2048, res=True, drop=0.1),
    case("dropout_pitch", PERSIST, M=8129, C=128, Nc=2048, res=True, drop=0.1, pitch=64),
    # refusals: the same row counts on the tiled kernel
    case("refuse_Nc384", T64, M=33000, C=64, Nc=384, res=True, relu=True, stages=2),
    case("refuse_Nc768", T64, M=33000, C=64, Nc=768, mask=True, stages=2),
    case("refuse_K320", T64, M=32705, C=320, Nc=512, res=True, stages=2),
    case("refuse_alpha", T64, M=8129, C=64, Nc=2048, alpha=0.5, stages=2),
    case("refuse_sigmoid", T64, M=8129, C=64, Nc=2048, sigmoid=True, stages=2),
]

# ------------------------------------------------------------------------------------------------
# 256-row tiles, pointwise (conv_gemm_big8_kernel<false, RES> at Nc % 256 == 0, conv_gemm_big8n_kernel<false> otherwise), bf16:
# needs 512 <= K <= 64 * 154 and cdiv(M, 256) * (Nc / (256 or 128)) >= 160
BIG_POINTWISE = [
    case("Nc2048_K512_M4864_tiled", T64, M=4864, C=512, Nc=2048, relu=True, stages=2),
    case("Nc2048_K512_M4865", BIG_PW, M=4865, C=512, Nc=2048, relu=True, bn=256),
    case("Nc2048_K512_M4865_pitch", BIG_PW, M=4865, C=512, Nc=2048, relu=True, pitch=64, bn=256),
    case("Nc256_K512_M40704_res_tiled", T64, M=40704, C=512, Nc=256, res=True, relu=True, stages=2),
    case("Nc256_K512_M40705_res_inplace", BIG_PW, M=40705, C=512, Nc=256, res=True, relu=True, inplace=True, bn=256),
    case("Nc384_K576_M13568_res_tiled", T64, M=13568, C=576, Nc=384, res=True, stages=2),
    case("Nc384_K576_M13569_res", BIG_PW, M=13569, C=576, Nc=384, res=True, pitch=64, inplace=True, bn=128),  # 128 wide, three column tiles
    case("Nc128_K512_M40705_mask", BIG_PW, M=40705, C=512, Nc=128, mask=True, bn=128),
    case("Nc2048_M4865_res_mask", BIG_PW, M=4865, C=640, Nc=2048, res=True, mask=True, bn=256),
    case("K448_tiled", T64, M=4865, C=448, Nc=2048, relu=True, stages=2),
    case("K9856_last_table_entry", BIG_PW, M=4865, C=9856, Nc=2048, relu=True, bn=256),
    case("K9920_tiled_128x128", T128, M=4865, C=9920, Nc=2048, relu=True, stages=2),
    case("dropout_falls_back_to_tiles", T64, M=4865, C=512, Nc=2048, drop=0.1, stages=2),
    case("dropout_falls_back_to_tiles_pitch", T64, M=4865, C=512, Nc=2048, drop=0.1, pitch=64, stages=2),
    case("dropout_falls_back_to_tiles_K576", T128, M=4865, C=576, Nc=2048, drop=0.1, pitch=64, stages=2),
]

# ------------------------------------------------------------------------------------------------
# 256-row tiles, tap-uniform walk (conv_gemm_big8_kernel<true, RES> / conv_gemm_big8n_kernel<true>): at most 32 taps, C % 64 == 0.
# Nc = 1024: four column tiles, cdiv(M, 256) >= 40 from M = 9985; Nc = 512: M >= 20225.  3 x 59 x 58 = 10266 rows, ragged last tile.
_OUT = dict(N=3, Nc=1024)
BIG_TAP_UNIFORM = [
    case("3x3_s1", BIG, N=5, H=65, W=63, C=64, Nc=512, R=3, S=3, pad=1, relu=True, bn=256),
    case("3x3_s1_pitch", BIG, N=5, H=65, W=63, C=64, Nc=512, R=3, S=3, pad=1, relu=True, pitch=64, bn=256),
    case("3x3_s2", BIG, H=117, W=115, C=64, R=3, S=3, stride=2, pad=1, relu=True, bn=256, **_OUT),
    case("5x5", BIG, H=59, W=58, C=64, R=5, S=5, pad=2, relu=True, bn=256, **_OUT),
    case("1x3", BIG, H=57, W=58, C=192, R=1, S=3, pad=1, bn=256, **_OUT),
    case("3x1", BIG, H=59, W=56, C=192, R=3, S=1, pad=1, bn=256, **_OUT),
    case("3x3_pad0", BIG, H=61, W=60, C=64, R=3, S=3, pad=0, bn=256, **_OUT),
    case("3x3_pad2", BIG, H=57, W=56, C=64, R=3, S=3, pad=2, res=True, bn=256, **_OUT),
    case("3x3_C1088_K9792", BIG, H=59, W=58, C=1088, R=3, S=3, pad=1, bn=256, **_OUT),
    case("3x3_C1152_K10368_tiled", T128, H=59, W=58, C=1152, R=3, S=3, pad=1, stages=2, **_OUT),
    case("3x3_rows_below_threshold_tiled", T128, H=59, W=56, C=64, R=3, S=3, pad=1, stages=2, **_OUT),  # 9912 rows: 39 row tiles x 4 = 156 workgroups
    case("3x3_mode1_res_mask", BIG, H=59, W=58, C=64, R=3, S=3, pad=1, mode=1, bias=False, res=True, mask=True, bn=256, **_OUT),
    case("5x5_mode1_res_mask", BIG, H=59, W=58, C=64, R=5, S=5, pad=2, mode=1, bias=False, res=True, mask=True, pitch=64, inplace=True, bn=256, **_OUT),
    case("1x3_mode1_res_mask", BIG, H=59, W=58, C=192, R=1, S=3, pad=1, mode=1, bias=False, res=True, mask=True, bn=256, **_OUT),
]

# ------------------------------------------------------------------------------------------------
# tiled kernel (conv_gemm_kernel): 128x64 tiles at Nc <= 64; else 64x128 when cdiv(M, 128) * cdiv(Nc, 128) < 512 or K <= 512; else 128x128.
# Nc = 120 (one column tile, no multiple of 128: the persistent and 256-row routes refuse bf16 launches) stands on 511 / 512 tiles exactly:
# M = 65408 and 65409; Nc = 776 (seven column tiles) adds 73 x 7 = 511 against 74 x 7 = 518.
# Scalar epilogue (vec_ok false): ldc no multiple of 16 bytes (bf16: ldc % 8, fp32: ldc % 4) or a ragged last 16 bytes - bf16 Nc = 1, 2, 4, 100,
# 12 at ldc = 76, 65; fp32 Nc = 1, 2, 6, 101, 65 at ldc = 129 (fp32 Nc = 4, 12, 100 at ldc = Nc take the vector epilogue).
# Stage count (stages=; the profiler does not record it): three when the 64x128 grid 8 * cdiv(cdiv(M, 64), 8) * cdiv(Nc, 128) <= 512 and
# K >= 1024, bf16 only.  Nc = 128: grid 512 up to M = 32768 = 8 x 64 x 64, grid 520 at 8 x 64 x 65 rows; 128 / 130 workgroups of 256 rows stay
# below the 256-row route.
_SQ = dict(N=8, Nc=128)
TILED = [
    case("Nc64_narrow", T128x64, M=1000, C=128, Nc=64, res=True, relu=True, stages=2),
    case("Nc64_narrow_pitch", T128x64, M=1000, C=128, Nc=64, res=True, relu=True, pitch=64, stages=2),
    case("Nc65", T64, M=1000, C=128, Nc=65, res=True, relu=True, stages=2),
    case("Nc1", T128x64, M=777, C=96, Nc=1, res=True, relu=True, stages=2),
    case("Nc2", T128x64, M=777, C=96, Nc=2, mask=True, stages=2),
    case("Nc4_sigmoid", T128x64, M=777, C=96, Nc=4, sigmoid=True, stages=2),
    case("Nc4", T128x64, M=777, C=96, Nc=4, res=True, mask=True, stages=2),
    case("Nc12", T128x64, M=777, C=96, Nc=12, res=True, relu=True, pitch=64, stages=2),
    case("Nc100", T64, M=777, C=96, Nc=100, res=True, relu=True, stages=2),
    case("Nc100_dropout", T64, M=777, C=96, Nc=100, drop=0.25, stages=2),
    case("Nc100_dropout_pitch", T64, M=777, C=96, Nc=100, drop=0.25, pitch=64, stages=2),  # scalar epilogue, key m * 164 + n
    case("Nc256_dropout_pitch", T64, M=777, C=96, Nc=256, res=True, drop=0.25, pitch=64, stages=2),  # vector epilogue on 64x128 tiles
    case("Nc64_dropout_pitch", T128x64, M=1000, C=128, Nc=64, res=True, drop=0.25, pitch=64, stages=2),  # 128x64 tiles
    case("tiles128_511_exact_K576", T64, M=65408, C=576, Nc=120, relu=True, stages=2),
    case("tiles128_512_exact_K576", T128, M=65409, C=576, Nc=120, relu=True, stages=2),
    case("tiles128_511_K576", T64, M=9344, C=576, Nc=776, relu=True, stages=2),
    case("tiles128_518_K576", T128, M=9345, C=576, Nc=776, relu=True, stages=2),
    case("tiles128_518_K576_pitch", T128, M=9345, C=576, Nc=776, res=True, mask=True, pitch=64, stages=2),
    case("tiles128_518_K512", T64, M=9345, C=512, Nc=776, relu=True, stages=2),
    # two against three stages: pointwise, tap-uniform, generic gather
    case("pw_K960_grid512", T64, M=32768, C=960, Nc=128, relu=True, stages=2, walk=PW),
    case("pw_K1024_grid512_three_stages", T64, M=32768, C=1024, Nc=128, relu=True, stages=3, walk=PW),
    case("pw_K1024_grid520", T64, M=32769, C=1024, Nc=128, relu=True, stages=2, walk=PW),
    case("tu_3x5_K960_grid512", T64, H=64, W=66, C=64, R=3, S=5, pad=1, stages=2, walk=TU, **_SQ),
    case("tu_4x4_K1024_grid512_three_stages", T64, H=65, W=65, C=64, R=4, S=4, pad=1, res=True, relu=True, stages=3, walk=TU, **_SQ),
    case("tu_4x4_K1024_grid520", T64, H=65, W=66, C=64, R=4, S=4, pad=1, stages=2, walk=TU, **_SQ),
    case("generic_3x3_C104_K936_grid512", T64, H=64, W=64, C=104, R=3, S=3, pad=1, stages=2, walk=GATHER, **_SQ),
    case("generic_3x3_C120_K1080_grid512_three_stages", T64, H=64, W=64, C=120, R=3, S=3, pad=1, res=True, relu=True, stages=3, walk=GATHER, **_SQ),
    case("generic_3x3_C120_K1080_grid520", T64, H=64, W=65, C=120, R=3, S=3, pad=1, stages=2, walk=GATHER, **_SQ),
    case("generic_3x3_C120_mode1", T64, H=64, W=64, C=120, R=3, S=3, pad=1, mode=1, bias=False, res=True, mask=True, stages=3, walk=GATHER, **_SQ),  # the shape of the case above: three stages in mode 1 too
    case("7x7_C64_49_taps_generic", T64, N=2, H=30, W=30, C=64, Nc=128, R=7, S=7, pad=3, relu=True, stages=3, walk=GATHER),  # 32 workgroups, K = 3136: three stages
    case("M1", T64, M=1, C=128, Nc=256, res=True, stages=2),
    case("M63", T64, M=63, C=128, Nc=256, res=True, pitch=64, stages=2),
    case("M65", T64, M=65, C=128, Nc=256, mask=True, stages=2),
]
TILED_FP32 = [
    case("fp32_tap_uniform_C96", T64, dt=F32, N=2, H=20, W=21, C=96, Nc=128, R=3, S=3, pad=1, relu=True, stages=2, walk=TU),
    case("fp32_tap_uniform_C96_s2", T64, dt=F32, N=2, H=21, W=23, C=96, Nc=128, R=3, S=3, stride=2, pad=1, res=True, stages=2, walk=TU),
    case("fp32_Nc64_narrow", T128x64, dt=F32, M=1000, C=128, Nc=64, res=True, relu=True, stages=2),
    case("fp32_Nc65", T64, dt=F32, M=1000, C=128, Nc=65, res=True, relu=True, pitch=64, stages=2),
    case("fp32_Nc1", T128x64, dt=F32, M=777, C=100, Nc=1, res=True, relu=True, stages=2),
    case("fp32_Nc2", T128x64, dt=F32, M=777, C=100, Nc=2, mask=True, stages=2),
    case("fp32_Nc4", T128x64, dt=F32, M=777, C=100, Nc=4, res=True, mask=True, stages=2),
    case("fp32_Nc12", T128x64, dt=F32, M=777, C=100, Nc=12, res=True, relu=True, stages=2),
    case("fp32_Nc100", T64, dt=F32, M=777, C=100, Nc=100, res=True, relu=True, stages=2),
    case("fp32_Nc6_scalar", T128x64, dt=F32, M=777, C=100, Nc=6, res=True, mask=True, stages=2),
    case("fp32_Nc101_scalar", T64, dt=F32, M=777, C=100, Nc=101, res=True, relu=True, stages=2),
    case("fp32_Nc101_scalar_dropout_pitch", T64, dt=F32, M=777, C=100, Nc=101, drop=0.25, pitch=64, stages=2),
    case("fp32_tiles128_511_exact_K576", T64, dt=F32, M=65408, C=576, Nc=120, relu=True, stages=2),
    case("fp32_tiles128_512_exact_K576", T128, dt=F32, M=65409, C=576, Nc=120, res=True, relu=True, stages=2),
    case("fp32_tiles128_511_K576", T64, dt=F32, M=9344, C=576, Nc=776, relu=True, stages=2),
    case("fp32_tiles128_518_K576", T128, dt=F32, M=9345, C=576, Nc=776, res=True, relu=True, stages=2),
    case("fp32_tiles128_518_K512", T64, dt=F32, M=9345, C=512, Nc=776, relu=True, stages=2),
    case("fp32_7x7_C64", T64, dt=F32, N=2, H=30, W=30, C=64, Nc=128, R=7, S=7, pad=3, relu=True, stages=2, walk=GATHER),
    case("fp32_M1", T64, dt=F32, M=1, C=128, Nc=256, res=True, stages=2),
    case("fp32_M63", T64, dt=F32, M=63, C=128, Nc=256, res=True, stages=2),
    case("fp32_M65", T64, dt=F32, M=65, C=128, Nc=256, mask=True, pitch=64, stages=2),
]

# ------------------------------------------------------------------------------------------------
# (double)M * ldc < 2 147 483 000 admits the routes with 32-bit output offsets: Nc = 2048, K = 64 is the persistent instance's shape
OFFSET_EDGE = [
    case("M1048575_below_persistent", PERSIST, M=1048575, C=64, Nc=2048, relu=True),
    case("M1048600_above_tiled", T64, M=1048600, C=64, Nc=2048, relu=True, stages=2),
]

# ------------------------------------------------------------------------------------------------
# input gradient of a 3x3 / stride 2 / pad 1 convolution: four parity-class launches on even extents, one gather otherwise
# forward layer: Nc -> C channels; g [N, 12, 10, C] -> dx [N, H, W, Nc]
_S2 = dict(N=3, C=64, Nc=128, R=3, S=3, stride=2, pad=1, mode=1, bias=False, res=True, mask=True)
STRIDE2_GRAD = [
    case("even_extent_four_launches", [(T64, 1, 3 * 12 * 10, 128, taps * 64, r, 1, 0) for r, taps in ((1, 1), (1, 2), (2, 2), (2, 4))], H=24, W=20, **_S2),
    case("odd_extent_one_launch", [(T64, 1, 3 * 23 * 19, 128, 9 * 64, 3, 2, 1)], H=23, W=19, walk=GATHER, **_S2),
]

# ------------------------------------------------------------------------------------------------
# td_linear_ex (the GX instances of conv_gemm_kernel): K1 = K2 = 320
LINEAR_EX = [  # id, family, M, N
    ("128x128", T128, 8192, 1024),
    ("64x128", T64, 512, 1024),
    ("128x64", T128x64, 512, 48),
]
