"""Job lists of td_conv_wgrad_batch, one source for both sides: the GPU tests launch them (test_ops_gpu.py, test_bench_shapes_gpu.py), and
tests/test_wgrad_plan_cpu.py plans them without a GPU through td_conv_wgrad_batch_plan and compares the plan with tests/golden/wgrad_plan.json.

A job here is the geometry td_wgrad_job carries and nothing else (no tensor): conv jobs as ops.conv_wgrad_batch builds them, linear jobs as
ops.linear_wgrad_batch does."""
BF16, F32 = 1, 0

# (N, Cin, H, W, Cout, R, stride, pad): test_ops_gpu.py's per-op shapes ...
CONVS = [
    (2, 64, 12, 12, 64, 1, 1, 0),
    (3, 64, 11, 13, 256, 1, 1, 0),
    (2, 128, 14, 14, 128, 3, 1, 1),
    (2, 128, 15, 13, 128, 3, 2, 1),
    (2, 256, 9, 9, 512, 1, 2, 0),
    (2, 8, 30, 34, 64, 7, 2, 3),
    (1, 512, 6, 6, 2048, 1, 1, 0),
    (5, 256, 22, 22, 256, 3, 1, 1),
]
# ... and test_conv_wgrad_batch_matches_autograd's batch: the last two are long enough to split (> 512 stages of 64 rows)
AUTOGRAD_CFGS = CONVS + [(44, 64, 28, 28, 64, 1, 1, 0), (60, 64, 24, 24, 128, 3, 1, 1)]
STEM_PADDED = (2, 8, 30, 34, 64, 7, 2, 3)  # its second call: 3 real channels stored as 8 (ci_real = 3)

# test_conv_wgrad_batch_wide_tiles: M = 33 800 / 36 000 / 37 800 rows: split in two (atomics), the others unsplit
WIDE_CFGS = [(8, 128, 28, 27, 128, 3, 1, 1), (52, 256, 26, 25, 256, 3, 1, 1), (5, 1024, 30, 31, 256, 1, 1, 0), (40, 512, 30, 30, 128, 1, 1, 0),
             (6, 128, 28, 28, 512, 1, 1, 0), (8, 128, 57, 57, 128, 3, 2, 1), (2, 64, 12, 12, 64, 1, 1, 0), (3, 512, 40, 40, 512, 3, 1, 1),
             (50, 128, 28, 27, 128, 3, 1, 1)]

# test_trunk_weight_gradient_table_at_bench_shape: (Ci, H, W, Co, R, stride, pad) at TRUNK_FRAMES frames
TRUNK_FRAMES = 200
TRUNK_SHAPES = [(256, 88, 88, 128, 1, 1, 0), (128, 88, 88, 128, 3, 2, 1), (128, 44, 44, 512, 1, 1, 0), (256, 88, 88, 512, 1, 2, 0),
                (512, 44, 44, 128, 1, 1, 0), (128, 44, 44, 128, 3, 1, 1),
                (512, 44, 44, 256, 1, 1, 0), (256, 44, 44, 256, 3, 2, 1), (256, 22, 22, 1024, 1, 1, 0), (512, 44, 44, 1024, 1, 2, 0),
                (1024, 22, 22, 256, 1, 1, 0), (256, 22, 22, 256, 3, 1, 1),
                (1024, 22, 22, 512, 1, 1, 0), (512, 22, 22, 512, 3, 2, 1), (512, 11, 11, 2048, 1, 1, 0), (1024, 22, 22, 2048, 1, 2, 0),
                (2048, 11, 11, 512, 1, 1, 0), (512, 11, 11, 512, 3, 1, 1)]

# test_wide_weight_gradient_tiles_at_their_smallest_ragged_shapes: (Ci, H, Co, R, stride, pad) at RAGGED_FRAMES frames
RAGGED_FRAMES = 37
RAGGED_SHAPES = [(256, 22, 256, 3, 1, 1), (256, 22, 1024, 1, 1, 0), (1024, 22, 256, 1, 1, 0), (128, 44, 256, 3, 1, 1), (2048, 11, 512, 1, 1, 0)]


def conv_out(h, r, stride, pad):
    return (h + 2 * pad - r) // stride + 1


def conv_job(N, Ci, H, W, Co, R, stride, pad, ci_real=None):
    """the td_wgrad_job of ops.conv_wgrad_batch for one (g, x, R, S, stride, pad, scale, ci_real) entry"""
    return dict(N=N, Hs=H, Ws=W, C=Ci, Ho=conv_out(H, R, stride, pad), Wo=conv_out(W, R, stride, pad), R=R, S=R, stride=stride, pad=pad, Nc=Co,
                ldg=Co, ci_real=Ci if ci_real is None else ci_real, dbias=False, accumulate=False, prezeroed=False)


def linear_job(M, K, Nn, ldg=None, dbias=True, accumulate=False, prezeroed=False):
    """the td_wgrad_job of ops.linear_wgrad_batch for one (g [M, Nn] with row stride ldg, x [M, K]) entry"""
    return dict(N=1, Hs=M, Ws=1, C=K, Ho=M, Wo=1, R=1, S=1, stride=1, pad=0, Nc=Nn, ldg=Nn if ldg is None else ldg, ci_real=K, dbias=dbias,
                accumulate=accumulate, prezeroed=prezeroed)


# a deferred batch of the transformer's linears (functional._wgrad): bias gradients riding along, the Q/K projection's positional operand as
# an accumulating second job on a column block of a wider gradient (ldg > Nc), one caller-zeroed output, one M long enough to split
LINEARS = [linear_job(1600, 256, 256), linear_job(1600, 256, 512, ldg=768), linear_job(1600, 256, 512, ldg=768, dbias=False, accumulate=True),
           linear_job(1600, 256, 2048), linear_job(1600, 2048, 256), linear_job(60400, 256, 256, prezeroed=True), linear_job(60400, 256, 256),
           linear_job(60400, 256, 256, dbias=False, accumulate=True), linear_job(200, 768, 256), linear_job(8, 256, 8)]

# (dtype code, jobs) by name
CASES = {
    "ragged_37_frames": (BF16, [conv_job(RAGGED_FRAMES, Ci, H, H, Co, R, st, pad) for Ci, H, Co, R, st, pad in RAGGED_SHAPES]),
    "trunk_bench_shape": (BF16, [conv_job(TRUNK_FRAMES, *s) for s in TRUNK_SHAPES]),
    "wide_tiles": (BF16, [conv_job(*c) for c in WIDE_CFGS]),
    "autograd_bf16": (BF16, [conv_job(*c) for c in AUTOGRAD_CFGS]),
    "autograd_fp32": (F32, [conv_job(*c) for c in AUTOGRAD_CFGS]),
    "stem_padded_channels": (BF16, [conv_job(*STEM_PADDED, ci_real=3)]),
    "linears_dbias_accumulate": (BF16, LINEARS),
    "linears_fp32": (F32, LINEARS),
}


# ------------------------------------------------------------------------------------------------
# The bit-exact tests (test_wgrad_exact_gpu.py launches these on grid-valued operands, test_wgrad_exact_cpu.py pins their routes at 256 CUs).
# Not part of CASES: tests/golden/wgrad_plan.json is the recording of the lists above.

# single launches (td_conv_wgrad_bias, out_mode 0, then wgrad_finalize): stride-2 3x3, the 7x7 stem, pointwise, strided 1x1, and one with
# ragged Nc = 40 < 128 and K = 648 (last k tile part empty)
EXACT_CONVS = [(2, 128, 15, 13, 128, 3, 2, 1), (2, 8, 30, 34, 64, 7, 2, 3), (3, 64, 11, 13, 256, 1, 1, 0), (2, 256, 9, 9, 512, 1, 2, 0),
               (1, 72, 7, 9, 40, 3, 1, 1)]
EXACT_STEM_CI_REAL = 3  # EXACT_CONVS[1] once more with 3 real channels stored as 8

# one td_conv_wgrad_batch call: (geometry, ci_real or None, bf16 only).  The bf16-only jobs are the wide-tile ones (in fp32 they would only be
# larger jobs of the 128 x 128 instances the others reach already).
EXACT_BATCH_CONVS = [(c, None, False) for c in EXACT_CONVS] + [
    (EXACT_CONVS[1], EXACT_STEM_CI_REAL, False),      # padded stem: dW [64, 3, 7, 7]
    ((60, 64, 24, 24, 128, 3, 1, 1), None, False),    # M = 34 560: three splits (atomics + fill) on the 128 x 128 general instance
    ((5, 128, 29, 29, 128, 3, 1, 1), None, True),     # M = 4205, the fewest frames of 29 x 29 above the wide threshold: class 2 (128 x 256), K = 1152: last k tile half empty
    ((5, 256, 29, 29, 256, 3, 1, 1), None, True),     # class 3 (256 x 256)
    ((5, 1024, 29, 29, 256, 1, 1, 0), None, True),    # class 7 (pointwise 256 x 256)
    ((5, 128, 29, 29, 512, 1, 1, 0), None, True),     # class 5 (pointwise, 128 k columns)
    ((5, 128, 58, 58, 128, 3, 2, 1), None, True),     # class 2, stride 2
    ((26, 256, 22, 22, 256, 3, 1, 1), None, True),    # M = 12 584: class 3 split in two (atomics + fill)
    ((5, 256, 29, 29, 128, 1, 1, 0), None, True),     # class 6 (pointwise 128 x 256)
    ((5, 128, 58, 58, 256, 1, 2, 0), None, True),     # class 1 (256 x 128, not pointwise: a strided 1x1)
]

EXACT_PREZEROED = [6, 12]  # the two split jobs once more as a batch of their own, flagged `prezeroed`: no fill by the library, atomics into the caller's zeros

# ops.linear_wgrad (single launch, bias gradient riding along): (M, K, N)
EXACT_LINEAR_SINGLE = [(37, 768, 256), (600, 256, 8), (8, 256, 8), (3775, 256, 768)]
EXACT_LINEAR_BLOCK = [(37, 256, 512), (3775, 256, 512)]  # g = columns [256:768] of an [M, 768] buffer
BLOCK_LDG, BLOCK_COL = 768, 256

# one ops.linear_wgrad_batch call, small versions of LINEARS: (M, K, N, column block of a 768-wide gradient, bias, index of the job whose
# g and dW an accumulating job shares or None)
EXACT_LINEAR_BATCH = [
    (1600, 256, 256, False, True, None),
    (1600, 256, 512, True, True, None),    # ldg = 768 > Nc
    (1600, 256, 512, True, False, 1),      # its positional operand x2: phase 1, atomics onto what job 1 stored
    (200, 768, 256, False, True, None),
    (8, 256, 8, False, True, None),        # M = 8 < one stage, Nc = 8
    (12544, 256, 256, False, True, None),  # two splits (bf16) / three (fp32) at the 192-stage floor: dW and dbias filled, both written with atomics
    (12544, 256, 256, False, False, 5),    # bf16: wide class 7 in phase 1, two splits
    (4224, 128, 256, False, True, None),
    (4224, 128, 256, False, False, 7),     # bf16: wide class 5 (128 k columns) at its smallest M above the threshold
]
EXACT_LINEAR_MIXED = [(0, BF16), (3, F32), (4, BF16)]  # a mixed-dtype queue: (index into EXACT_LINEAR_BATCH, dtype code)


def exact_linear_jobs(rows=EXACT_LINEAR_BATCH):
    return [linear_job(M, K, Nn, ldg=BLOCK_LDG if block else None, dbias=bias, accumulate=onto is not None) for M, K, Nn, block, bias, onto in rows]


def exact_conv_jobs(dtype_code):
    return [conv_job(*c, ci_real=ci) for c, ci, bf16_only in EXACT_BATCH_CONVS if dtype_code == BF16 or not bf16_only]


# Where every job lands at 256 CUs with the deterministic flag off: (kernel, cls, splits, out_mode, fill_dw, fill_dbias, phase) per job, by
# dtype code.  Kernels: 0 general, 1 pointwise, 2 wide.  out_mode 2 = plain stores, 1 = atomics.
ROUTE_FIELDS = ("kernel", "cls", "splits", "out_mode", "fill_dw", "fill_dbias", "phase")
EXACT_LINEAR_ROUTES = {
    BF16: [(1, 0, 1, 2, 0, 0, 0), (1, 0, 1, 2, 0, 0, 0), (1, 0, 1, 1, 0, 0, 1), (1, 0, 1, 2, 0, 0, 0), (1, 0, 1, 2, 0, 0, 0),
           (1, 0, 2, 1, 1, 1, 0), (2, 7, 2, 1, 0, 0, 1), (1, 0, 1, 2, 0, 0, 0), (2, 5, 1, 1, 0, 0, 1)],
    F32: [(1, 0, 1, 2, 0, 0, 0), (1, 0, 1, 2, 0, 0, 0), (1, 0, 1, 1, 0, 0, 1), (1, 0, 1, 2, 0, 0, 0), (1, 0, 1, 2, 0, 0, 0),
          (1, 0, 3, 1, 1, 1, 0), (1, 0, 3, 1, 0, 0, 1), (1, 0, 1, 2, 0, 0, 0), (1, 0, 1, 1, 0, 0, 1)],
}
_SMALL = [(0, 0, 1, 2, 0, 0, 0), (0, 0, 1, 2, 0, 0, 0), (1, 0, 1, 2, 0, 0, 0), (0, 0, 1, 2, 0, 0, 0), (0, 0, 1, 2, 0, 0, 0), (0, 0, 1, 2, 0, 0, 0)]
EXACT_CONV_ROUTES = {
    BF16: _SMALL + [(0, 0, 3, 1, 1, 0, 0), (2, 2, 1, 2, 0, 0, 0), (2, 3, 1, 2, 0, 0, 0), (2, 7, 1, 2, 0, 0, 0), (2, 5, 1, 2, 0, 0, 0),
                    (2, 2, 1, 2, 0, 0, 0), (2, 3, 2, 1, 1, 0, 0), (2, 6, 1, 2, 0, 0, 0), (2, 1, 1, 2, 0, 0, 0)],
    F32: _SMALL + [(0, 0, 6, 1, 1, 0, 0)],
}


def deterministic_route(route):
    """the same job under the deterministic flag: one split; an overwriting job then owns its tiles (plain stores, nothing to fill)"""
    kernel, cls, splits, out_mode, fill_dw, fill_dbias, phase = route
    return (kernel, cls, 1, 1 if phase else 2, 0, 0, phase)


def exact_routes(table, dtype_code, det):
    return [deterministic_route(r) if det else r for r in table[dtype_code]]


def wgrad_jobs(specs, ptr=16):
    """ctypes array of td_wgrad_job for a list of job dicts; every pointer the job carries is `ptr` (only tested for NULL by the planner)"""
    from tubedetr_amd import _hip

    arr = (_hip.WgradJob * len(specs))()
    for a, s in zip(arr, specs):
        a.g = a.src = a.dW = ptr
        a.scale = None
        a.d = _hip.ConvDesc(s["N"], s["Hs"], s["Ws"], s["C"], s["Ho"], s["Wo"], s["R"], s["S"], s["stride"], s["pad"], 0, s["Nc"], s["Nc"], 1, 0, 0)
        a.ldg, a.ci_real = s["ldg"], s["ci_real"]
        a.dbias = ptr if s["dbias"] else None
        a.accumulate, a.prezeroed = int(s["accumulate"]), int(s["prezeroed"])
    return arr
