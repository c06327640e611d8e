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
