"""Every weight-gradient kernel, output mode and output path of csrc/conv_wgrad.hip against a plain float64 reference, BIT FOR BIT.

The operands come from a dyadic integer grid chosen so that every fp32 sum the kernels can form is exact in any order, inside an MFMA or as
an atomic (tests/wgrad_exact_ref.py states the condition and asserts it per case; test_wgrad_exact_cpu.py checks the reference against
autograd and pins, at 256 CUs, the route of every batched case).  One dropped reduction row, one wrong border tap, a missing zero fill under a
split job or a second accumulation is then a named element and two numbers, not a fraction of a tolerance.

  1  single launches: td_conv_wgrad_bias (out_mode 0, auto / 1 / 3 splits) and wgrad_finalize (plain, scaled, accumulating)
  2  ops.linear_wgrad with the bias gradient riding along, also on a column block of a wider gradient (ldg > Nc)
  3  ops.linear_wgrad_batch: bias epilogues (store / atomics), accumulating second phase on the 128 x 128 and the wide kernel, fills, M = 8
  4  ops.conv_wgrad_batch / td_conv_wgrad_batch: every reachable tile class, split and unsplit, padded stem channels
Outputs of the batched calls start as canaries with a guard row behind them."""
import ctypes as C
import functools

import pytest
import torch

import wgrad_exact_ref as X
from wgrad_plan_cases import (BF16, BLOCK_COL, BLOCK_LDG, EXACT_BATCH_CONVS, EXACT_CONV_ROUTES, EXACT_CONVS, EXACT_LINEAR_BATCH, EXACT_LINEAR_BLOCK,
                              EXACT_LINEAR_MIXED, EXACT_LINEAR_ROUTES, EXACT_PREZEROED, EXACT_LINEAR_SINGLE, EXACT_STEM_CI_REAL, F32, ROUTE_FIELDS, exact_conv_jobs,
                              exact_linear_jobs, exact_routes, wgrad_jobs)

pytestmark = pytest.mark.gpu

DT = [torch.bfloat16, torch.float32]
CODE = {torch.bfloat16: BF16, torch.float32: F32}
CANARY = 7.0
UNIT = 1.0 / 2 ** X.SHIFT


def dev():
    return torch.device("cuda:0")


@pytest.fixture(autouse=True)
def deterministic_flag_off():
    """every test starts with the split (atomic) reductions; the ones that switch the flag restore it themselves, this is the backstop"""
    import tubedetr_amd

    was = tubedetr_amd.is_deterministic()
    tubedetr_amd.set_deterministic(False)
    yield
    tubedetr_amd.set_deterministic(was)


def guarded(shape, start=None):
    """fp32 device tensor `shape` holding `start` (a CPU tensor, 0.0, or None = canaries) with one guard row of canaries right behind it"""
    n = 1
    for s in shape:
        n *= s
    buf = torch.full((n + max(shape[-1], 64),), CANARY, dtype=torch.float32, device=dev())
    out = buf[:n].view(shape)
    if start is not None:
        out.copy_(start) if torch.is_tensor(start) else out.fill_(start)
    return out, buf[n:]


def same(got, ref64, what, guard=None):
    """got (device fp32) holds exactly the float64 reference; ref64 -> fp32 is lossless under the exactness condition"""
    ref = ref64.to(torch.float32)
    assert torch.equal(ref.double(), ref64), f"{what}: the reference itself does not fit fp32"
    diff = X.first_difference(got, ref)
    assert diff is None, f"{what}: {diff}"
    if guard is not None:
        assert (guard == CANARY).all(), f"{what}: the guard row behind the output was written"


def product_grid(shape, seed, bound):
    """a value the output already holds: one more product of the grid (a multiple of 2^-8 bounded by bound^2 / 2^8), never zero"""
    t = X.grid_tensor(shape, torch.Generator().manual_seed(seed), bound * bound, 2 * X.SHIFT)
    return X.fill_zeros_(t, UNIT * UNIT)


def check_routes(specs, table, dt, det):
    """the plan of this batch on THIS device; skips if a job lands elsewhere than the CPU test pins for 256 CUs"""
    from tubedetr_amd import ops

    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    jobs, _ = ops.conv_wgrad_batch_plan(wgrad_jobs(specs), dt, n_cu, det)
    got = [tuple(getattr(j, f) for f in ROUTE_FIELDS) for j in jobs]
    want = exact_routes(table, CODE[dt], det)
    if got != want:
        pytest.skip(f"on {n_cu} CUs the batch is planned differently than on 256: job routes {[(i, g, w) for i, (g, w) in enumerate(zip(got, want)) if g != w]}")
    if det:
        assert all(j.splits == 1 for j in jobs)


# ------------------------------------------------------------------------------------------------
# 1. single launches
SINGLE = [(c, None) for c in EXACT_CONVS] + [(EXACT_CONVS[1], EXACT_STEM_CI_REAL)]


@functools.lru_cache(maxsize=None)
def single_case(cfg, ci_real):
    N, Ci, H, W, Co, R, stride, pad = cfg
    g, x, bound = X.conv_operands(cfg, seed=31, extra=1)  # + 1: wgrad_finalize accumulates onto one more grid value
    if ci_real is not None:
        x[..., ci_real:] = bound * UNIT  # padding channels: computed into dw_k, never read by wgrad_finalize
    ref = X.conv_wgrad_ref(g, x, R, R, stride, pad, ci_real)
    return g, x, bound, ref


# Explicit splits go through the C ABI (ops.conv_wgrad has no such argument).  With 3 asked for, rows per split are whole stages (64 bf16 /
# 32 fp32), so the five geometries (M = 112, 510, 429, 50, 63) run as
#   bf16: 64 + 48 | 192 + 192 + 126 | 192 + 192 + 45 | 50 | 63      fp32: 64 + 48 | 192 + 192 + 126 | 160 + 160 + 109 | 32 + 18 | 32 + 31
# i.e. the last split is ragged everywhere, shorter than one stage for M = 112, 429 (bf16), 50 and 63, and M = 50 / 63 are a single split
# shorter than one stage in bf16.
@pytest.mark.parametrize("splits", [0, 1, 3])
@pytest.mark.parametrize("dt", DT, ids=["bf16", "fp32"])
@pytest.mark.parametrize("cfg,ci_real", SINGLE, ids=[f"{c}-{ci}" for c, ci in SINGLE])
def test_single_launch_and_finalize(cfg, ci_real, dt, splits):
    from tubedetr_amd import _hip, ops

    N, Ci, H, W, Co, R, stride, pad = cfg
    g, x, bound, ref = single_case(cfg, ci_real)
    X.check_exactness_condition(X.conv_rows(cfg) + 1, bound, bound)
    gd, xd = g.to(dev(), dt), x.to(dev(), dt)
    dwk, dwk_guard = guarded((Co, R * R * Ci), 0.0)
    db, db_guard = guarded((Co,), 0.0)
    d = ops._desc(N, H, W, Ci, g.shape[1], g.shape[2], R, R, stride, pad, 0, Co, Co)
    _hip.check(_hip.lib().td_conv_wgrad_bias(_hip.ptr(gd), _hip.ptr(xd), _hip.ptr(dwk), _hip.ptr(db), C.byref(d), Co, _hip.dtype_code(dt), splits,
                                             _hip.stream_ptr()), "td_conv_wgrad_bias")
    shape = tuple(ref.shape)
    what = f"{cfg} ci_real={ci_real} {dt} splits={splits}"
    same(ops.wgrad_finalize(dwk, None, shape, Ci), ref, what + " finalize")
    scale = X.pow2_scale(Co)
    same(ops.wgrad_finalize(dwk, scale.to(dev()), shape, Ci), ref * scale.double().view(-1, 1, 1, 1), what + " finalize(scale)")
    start = product_grid(shape, 32, bound)
    out, out_guard = guarded(shape, start)
    ops.wgrad_finalize(dwk, None, shape, Ci, out=out, accumulate=True)
    same(out, ref + start.double(), what + " finalize(accumulate)", out_guard)
    same(db, g.double().sum((0, 1, 2)), what + " dbias", db_guard)
    assert (dwk_guard == CANARY).all(), what + ": the guard row behind dw_k was written"


# ------------------------------------------------------------------------------------------------
# 2. ops.linear_wgrad with dbias
LINEAR_SINGLE = [(s, False) for s in EXACT_LINEAR_SINGLE] + [(s, True) for s in EXACT_LINEAR_BLOCK]


@functools.lru_cache(maxsize=None)
def linear_single_case(M, K, Nn):
    g, x, bound = X.linear_operands(M, K, Nn, seed=41, M_total=M + 1)  # + 1: dW and dbias start from a grid value
    dW, db = X.linear_wgrad_ref(g, x)
    dW0 = product_grid((Nn, K), 42, bound)
    db0 = X.fill_zeros_(X.grid_tensor((Nn,), torch.Generator().manual_seed(43), bound), UNIT)
    return g, x, bound, dW0, db0, dW + dW0.double(), db + db0.double()


def column_block(g, bound, dt):
    """g as columns [BLOCK_COL : BLOCK_COL + Nc] of a BLOCK_LDG-wide device buffer whose other columns hold the largest grid value"""
    assert BLOCK_COL + g.shape[1] == BLOCK_LDG
    wide = torch.full((g.shape[0], BLOCK_LDG), bound * UNIT)
    wide[:, BLOCK_COL:] = g
    return wide.to(dev(), dt)[:, BLOCK_COL:]


@pytest.mark.parametrize("dt", DT, ids=["bf16", "fp32"])
@pytest.mark.parametrize("shape,block", LINEAR_SINGLE, ids=[f"{s}{'-block' if b else ''}" for s, b in LINEAR_SINGLE])
def test_linear_wgrad_adds_weight_and_bias_gradient(shape, block, dt):
    from tubedetr_amd import ops

    M, K, Nn = shape
    g, x, bound, dW0, db0, dW_ref, db_ref = linear_single_case(M, K, Nn)
    X.check_exactness_condition(M + 1, bound, bound)
    gd = column_block(g, bound, dt) if block else g.to(dev(), dt)
    assert gd.stride(0) == (BLOCK_LDG if block else Nn)
    dW, dW_guard = guarded((Nn, K), dW0)
    db, db_guard = guarded((Nn,), db0)
    ops.linear_wgrad(gd, x.to(dev(), dt), out=dW, dbias=db)
    same(dW, dW_ref, f"{shape} block={block} {dt} dW", dW_guard)
    same(db, db_ref, f"{shape} block={block} {dt} dbias", db_guard)


# ------------------------------------------------------------------------------------------------
# 3. ops.linear_wgrad_batch
@functools.lru_cache(maxsize=None)
def linear_batch_case():
    """per job of EXACT_LINEAR_BATCH: (g, x, bound); per overwriting job the references (dW incl. its accumulating partners, dbias)"""
    totals = X.linear_batch_totals(EXACT_LINEAR_BATCH)
    ops_, refs = [], {}
    for i, (M, K, Nn, block, bias, onto) in enumerate(EXACT_LINEAR_BATCH):
        if onto is None:
            g, x, bound = X.linear_operands(M, K, Nn, seed=50 + i, M_total=totals[i])
            dW, db = X.linear_wgrad_ref(g, x)
            refs[i] = [dW, db if bias else None]
        else:
            g, _, bound = ops_[onto]
            assert EXACT_LINEAR_BATCH[onto][:4] == (M, K, Nn, block) and totals[i] == totals[onto]
            x = X.activation_rows((M, K), torch.Generator().manual_seed(50 + i), bound)  # the second operand stream
            refs[onto][0] = refs[onto][0] + X.linear_wgrad_ref(g, x)[0]
        X.check_exactness_condition(totals[i], bound, bound)
        ops_.append((g, x, bound))
    return ops_, refs


def linear_batch_on_device(rows, dts):
    """rows: indices into EXACT_LINEAR_BATCH, dts: dtype per row -> (job tuples for ops.linear_wgrad_batch, outputs {row: (dW, guard, db, guard)})"""
    operands, _ = linear_batch_case()
    jobs, outs, gdev = [], {}, {}
    for i, dt in zip(rows, dts):
        M, K, Nn, block, bias, onto = EXACT_LINEAR_BATCH[i]
        g, x, bound = operands[i]
        if onto is None:
            gdev[i] = column_block(g, bound, dt) if block else g.to(dev(), dt)
            outs[i] = guarded((Nn, K)) + (guarded((Nn,)) if bias else (None, None))
            jobs.append((gdev[i], x.to(dev(), dt), outs[i][0].data_ptr(), outs[i][2].data_ptr() if bias else None))
        else:
            jobs.append((gdev[onto], x.to(dev(), dt), outs[onto][0].data_ptr(), None, True))
    return jobs, outs


def check_linear_outputs(outs, what):
    _, refs = linear_batch_case()
    for i, (dW, dW_guard, db, db_guard) in outs.items():
        same(dW, refs[i][0], f"{what} job {i} {EXACT_LINEAR_BATCH[i]} dW", dW_guard)
        if db is not None:
            same(db, refs[i][1], f"{what} job {i} {EXACT_LINEAR_BATCH[i]} dbias", db_guard)


@pytest.mark.parametrize("det", [False, True], ids=["split", "deterministic"])
@pytest.mark.parametrize("dt", DT, ids=["bf16", "fp32"])
def test_linear_wgrad_batch(dt, det):
    import tubedetr_amd
    from tubedetr_amd import ops

    was = tubedetr_amd.is_deterministic()
    try:
        tubedetr_amd.set_deterministic(det)
        check_routes(exact_linear_jobs(), EXACT_LINEAR_ROUTES, dt, det)
        jobs, outs = linear_batch_on_device(range(len(EXACT_LINEAR_BATCH)), [dt] * len(EXACT_LINEAR_BATCH))
        ops.linear_wgrad_batch(jobs)
        torch.cuda.synchronize()
        check_linear_outputs(outs, f"{dt} det={det} first call")
        first = {i: (o[0].clone(), None if o[2] is None else o[2].clone()) for i, o in outs.items()}
        ops.linear_wgrad_batch(jobs)  # the outputs now hold results, not canaries: split outputs are zero-filled again, nothing is added twice
        torch.cuda.synchronize()
    finally:
        tubedetr_amd.set_deterministic(was)
    check_linear_outputs(outs, f"{dt} det={det} second call")
    for i, o in outs.items():
        assert torch.equal(o[0], first[i][0]) and (o[2] is None or torch.equal(o[2], first[i][1])), f"job {i}: the second call gave other bits"


def test_linear_wgrad_batch_mixed_dtype_queue():
    """one fp32 job between bf16 jobs: launched per dtype, every result exact"""
    from tubedetr_amd import ops

    rows = [i for i, _ in EXACT_LINEAR_MIXED]
    dts = [torch.bfloat16 if code == BF16 else torch.float32 for _, code in EXACT_LINEAR_MIXED]
    jobs, outs = linear_batch_on_device(rows, dts)
    assert len({j[0].dtype for j in jobs}) == 2
    ops.linear_wgrad_batch(jobs)
    torch.cuda.synchronize()
    check_linear_outputs(outs, "mixed queue")


# ------------------------------------------------------------------------------------------------
# 4. ops.conv_wgrad_batch
@functools.lru_cache(maxsize=None)
def conv_batch_case(i):
    cfg, ci_real, _ = EXACT_BATCH_CONVS[i]
    N, Ci, H, W, Co, R, stride, pad = cfg
    g, x, bound = X.conv_operands(cfg, seed=70 + i)
    X.check_exactness_condition(X.conv_rows(cfg), bound, bound)
    if ci_real is not None:
        x[..., ci_real:] = bound * UNIT  # what the padding channels hold must not matter
    scale = X.pow2_scale(Co) if i % 2 == 0 else None
    return g, x, scale, X.conv_wgrad_ref(g, x, R, R, stride, pad, ci_real, scale)


def launch_conv_batch(arr, jobs, outputs, dt):
    """td_conv_wgrad_batch over the ctypes array `arr`, filled here from ops.conv_wgrad_batch-style job tuples and the dW tensors to write"""
    from tubedetr_amd import _hip, ops

    for a, (g, x, R, S, stride, pad, scale, ci_real), dW in zip(arr, jobs, outputs):
        N, H, W, Ci = x.shape
        _, Ho, Wo, Co = g.shape
        assert tuple(dW.shape) == (Co, ci_real, R, S)
        a.g, a.src, a.dW, a.scale, a.dbias = g.data_ptr(), x.data_ptr(), dW.data_ptr(), _hip.ptr(scale), None
        a.d = ops._desc(N, H, W, Ci, Ho, Wo, R, S, stride, pad, 0, Co, Co)
        a.ldg, a.ci_real = Co, ci_real
    nbytes = _hip.lib().td_conv_wgrad_batch_table_bytes(len(jobs))
    th, td_, done = ops.job_tables.take(nbytes, dev())
    _hip.check(_hip.lib().td_conv_wgrad_batch(arr, len(jobs), _hip.dtype_code(dt), th.data_ptr(), td_.data_ptr(), nbytes, _hip.stream_ptr()), "td_conv_wgrad_batch")
    done()


@pytest.mark.parametrize("dt", DT, ids=["bf16", "fp32"])
def test_prezeroed_split_jobs_add_into_the_callers_zeros(dt):
    """the trunk's form (td_resnet_bwd: one fill over a flat buffer of every dW): split jobs flagged `prezeroed` get no fill from the library and
    add their splits with atomics - on the 128 x 128 kernel and, in bf16, on the wide kernel"""
    from tubedetr_amd import _hip, ops

    rows = [i for i in EXACT_PREZEROED if dt == torch.bfloat16 or not EXACT_BATCH_CONVS[i][2]]
    jobs, refs, outs = [], [], []
    for i in rows:
        (N, Ci, H, W, Co, R, stride, pad), ci_real, _ = EXACT_BATCH_CONVS[i]
        g, x, scale, ref = conv_batch_case(i)
        jobs.append((g.to(dev(), dt), x.to(dev(), dt), R, R, stride, pad, None if scale is None else scale.to(dev()), Ci))
        refs.append(ref)
        outs.append(guarded(tuple(ref.shape), 0.0))
    arr = (_hip.WgradJob * len(jobs))()
    for a in arr:
        a.prezeroed = 1
    launch_conv_batch(arr, jobs, [o[0] for o in outs], dt)
    plan, _ = ops.conv_wgrad_batch_plan(arr, dt, torch.cuda.get_device_properties(0).multi_processor_count)
    assert all((p.splits > 1, p.out_mode, p.fill_dw, p.fill_dbias) == (True, 1, 0, 0) for p in plan)  # (at the 192-stage floor whatever the CU count)
    torch.cuda.synchronize()
    for i, (out, guard), ref in zip(rows, outs, refs):
        same(out, ref, f"{dt} prezeroed job {i} {EXACT_BATCH_CONVS[i][0]}", guard)


@pytest.mark.parametrize("det", [False, True], ids=["split", "deterministic"])
@pytest.mark.parametrize("dt", DT, ids=["bf16", "fp32"])
def test_conv_wgrad_batch(dt, det):
    import tubedetr_amd
    from tubedetr_amd import _hip, ops

    rows = [i for i, (_, _, bf16_only) in enumerate(EXACT_BATCH_CONVS) if dt == torch.bfloat16 or not bf16_only]
    assert len(rows) == len(exact_conv_jobs(CODE[dt]))
    jobs, refs = [], []
    for i in rows:
        (N, Ci, H, W, Co, R, stride, pad), ci_real, _ = EXACT_BATCH_CONVS[i]
        g, x, scale, ref = conv_batch_case(i)
        jobs.append((g.to(dev(), dt), x.to(dev(), dt), R, R, stride, pad, None if scale is None else scale.to(dev()), Ci if ci_real is None else ci_real))
        refs.append(ref)
    was = tubedetr_amd.is_deterministic()
    try:
        tubedetr_amd.set_deterministic(det)
        check_routes(exact_conv_jobs(CODE[dt]), EXACT_CONV_ROUTES, dt, det)
        outs = ops.conv_wgrad_batch(jobs)
        # once more through the C ABI, into canaried outputs with a guard row behind each
        mine = [guarded(tuple(ref.shape)) for ref in refs]
        launch_conv_batch((_hip.WgradJob * len(jobs))(), jobs, [m[0] for m in mine], dt)
        torch.cuda.synchronize()
    finally:
        tubedetr_amd.set_deterministic(was)
    for i, got, (canaried, guard), ref in zip(rows, outs, mine, refs):
        what = f"{dt} det={det} job {i} {EXACT_BATCH_CONVS[i][:2]}"
        same(got, ref, what + " (ops.conv_wgrad_batch)")
        same(canaried, ref, what + " (canaried output)", guard)
