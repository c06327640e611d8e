"""The CPU side of the bit-exact weight-gradient tests (test_wgrad_exact_gpu.py): the plain float64 reference equals torch.autograd, every case
satisfies the condition under which fp32 sums are exact in any order (wgrad_exact_ref.py), grid values survive bf16, and every batched case
is planned - at 256 CUs, deterministic flag off and on - onto the kernel, tile class, split count, output mode, fills and phase its comment in
wgrad_plan_cases.py names, so that the GPU test cannot silently stop covering a route when the planner changes."""
import os

import pytest
import torch
import torch.nn.functional as F

import wgrad_exact_ref as X
from wgrad_plan_cases import (BF16, EXACT_BATCH_CONVS, EXACT_CONV_ROUTES, EXACT_CONVS, EXACT_LINEAR_BATCH, EXACT_LINEAR_BLOCK, EXACT_LINEAR_MIXED,
                              EXACT_LINEAR_ROUTES, EXACT_LINEAR_SINGLE, EXACT_PREZEROED, EXACT_STEM_CI_REAL, F32, ROUTE_FIELDS, exact_conv_jobs, exact_linear_jobs,
                              conv_job, exact_routes, wgrad_jobs)

N_CU = 256
GENERAL, POINTWISE, WIDE = 0, 1, 2
CONV_CASES = [(c, None) for c in EXACT_CONVS] + [(c, ci) for c, ci, _ in EXACT_BATCH_CONVS[len(EXACT_CONVS):]]


@pytest.mark.parametrize("cfg,ci_real", CONV_CASES, ids=[f"{c}-{ci}" for c, ci in CONV_CASES])
def test_reference_equals_autograd(cfg, ci_real):
    """float64 sums of these integers over 2^8 are exact in any order: the im2col reference and autograd agree to the bit"""
    N, Ci, H, W, Co, R, stride, pad = cfg
    g, x, _ = X.conv_operands(cfg, seed=5)
    scale = X.pow2_scale(Co)
    ref = X.conv_wgrad_ref(g, x, R, R, stride, pad, ci_real, scale)
    w = torch.zeros(Co, Ci, R, R, dtype=torch.float64, requires_grad=True)
    F.conv2d(x.permute(0, 3, 1, 2).double(), w, None, stride=stride, padding=pad).backward(g.permute(0, 3, 1, 2).double())
    want = (w.grad * scale.double().view(-1, 1, 1, 1))[:, :ci_real]
    assert ref.shape == (Co, Ci if ci_real is None else ci_real, R, R) and ref.dtype == torch.float64
    assert X.first_difference(ref, want) is None, X.first_difference(ref, want)
    # and the comparison the GPU tests make is lossless: the sums fit fp32
    assert torch.equal(ref.to(torch.float32).double(), ref)


def test_linear_reference_equals_autograd():
    g, x, _ = X.linear_operands(600, 256, 8, seed=6, M_total=601)
    dW, db = X.linear_wgrad_ref(g, x)
    w = torch.zeros(8, 256, dtype=torch.float64, requires_grad=True)
    b = torch.zeros(8, dtype=torch.float64, requires_grad=True)
    F.linear(x.double(), w, b).backward(g.double())
    assert torch.equal(dW, w.grad) and torch.equal(db, b.grad)


def test_every_case_satisfies_the_exactness_condition():
    """what the GPU tests draw their operands with (conv_operands / linear_operands pick the bound from the same totals)"""
    totals = [X.conv_rows(c) + 1 for c in EXACT_CONVS]                      # single launches: finalize accumulates onto one more grid value
    totals += [X.conv_rows(c) for c, _, _ in EXACT_BATCH_CONVS]
    totals += [M + 1 for M, _, _ in EXACT_LINEAR_SINGLE + EXACT_LINEAR_BLOCK]  # dW and dbias start from a grid value
    totals += X.linear_batch_totals(EXACT_LINEAR_BATCH)
    assert max(totals) == 34560 and X.linear_batch_totals(EXACT_LINEAR_BATCH)[5:7] == [25088, 25088]
    for m in totals:
        a = X.pick_bound(m)
        X.check_exactness_condition(m, a, a)
        X.check_exactness_condition(m, a, 1)  # column sums (dbias)
        assert a == 63 or m * (2 * a + 1) ** 2 >= 2 ** 24  # the largest grid of the ladder that fits
    assert [X.pick_bound(m) for m in (4096, 4227, 4228, 16384, 17459, 65536)] == [63, 63, 31, 31, 15, 15]
    with pytest.raises(AssertionError):
        X.check_exactness_condition(4228, 63, 63)
    with pytest.raises(AssertionError):
        X.check_exactness_condition(10, 128, 1)


def test_grid_tensors_survive_bf16_and_have_the_promised_shape():
    gen = torch.Generator().manual_seed(7)
    for bound in X.BOUNDS:
        t = X.grid_tensor((64, 257), gen, bound, X.SHIFT, 0.5)
        assert torch.equal(t.to(torch.bfloat16).to(torch.float32), t)
        assert t.abs().max() <= bound / 16 and torch.equal(t * 16, (t * 16).round())
        assert 0.45 < (t == 0).float().mean() < 0.55 + 0.5 / (2 * bound + 1)  # the zeroed half, and the zeros the draw itself gives
    assert X.grid_tensor((64, 64), gen, 63).abs().max() == 63 / 16  # (the bound itself is drawn)
    g, x, bound = X.conv_operands(EXACT_CONVS[0], seed=8)
    for t in (g, x):
        assert torch.equal(t.to(torch.bfloat16).to(torch.float32), t) and t.abs().max() <= bound / 16
    assert (g.view(-1, g.shape[-1])[[0, -1]] != 0).all() and (g > 0).any() and (g < 0).any() and (g != 0).float().mean() > 0.95
    assert (x[:, [0, -1]] != 0).all() and (x[:, :, [0, -1]] != 0).all() and 0.3 < (x == 0).float().mean() < 0.6
    g, x, _ = X.linear_operands(37, 768, 256, seed=9, M_total=38)
    assert (g[[0, -1]] != 0).all() and (x[[0, -1]] != 0).all() and 0.3 < (x == 0).float().mean() < 0.6
    sc = X.pow2_scale(6)
    assert sc.tolist() == [0.5, 1.0, 2.0, 4.0, 0.5, 1.0]


# ------------------------------------------------------------------------------------------------
_knobs = sorted(k for k in os.environ if k.startswith("TD_WGRAD_"))
needs_default_knobs = pytest.mark.skipif(bool(_knobs), reason=f"weight-gradient knobs set in the environment ({', '.join(_knobs)}): the routes pinned here are the default ones")


@pytest.fixture(scope="module")
def lib():
    from tubedetr_amd import _hip
    from tubedetr_amd.build import build_lib

    build_lib(verbose=False)
    return _hip.lib()


def routes(specs, dt, det):
    from tubedetr_amd import ops

    jobs, launches = ops.conv_wgrad_batch_plan(wgrad_jobs(specs), torch.bfloat16 if dt == BF16 else torch.float32, N_CU, det)
    return [tuple(getattr(j, f) for f in ROUTE_FIELDS) for j in jobs], launches


@needs_default_knobs
@pytest.mark.parametrize("det", [False, True], ids=["split", "deterministic"])
@pytest.mark.parametrize("dt", [BF16, F32], ids=["bf16", "fp32"])
def test_batched_cases_land_where_their_comments_say(dt, det, lib):
    got, _ = routes(exact_linear_jobs(), dt, det)
    assert got == exact_routes(EXACT_LINEAR_ROUTES, dt, det)
    got, _ = routes(exact_conv_jobs(dt), dt, det)
    assert got == exact_routes(EXACT_CONV_ROUTES, dt, det)
    if det:
        assert all(r[2] == 1 for r in got)


@needs_default_knobs
def test_the_exact_cases_reach_every_reachable_instance(lib):
    """kernel x phase x output mode x fill of the batched launches, and the wide classes.  Classes 0 and 4 (128 channels x 128 k columns) do
    not exist: the planner sends a job to the wide kernel only if Nc % 256 == 0 or K >= 256.  A wide job carries no bias (planner rule)."""
    lin, _ = routes(exact_linear_jobs(), BF16, False)
    conv, _ = routes(exact_conv_jobs(BF16), BF16, False)
    lin32, _ = routes(exact_linear_jobs(), F32, False)
    conv32, _ = routes(exact_conv_jobs(F32), F32, False)
    assert {r[1] for r in lin + conv if r[0] == WIDE} == {1, 2, 3, 5, 6, 7}
    kpm = lambda rs: {(r[0], r[6], r[3]) for r in rs}  # (kernel, phase, out_mode)
    assert kpm(lin + conv) == {(GENERAL, 0, 2), (GENERAL, 0, 1), (POINTWISE, 0, 2), (POINTWISE, 0, 1), (POINTWISE, 1, 1), (WIDE, 0, 2), (WIDE, 0, 1), (WIDE, 1, 1)}
    assert kpm(lin32 + conv32) == {(GENERAL, 0, 2), (GENERAL, 0, 1), (POINTWISE, 0, 2), (POINTWISE, 0, 1), (POINTWISE, 1, 1)}
    assert {(r[4], r[5]) for r in lin + conv} == {(0, 0), (1, 0), (1, 1)}
    # the wide kernel in phase 1: split (atomics from two workgroups per tile onto stored values) and unsplit
    assert {r[2] for r in lin if r[0] == WIDE and r[6] == 1} == {1, 2}
    # the mixed-dtype queue: per-dtype groups of jobs that all exist in the batch above
    assert {dt for _, dt in EXACT_LINEAR_MIXED} == {BF16, F32} and all(EXACT_LINEAR_BATCH[i][5] is None for i, _ in EXACT_LINEAR_MIXED)
    assert EXACT_BATCH_CONVS[len(EXACT_CONVS)][1] == EXACT_STEM_CI_REAL


@needs_default_knobs
def test_prezeroed_split_jobs_get_no_fill(lib):
    for dt in (BF16, F32):
        specs = [dict(conv_job(*EXACT_BATCH_CONVS[i][0]), prezeroed=True) for i in EXACT_PREZEROED if dt == BF16 or not EXACT_BATCH_CONVS[i][2]]
        got, _ = routes(specs, dt, False)
        assert got == ([(GENERAL, 0, 3, 1, 0, 0, 0), (WIDE, 3, 2, 1, 0, 0, 0)] if dt == BF16 else [(GENERAL, 0, 6, 1, 0, 0, 0)])
