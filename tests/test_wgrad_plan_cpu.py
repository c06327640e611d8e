"""How td_conv_wgrad_batch lays a call out on the device ("How a td_conv_wgrad_batch call is planned"), asserted without a GPU:
td_conv_wgrad_batch_plan runs the planner the launching call runs (csrc/wgrad_plan.h) and returns the plan.  Every job list of
tests/wgrad_plan_cases.py - the batches the GPU tests launch, a batch of linears with bias gradients and accumulating second-operand jobs, and
fp32 batches - is planned for 256 CUs, with and without the deterministic flag, and compared with

  recording   tests/golden/wgrad_plan.json: what the code before the planner existed put into its job tables, XCD indices and grids for the same
              lists (dumped once at its table-upload site; pointers excluded), field by field;
  invariants  what the kernels' indexing relies on (the binary search over first slots inside an XCD's table range), and the rules of the
              plan that can be stated without the recording.

Every argument check is reached once through the query and once through the launching call (which returns before anything is enqueued): same
code, same message.  (The launching call's own "job-table workspace" check has no counterpart: the query takes no table.)"""
import ctypes
import json
import os

import pytest

from wgrad_plan_cases import BF16, CASES, F32, conv_job, linear_job, wgrad_jobs

_knobs = sorted(k for k in os.environ if k.startswith("TD_WGRAD_"))
if _knobs:
    pytest.skip(f"weight-gradient knobs set in the environment ({', '.join(_knobs)}): the plans asserted here are the default ones", allow_module_level=True)

N_CU = 256
GENERAL, POINTWISE, WIDE = 0, 1, 2
JOB_FIELDS = ("phase", "kernel", "cls", "tn", "tk", "splits", "mper", "out_mode", "fill_dw", "fill_dbias", "xcd", "first")
LAUNCH_FIELDS = ("phase", "kernel", "n_jobs", "grid", "block", "item_stages")
PTR = ctypes.c_void_p(16)  # stands for a device pointer: the planner only tests it for NULL, the launching call returns before it is used


def cdiv(a, b):
    return -(-a // b)


@pytest.fixture(scope="module")
def lib():
    from tubedetr_amd import _hip
    from tubedetr_amd.build import build_lib

    build_lib(verbose=False)
    return _hip.lib()


@pytest.fixture(scope="module")
def recording():
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "wgrad_plan.json")) as f:
        return json.load(f)


def plan(name, det):
    import torch
    from tubedetr_amd import ops

    dt, specs = CASES[name]
    return ops.conv_wgrad_batch_plan(wgrad_jobs(specs), torch.bfloat16 if dt == BF16 else torch.float32, N_CU, det)


MODES = [pytest.param(False, id="split"), pytest.param(True, id="deterministic")]


@pytest.mark.parametrize("det", MODES)
@pytest.mark.parametrize("name", list(CASES))
def test_plan_equals_the_recording(name, det, lib, recording):
    jobs, launches = plan(name, det)
    want = recording[f"{name}/{'deterministic' if det else 'split'}"]
    assert len(jobs) == len(want["jobs"]) and len(launches) == len(want["launches"])
    for i, (j, w) in enumerate(zip(jobs, want["jobs"])):
        for f in JOB_FIELDS:
            assert getattr(j, f) == w[f], (i, f, getattr(j, f), w[f])
    for i, (l, w) in enumerate(zip(launches, want["launches"])):
        for f in LAUNCH_FIELDS:
            assert getattr(l, f) == w[f], (i, f, getattr(l, f), w[f])
        assert list(l.start) == w["start"] and list(l.slots) == w["slots"], i
    # the profiler's row of a phase: the sums over its launches (whole numbers well below 2^53: exact in any order)
    for w in want["phases"]:
        mine = [l for l in launches if l.phase == w["phase"]]
        assert sum(l.flops for l in mine) == w["flops"] and sum(l.bytes for l in mine) == w["bytes"], w


@pytest.mark.parametrize("det", MODES)
@pytest.mark.parametrize("name", list(CASES))
def test_plan_invariants(name, det, lib):
    dt, specs = CASES[name]
    jobs, launches = plan(name, det)
    mk = 64 if dt == BF16 else 32
    assert [(l.phase, l.kernel) for l in launches] == sorted({(j.phase, j.kernel) for j in jobs})  # launch order: phase, then kernel
    for l_idx, l in enumerate(launches):
        mine = sorted((j for j in jobs if j.launch == l_idx), key=lambda j: j.pos)
        assert all((j.phase, j.kernel) == (l.phase, l.kernel) for j in mine)
        assert [j.pos for j in mine] == list(range(l.n_jobs))  # every table row exactly once
        start, slots = list(l.start), list(l.slots)
        assert start[0] == 0 and start == sorted(start) and start[8] == l.n_jobs
        for x in range(8):
            rows = mine[start[x]:start[x + 1]]
            assert all(j.xcd == x for j in rows)
            at = 0  # the XCD's jobs tile [0, slots[x]) without gap or overlap, first slots ascending (the kernel's binary search)
            for j in rows:
                assert j.first == at, (l_idx, x, j.pos)
                at += j.tn * j.tk * j.splits
            assert at == slots[x]
        assert l.grid == 8 * max(slots) and l.block == (1024 if l.kernel == WIDE else 256)
        assert 192 <= l.item_stages <= 2048
    for j, s in zip(jobs, specs):
        M, K = s["N"] * s["Ho"] * s["Wo"], s["R"] * s["S"] * s["C"]
        assert j.phase == int(s["accumulate"])
        assert j.splits * j.mper >= M > (j.splits - 1) * j.mper and j.mper % mk == 0
        assert not det or j.splits == 1
        assert (j.out_mode == 2) == (j.splits == 1 and not s["accumulate"]) and j.out_mode in (1, 2)
        assert bool(j.fill_dw) == (j.splits > 1 and not s["accumulate"] and not s["prezeroed"])
        assert bool(j.fill_dbias) == (bool(j.fill_dw) and s["dbias"])
        pointwise = s["R"] * s["S"] == 1 and s["stride"] == 1 and s["pad"] == 0
        wide = (dt == BF16 and M >= 4096 and s["Nc"] % 128 == 0 and s["C"] % 128 == 0 and not s["dbias"] and s["R"] * s["S"] <= 255
                and (s["Nc"] % 256 == 0 or K >= 256))
        assert j.kernel == (WIDE if wide else POINTWISE if pointwise else GENERAL)
        gs, xs = (2 if s["Nc"] % 256 == 0 else 1, 2 if K >= 256 else 1) if wide else (1, 1)
        assert j.cls == ((gs - 1) | ((xs - 1) << 1) | (4 if pointwise else 0) if wide else 0)
        assert (j.tn, j.tk) == (cdiv(s["Nc"], gs * 128), cdiv(K, xs * 128))


def test_the_cases_reach_every_kernel_both_phases_and_both_fills(lib):
    seen, fills = set(), set()
    for name in CASES:
        jobs, _ = plan(name, False)
        seen |= {(j.phase, j.kernel) for j in jobs}
        fills |= {(j.fill_dw, j.fill_dbias, j.splits > 1) for j in jobs}
    assert seen >= {(0, GENERAL), (0, POINTWISE), (0, WIDE), (1, POINTWISE)}
    assert fills >= {(1, 1, True), (1, 0, True), (0, 0, True), (0, 0, False)}


# ------------------------------------------------------------------------------------------------
# argument checks: (id, message, dtype code, jobs, fields changed on the last job: descriptor fields by name, "null" = its dW pointer)
_OK = conv_job(1, 8, 4, 4, 8, 1, 1, 0)
_MANY = dict(N=1, Hs=1, Ws=1, C=256000, Ho=2048 * 32 * 101, Wo=1, R=1, S=1, stride=1, pad=0, Nc=128000, ldg=8, ci_real=256000, dbias=False, accumulate=False,
             prezeroed=False)  # fp32: 1000 x 2000 tiles x 101 splits of 2048 stages on one XCD
ERRORS = [
    ("no_jobs", "td_conv_wgrad_batch: no jobs", BF16, [], {}),
    ("null_pointer", "td_conv_wgrad_batch: job 1 has a null pointer", BF16, [_OK, _OK], dict(null=True)),
    ("dtype", "td_conv_wgrad_batch: bad dtype 7", 7, [_OK], {}),
    ("channels", "td_conv_wgrad_batch: source channels C=12 must be a multiple of 8 (pad them)", BF16, [_OK], dict(C=12, ci_real=12)),
    ("geometry", "td_conv_wgrad_batch: bad geometry", BF16, [_OK], dict(Wo=0)),
    ("source_elements", "td_conv_wgrad_batch: source tensor exceeds 2^31 elements", BF16, [_OK], dict(N=4096, Hs=1024, Ws=1024)),
    ("aniso_mode", "td_conv_wgrad_batch: anisotropic stride / padding is a forward-only geometry", BF16, [_OK], dict(aniso=1, stride_w=1, mode=1)),
    ("input_gradient_geometry", "td_conv_wgrad_batch: isotropic forward geometry expected", BF16, [_OK], dict(mode=1)),
    ("aniso", "td_conv_wgrad_batch: isotropic forward geometry expected", BF16, [_OK], dict(aniso=1, stride_w=1)),
    ("multiples", "td_conv_wgrad_batch: Nc=8 / ldg=12 must be multiples of 8", BF16, [_OK], dict(ldg=12)),
    ("descriptor_range", "td_conv_wgrad_batch: operand exceeds the 4 GiB buffer-descriptor range", BF16, [_OK], dict(Hs=1 << 20, Ws=1, Ho=1 << 20, Wo=1, ldg=4096)),
    ("ci_real", "td_conv_wgrad_batch: job 1: ci_real=0 out of range", BF16, [_OK, _OK], dict(ci_real=0)),
    ("ci_real_above_C", "td_conv_wgrad_batch: job 0: ci_real=9 out of range", BF16, [_OK], dict(ci_real=9)),
    ("accumulate_dbias", "td_conv_wgrad_batch: job 1: an accumulating job cannot carry a bias gradient", BF16, [_OK, _OK], dict(accumulate=True, dbias=True)),
    ("work_items", "td_conv_wgrad_batch: too many work items", F32, [_OK, _MANY], {}),
]


@pytest.mark.parametrize("message,code,specs,change", [c[1:] for c in ERRORS], ids=[c[0] for c in ERRORS])
def test_argument_errors_match_the_launching_call(message, code, specs, change, lib):
    from tubedetr_amd import _hip

    arr = wgrad_jobs(specs or [_OK])
    last = arr[len(arr) - 1]
    for k, v in change.items():
        if k == "null":
            last.dW = None
        elif k == "dbias":
            last.dbias = 16
        elif k in ("ldg", "ci_real", "accumulate"):
            setattr(last, k, int(v))
        else:
            setattr(last.d, k, v)
    n = len(specs)
    was = lib.td_get_deterministic()
    lib.td_set_deterministic(0)  # (the work-item cap is only reached by a split job)
    try:
        rc_launch = lib.td_conv_wgrad_batch(arr, n, code, PTR, PTR, ctypes.c_size_t(1 << 40), None)
        msg_launch = lib.td_last_error()
    finally:
        lib.td_set_deterministic(was)
    pj, pl, nl = (_hip.WgradPlanJob * len(arr))(), (_hip.WgradPlanLaunch * 6)(), ctypes.c_int(0)
    rc_query = lib.td_conv_wgrad_batch_plan(arr, n, code, N_CU, 0, pj, pl, ctypes.byref(nl))
    assert rc_launch != 0 and rc_query == rc_launch
    assert lib.td_last_error() == msg_launch == message.encode()


def test_single_launch_argument_checks(lib):
    """td_conv_wgrad's own argument checks are the planner's too (same helper, the call's name in the message)"""
    from tubedetr_amd import _hip

    d = _hip.ConvDesc(1, 4, 4, 8, 4, 4, 1, 1, 1, 0, 1, 8, 8, 1, 0, 0)  # input-gradient geometry
    rc = lib.td_conv_wgrad(PTR, PTR, PTR, ctypes.byref(d), 8, BF16, 0, None)
    assert rc != 0 and lib.td_last_error() == b"td_conv_wgrad: isotropic forward geometry expected"
    d.mode = 0
    rc = lib.td_conv_wgrad(PTR, PTR, PTR, ctypes.byref(d), 12, BF16, 0, None)
    assert rc != 0 and lib.td_last_error() == b"td_conv_wgrad: Nc=8 / ldg=12 must be multiples of 8"
