"""The cases of tests/optim_guard_ref.py are well posed (no GPU): every mutant of the guard's rules changes the outcome of at
least one of them, which is the proof that tests/test_optim_guard_gpu.py - the same cases on the kernels - can fail.  Also
here: the layout of td_step_record and of the guard block, and the host-side argument checks of the two guarded entry
points, which return an error code and a message before any launch."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import optim_guard_ref as G
import optim_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def outcomes():
    """The reference's outcome of every case, computed once."""
    cases = G.cpu_cases()
    return cases, {name: G.run(**kw) for name, kw in cases.items()}


def test_reference_on_the_cases(outcomes):
    cases, ref = outcomes
    for name, out in ref.items():
        kw = cases[name]
        p, m, v, ema = (x.astype(np.float64) for x in kw["state"])
        if name.startswith("finite"):
            assert (out["attempts"], out["skipped"], out["consecutive_skipped"], out["applied_now"]) == (1, 0, 0, 1), name
            assert out["step"] == kw["step0"] + 1 and out["clip"] > 0 and not np.array_equal(out["ema"], ema), name
        elif name.startswith("bad") or name == "fp32 norm overflow":
            assert (out["attempts"], out["skipped"], out["consecutive_skipped"], out["applied_now"]) == (1, 1, 1, 0), name
            assert out["step"] == kw["step0"] and out["clip"] == 0 and not np.isfinite(G.to_f32(out["norm"])), name
            for k, x in zip(("param", "exp_avg", "exp_avg_sq", "ema"), (p, m, v, ema)):
                assert np.array_equal(out[k], x), (name, k)
    assert np.isfinite(ref["fp32 norm overflow"]["norm"])  # ... finite in float64: only the fp32 norm overflows
    assert all(np.isfinite(g[R.seg_arrays(len(g), outcomes[0]["fp32 norm overflow"]["segs"])[1]]).all() for g, _ in outcomes[0]["fp32 norm overflow"]["attempts"])
    seq = ref["sequence"]
    assert (seq["attempts"], seq["skipped"], seq["consecutive_skipped"], seq["step"]) == (4, 2, 0, 2)
    assert [r["applied"] for r in seq["ring"][:4]] == [1, 0, 0, 1] and seq["ring"][4:] == [None] * 4
    assert [r["step"] for r in seq["ring"][:4]] == [1, 1, 1, 2]
    losses = [r["loss"] for r in seq["ring"][:4]]
    assert losses[0] == 2.5 and np.isnan(losses[1]) and np.isnan(losses[2]) and losses[3] == float("inf")
    wrap = ref["ring wrap"]
    assert [r["attempt"] for r in wrap["ring"]] == [5, 6, 3, 4] and (wrap["attempts"], wrap["skipped"], wrap["consecutive_skipped"]) == (6, 2, 0)
    assert ref["history 0"]["ring"] == [] and ref["history 0"]["attempts"] == 6


@pytest.mark.parametrize("mut", list(G.MUTANTS))
def test_every_mutant_is_told_apart(outcomes, mut):
    cases, ref = outcomes
    apart = [name for name, kw in cases.items() if not G.same_outcome(G.run(**kw, mut=mut), ref[name])]
    print(mut, "->", len(apart), "cases, e.g.", apart[:3])
    assert apart, f"no case tells {mut} ({G.MUTANTS[mut]}) from the reference"
    # ... and by the kind of case that is meant to catch it
    kind = {"step_incremented_on_skip": "bad", "ema_moves_on_skip": "bad", "moments_updated_on_skip": "bad", "inactive_nonfinite_counts": "finite",
            "consecutive_not_reset": "sequence", "ring_index_off_by_one": "ring wrap", "loss_decides": "sequence"}[mut]
    assert any(name.startswith(kind) for name in apart), (mut, apart)


def test_the_reference_equals_itself(outcomes):
    cases, ref = outcomes
    for name in ("sequence", "ring wrap", "bad nan at straddle[5]"):
        assert G.same_outcome(G.run(**cases[name]), ref[name])


def test_record_comparison_can_fail(outcomes):
    want = outcomes[1]["sequence"]["ring"][0]
    got = dict(want, norm=float(np.float32(want["norm"])), clip=float(np.float32(want["clip"])), group_norm=[float(np.float32(x)) for x in want["group_norm"]])
    assert G.record_mismatch(got, want) is None
    g2 = list(got["group_norm"])
    g2[1] = float(np.nextafter(np.nextafter(np.float32(g2[1]), np.float32(np.inf)), np.float32(np.inf)))  # two ulps off
    for bad in (dict(got, step=got["step"] + 1), dict(got, loss=float("nan")), dict(got, norm=got["norm"] * (1 + 3e-6)), dict(got, group_norm=g2),
                dict(got, applied=0)):
        assert G.record_mismatch(bad, want) is not None


# ------------------------------------------------------------------------------------------------------------- layouts
def test_step_record_mirror_and_sizes():
    from tubedetr_amd import _hip

    src = open(os.path.join(ROOT, "include", "tubedetr_hip.h")).read()
    flat = " ".join(re.sub(r"/\*.*?\*/", "", src, flags=re.S).split())
    body = re.search(r"typedef struct td_step_record \{(.*?)\} td_step_record;", flat).group(1)
    fields = [d.strip() for d in body.split(";") if d.strip()]
    assert len(fields) == len(_hip.StepRecord._fields_) == 7
    assert [f.split()[-1].split("[")[0] for f in fields] == [n for n, _ in _hip.StepRecord._fields_]
    assert C.sizeof(_hip.StepRecord) == G.RECORD_BYTES == 40
    assert int(re.search(r"#define TD_GUARD_HISTORY_MAX (\d+)", src).group(1)) == _hip.TD_GUARD_HISTORY_MAX == G.HISTORY_MAX
    assert int(re.search(r"#define TD_OPTIM_MAX_GROUPS (\d+)", src).group(1)) == _hip.TD_OPTIM_MAX_GROUPS == G.GROUPS
    L = _hip.lib()
    for h in (0, 1, 8, 64, 4096):
        assert L.td_guard_bytes(h) == G.HEADER_BYTES + G.RECORD_BYTES * h
    assert L.td_grad_norm_guard_ws_bytes() >= L.td_grad_norm_ws_bytes()
    assert L.td_grad_norm_guard_ws_bytes() == (1 + G.GROUPS) * L.td_grad_norm_ws_bytes()  # the total and one row per group
    assert L.td_abi_version() == 11  # additions only


def test_snapshot_decoding():
    """FusedAdamWEMA's decoding of a guard block (pure host code): counters, newest record, ring oldest first."""
    from tubedetr_amd import _hip
    from tubedetr_amd.optim import _decode_guard

    def block(attempts, skipped, consecutive, history, written):
        raw = bytearray(16 + 40 * history)
        raw[:16] = bytes((C.c_int * 4)(attempts, skipped, consecutive, 0))
        for a in written:
            r = _hip.StepRecord(a, a - 1, a % 2, 1.5, 0.25, float(a), (C.c_float * 4)(1, 2, 3, 4))
            at = 16 + 40 * ((a - 1) % history)
            raw[at : at + 40] = bytes(r)
        return bytes(raw)

    s = _decode_guard(block(2, 1, 0, 4, [1, 2]), 4)
    assert (s["attempts"], s["skipped"], s["consecutive_skipped"]) == (2, 1, 0) and [r["attempt"] for r in s["history"]] == [1, 2]
    assert s["last"] == {"attempt": 2, "step": 1, "applied": False, "norm": 1.5, "clip": 0.25, "loss": 2.0, "group_norm": [1.0, 2.0, 3.0, 4.0]}
    s = _decode_guard(block(6, 2, 0, 4, [1, 2, 3, 4, 5, 6]), 4)
    assert [r["attempt"] for r in s["history"]] == [3, 4, 5, 6] and s["last"]["attempt"] == 6
    s = _decode_guard(block(0, 0, 0, 4, []), 4)
    assert s["history"] == [] and s["last"] is None
    s = _decode_guard(block(3, 3, 3, 0, []), 0)
    assert s["history"] == [] and s["last"] is None and s["consecutive_skipped"] == 3


# --------------------------------------------------------------------------------------------------- host-side rejections
def _segs(segs):
    from tubedetr_amd import _hip

    arr = (_hip.OptimSegment * len(segs))()
    for s, (b, e, g, a) in zip(arr, segs):
        s.begin, s.end, s.group, s.active = b, e, g, a
    return arr


OK_SEGS = [(0, 4, 0, 1), (4, 10, 1, 1)]
P = C.c_void_p(4096)  # never dereferenced: every call below is rejected on the host, before a launch


def _norm(L, **kw):
    a = dict(grad=P, n=10, segs=OK_SEGS, max_norm=0.1, ws=P, ws_bytes=L.td_grad_norm_guard_ws_bytes(), norm_clip=P, step=P, loss=None, guard=P, history=8)
    a.update(kw)
    arr = _segs(a["segs"])
    return L.td_grad_norm_clip_guarded(a["grad"], a["n"], arr, len(arr), a["max_norm"], a["ws"], a["ws_bytes"], a["norm_clip"], a["step"], a["loss"],
                                       a["guard"], a["history"], None)


def _adam(L, **kw):
    a = dict(param=P, grad=P, exp_avg=P, exp_avg_sq=P, ema=P, n=10, segs=OK_SEGS, guard=P)
    a.update(kw)
    arr = _segs(a["segs"])
    return L.td_adamw_ema_step_guarded(a["param"], a["grad"], a["exp_avg"], a["exp_avg_sq"], a["ema"], a["n"], arr, len(arr), P, P, P, 0.9, 0.999, 1e-8,
                                       1e-4, 0.9998, a["guard"], None)


NORM_REJECTIONS = {
    "null guard": (dict(guard=None), b"guard"),
    "history -1": (dict(history=-1), b"history"),
    "history 4097": (dict(history=4097), b"history"),
    "workspace one byte short": (dict(ws_bytes=-1), b"workspace"),
    "unguarded workspace size": (dict(ws_bytes=-2), b"workspace"),
    "misaligned gradient": (dict(grad=C.c_void_p(4100)), b"aligned"),
    "misaligned workspace": (dict(ws=C.c_void_p(4100)), b"aligned"),
    "misaligned guard": (dict(guard=C.c_void_p(4098)), b"aligned"),
    "null gradient": (dict(grad=None), b"null"),
    "n = 0": (dict(n=0), b"empty"),
    "segments with a gap": (dict(segs=[(0, 4, 0, 1), (5, 10, 1, 1)]), b"segments"),
    "segments short of n": (dict(segs=[(0, 4, 0, 1), (4, 9, 1, 1)]), b"segments"),
    "group 4": (dict(segs=[(0, 4, 0, 1), (4, 10, 4, 1)]), b"group"),
    "33 segments": (dict(n=33, segs=[(i, i + 1, 0, 1) for i in range(33)]), b"segments"),
}
ADAM_REJECTIONS = {
    "null guard": (dict(guard=None), b"guard"),
    "misaligned guard": (dict(guard=C.c_void_p(4098)), b"guard"),
    "misaligned param": (dict(param=C.c_void_p(4100)), b"aligned"),
    "misaligned ema": (dict(ema=C.c_void_p(4100)), b"aligned"),
    "null exp_avg": (dict(exp_avg=None), b"null"),
    "segments overlap": (dict(segs=[(0, 6, 0, 1), (5, 10, 1, 1)]), b"segments"),
    "group -1": (dict(segs=[(0, 4, -1, 1), (4, 10, 1, 1)]), b"group"),
}


@pytest.mark.parametrize("what", list(NORM_REJECTIONS))
def test_norm_guarded_rejects_on_the_host(what):
    from tubedetr_amd import _hip

    L = _hip.lib()
    kw, word = NORM_REJECTIONS[what]
    kw = dict(kw)
    if kw.get("ws_bytes") == -1:
        kw["ws_bytes"] = L.td_grad_norm_guard_ws_bytes() - 1
    elif kw.get("ws_bytes") == -2:
        kw["ws_bytes"] = L.td_grad_norm_ws_bytes()
    assert _norm(L, **kw) == -1
    msg = L.td_last_error()
    assert b"td_grad_norm_clip_guarded" in msg and word in msg, msg


@pytest.mark.parametrize("what", list(ADAM_REJECTIONS))
def test_adam_guarded_rejects_on_the_host(what):
    from tubedetr_amd import _hip

    L = _hip.lib()
    kw, word = ADAM_REJECTIONS[what]
    assert _adam(L, **kw) == -1
    msg = L.td_last_error()
    assert b"td_adamw_ema_step_guarded" in msg and word in msg, msg
