"""Reference, mutants and cases for the guarded optimizer tail (td_grad_norm_clip_guarded + td_adamw_ema_step_guarded,
tubedetr_amd/csrc/optim.hip), shared by tests/test_optim_guard_cpu.py (which proves the cases can fail) and
tests/test_optim_guard_gpu.py (which runs the kernels).  Everything here is numpy on the host.

``run`` restates the rules documented in include/tubedetr_hip.h: a sequence of (gradient, loss) attempts goes in; the final
buffers, the counters, the step counter and the ring of records come out.  The arithmetic of an applied step is
tests/optim_ref.py's float64 ``adamw_ema_ref64``; the decision is isfinite() of the norm ROUNDED TO FLOAT32.
``MUTANTS`` are plausible mistakes in the guard; every one changes the outcome of at least one entry of ``CASES``."""
import numpy as np

import optim_ref as R

GROUPS = 4          # TD_OPTIM_MAX_GROUPS
RECORD_BYTES = 40   # sizeof(td_step_record): 3 int + 3 float + GROUPS float
HEADER_BYTES = 16   # int attempts, skipped, consecutive_skipped, applied_now
HISTORY_MAX = 4096  # TD_GUARD_HISTORY_MAX

MUTANTS = {
    "step_incremented_on_skip": "the step counter advances on a skipped step too",
    "ema_moves_on_skip": "a skipped step still moves the EMA towards the parameters",
    "moments_updated_on_skip": "a skipped step still decays both moments (an update with the gradient zeroed)",
    "inactive_nonfinite_counts": "stale NaN / Inf in an inactive segment decides",
    "consecutive_not_reset": "consecutive_skipped is not reset by an applied step",
    "ring_index_off_by_one": "the record goes to attempts % history instead of (attempts - 1) % history",
    "loss_decides": "a non-finite recorded loss skips the step",
}


def norms64(g, segs, count_inactive=False):
    """-> (total L2 norm over the active elements, [norm of each group's active elements, 0 for a group with none]), float64;
    squares of float32 values are exact in float64 and never overflow it."""
    group, active = R.seg_arrays(len(g), segs)
    use = np.ones_like(active) if count_inactive else active
    sq = g.astype(np.float64) ** 2
    with np.errstate(invalid="ignore"):
        total = float(np.sqrt(sq[use].sum()))
        per_group = [float(np.sqrt(sq[use & (group == q)].sum())) for q in range(GROUPS)]
    return total, per_group


def to_f32(x):
    """A float64 value converted to float32 as the kernel's (float) cast converts it (overflow -> Inf, silently)."""
    with np.errstate(over="ignore"):
        return np.float32(x)


def run(segs, state, attempts, lrs, hp, step0=0, history=8, mut=None):
    """state: (p, m, v, ema) float32 arrays (ema may be None); attempts: [(g float32, loss float or None), ...].
    -> {"param", "exp_avg", "exp_avg_sq", "ema": float64 arrays, "step", "attempts", "skipped", "consecutive_skipped",
        "applied_now", "norm", "clip", "ring": history entries, each None (never written) or a record dict}.
    A record's "norm" and "group_norm" are the exact float64 values; "clip" is the float64 coefficient from the float64 norm."""
    assert mut is None or mut in MUTANTS
    p, m, v, ema = (None if x is None else x.astype(np.float64) for x in state)
    n = len(p)
    _, active = R.seg_arrays(n, segs)
    out = {"step": step0, "attempts": 0, "skipped": 0, "consecutive_skipped": 0, "applied_now": 0, "norm": None, "clip": None,
           "ring": [None] * history}
    decay = float(R.f32(hp.decay))
    for g, loss in attempts:
        norm, group_norm = norms64(g, segs, count_inactive=(mut == "inactive_nonfinite_counts"))
        ok = bool(np.isfinite(to_f32(norm)))
        if mut == "loss_decides" and loss is not None and not np.isfinite(loss):
            ok = False
        out["attempts"] += 1
        if ok:
            mx = float(R.f32(hp.max_norm))
            clip = min(1.0, mx / (norm + float(R.f32(1e-6)))) if mx > 0 else 1.0
            out["step"] += 1
            # (the inactive slots of g may hold NaN / Inf: adamw_ema_ref64 never reads them into an output)
            new = R.adamw_ema_ref64(p, g, m, v, ema, segs, lrs, np.float32(clip), out["step"], hp)
            p, m, v, ema = new["param"], new["exp_avg"], new["exp_avg_sq"], new["ema"]
            out["applied_now"] = 1
            if mut != "consecutive_not_reset":
                out["consecutive_skipped"] = 0
        else:
            clip = 0.0
            out["applied_now"] = 0
            out["skipped"] += 1
            out["consecutive_skipped"] += 1
            if mut == "step_incremented_on_skip":
                out["step"] += 1
            if mut == "ema_moves_on_skip" and ema is not None:
                ema = ema * decay + (1.0 - decay) * p
            if mut == "moments_updated_on_skip":
                m = np.where(active, m * float(R.f32(hp.b1)), m)
                v = np.where(active, v * float(R.f32(hp.b2)), v)
        out["norm"], out["clip"] = norm, clip
        if history > 0:
            at = out["attempts"] % history if mut == "ring_index_off_by_one" else (out["attempts"] - 1) % history
            out["ring"][at] = {"attempt": out["attempts"], "step": out["step"], "applied": out["applied_now"], "norm": norm, "clip": clip,
                               "loss": float("nan") if loss is None else float(np.float32(loss)), "group_norm": group_norm}
    out.update(param=p, exp_avg=m, exp_avg_sq=v, ema=ema)
    return out


def _same_float(a, b):
    return bool(np.array_equal(np.asarray(a, np.float64), np.asarray(b, np.float64), equal_nan=True))


def same_outcome(a, b):
    """Two results of ``run`` agree: buffers, counters, step counter and every ring entry (NaN equals NaN)."""
    for k in ("step", "attempts", "skipped", "consecutive_skipped", "applied_now"):
        if a[k] != b[k]:
            return False
    for k in ("param", "exp_avg", "exp_avg_sq", "ema"):
        if (a[k] is None) != (b[k] is None) or (a[k] is not None and not _same_float(a[k], b[k])):
            return False
    if len(a["ring"]) != len(b["ring"]):
        return False
    for x, y in zip(a["ring"], b["ring"]):
        if (x is None) != (y is None):
            return False
        if x is not None and not (all(x[k] == y[k] for k in ("attempt", "step", "applied")) and
                                  all(_same_float(x[k], y[k]) for k in ("norm", "clip", "loss", "group_norm"))):
            return False
    return True


# --------------------------------------------------------------------------------------------------------------- cases
BAD_VALUES = {"nan": np.float32(np.nan), "+inf": np.float32(np.inf), "-inf": np.float32(-np.inf)}


def first_active(layout):
    n, segs = R.LAYOUTS[layout]
    return int(np.nonzero(R.seg_arrays(n, segs)[1])[0][0])


def norm_grid(n):
    """Workgroups of the gradient-norm kernels for n elements (optim.hip: opt_grid)."""
    return max(1, min(2048, (n // 4 + 255) // 256))


def big_positions():
    """(the last element of ``big``, an active element of ``big`` that a workgroup other than 0 sums)."""
    n, segs = R.LAYOUTS["big"]
    _, active = R.seg_arrays(n, segs)
    other = 4 * (256 * 5 + 17) + 2  # float4 number 256*5 + 17 belongs to workgroup 5 in the first sweep
    assert active[n - 1] and active[other] and ((other // 4) // 256) % norm_grid(n) == 5
    return n - 1, other


# where case 2 plants its one bad element: (layout, index).  Index 5 of straddle lies in the float4 [4, 8) that holds three
# groups, 1029 in its scalar tail; index 0 is active in every layout used here.
BAD_POSITIONS_SMALL = [("straddle", 0), ("n5", 0), ("straddle", 5), ("straddle", 1029)]


def bad_gradient(layout, index, value, step=3):
    g = R.make_state(layout, step)[1].copy()
    _, active = R.seg_arrays(*R.LAYOUTS[layout])
    assert active[index], (layout, index)
    g[index] = value
    return g


def overflow_gradient(layout="straddle", step=3):
    """Every active element finite, the float32 norm not: two active elements of 3e38 (sqrt(2) * 3e38 > FLT_MAX = 3.4e38)."""
    g = R.make_state(layout, step)[1].copy()
    idx = np.nonzero(R.seg_arrays(*R.LAYOUTS[layout])[1])[0]
    g[idx[0]] = g[idx[-1]] = np.float32(3e38)
    return g


def sequence_attempts(layout="straddle"):
    """applied, skipped (NaN), skipped (-Inf), applied.  The losses: a finite one, a NaN that was handed over, none at all, and
    +Inf handed over with a FINITE gradient - a per-rank loss that must not decide."""
    fin1, fin2 = R.make_state(layout, 3, seed=21)[1], R.make_state(layout, 3, seed=22)[1]
    at = first_active(layout)
    return [(fin1, 2.5), (bad_gradient(layout, at, BAD_VALUES["nan"]), float("nan")), (bad_gradient(layout, 5, BAD_VALUES["-inf"]), None),
            (fin2, float("inf"))]


def wrap_attempts(layout="n5"):
    """Six attempts for a ring of four: applied, skipped, applied, applied, skipped, applied."""
    fin = [R.make_state(layout, 3, seed=30 + i)[1] for i in range(6)]
    bad = bad_gradient(layout, first_active(layout), BAD_VALUES["+inf"])
    return [(fin[0], 0.5), (bad, 1.5), (fin[2], 2.5), (fin[3], None), (bad, 4.5), (fin[5], 5.5)]


def cpu_cases():
    """name -> keyword arguments of ``run``: the small-layout instances of every case of tests/test_optim_guard_gpu.py."""
    hp = R.RESOLVING
    cases = {}

    def add(name, layout, attempts, step, history):
        n, segs = R.LAYOUTS[layout]
        p, _, m, v, ema = R.make_state(layout, step)
        cases[name] = dict(segs=segs, state=(p, m, v, ema), attempts=attempts, lrs=hp.lrs, hp=hp, step0=step - 1, history=history)

    for layout in R.SMALL_LAYOUTS:
        for step in R.STEPS:
            add(f"finite {layout} step {step}", layout, [(R.make_state(layout, step)[1], None)], step, 4)
    for layout, index in BAD_POSITIONS_SMALL:
        for what, value in BAD_VALUES.items():
            add(f"bad {what} at {layout}[{index}]", layout, [(bad_gradient(layout, index, value), None)], 3, 4)
    add("fp32 norm overflow", "straddle", [(overflow_gradient(), None)], 3, 4)
    add("sequence", "straddle", sequence_attempts(), 1, 8)
    add("ring wrap", "n5", wrap_attempts(), 1, 4)
    add("history 0", "n5", wrap_attempts(), 1, 0)
    return cases


# ------------------------------------------------------------------------------------------ comparing a device record
def ulp32(x):
    return float(np.spacing(np.float32(abs(x))))


def record_mismatch(got, want):
    """got: a record read from the device (floats are float32 values); want: ``run``'s record.  -> None, or what differs.
    norm: 1e-6 relative, the bound tests/test_optim_kernels_gpu.py holds td_grad_norm_clip to; clip: 4 rounding units, as
    there; group norms: ONE float32 ulp of the float64 value (the kernel's double sums err by far less, but the value may
    straddle a rounding boundary); attempt / step / applied / loss: exact (NaN equals NaN)."""
    for k in ("attempt", "step", "applied"):
        if int(got[k]) != int(want[k]):
            return (k, got[k], want[k])
    if not _same_float(np.float32(got["loss"]), np.float32(want["loss"])):
        return ("loss", got["loss"], want["loss"])
    if not np.isfinite(to_f32(want["norm"])):
        if not _same_float(np.float32(got["norm"]), to_f32(want["norm"])) or got["clip"] != 0:
            return ("norm / clip of a skipped step", got["norm"], got["clip"], want["norm"])
    else:
        if not abs(got["norm"] - want["norm"]) <= 1e-6 * want["norm"]:
            return ("norm", got["norm"], want["norm"])
        if not abs(got["clip"] - want["clip"]) <= 4 * R.U * want["clip"]:
            return ("clip", got["clip"], want["clip"])
    for q in range(GROUPS):
        w = want["group_norm"][q]
        if np.isfinite(to_f32(w)):
            if not abs(float(got["group_norm"][q]) - w) <= ulp32(w):
                return ("group_norm", q, got["group_norm"][q], w)
        elif not _same_float(np.float32(got["group_norm"][q]), to_f32(w)):
            return ("group_norm", q, got["group_norm"][q], w)
    return None
