"""References, error bounds, mutants and cases for the optimizer-tail kernels (tubedetr_amd/csrc/optim.hip), shared by
tests/test_optim_cpu.py (which proves the cases can fail) and tests/test_optim_kernels_gpu.py (which runs the kernels).

Everything here is numpy on the host.  ``adamw_ema_ref64`` is the arithmetic documented for td_adamw_ema_step in
include/tubedetr_hip.h, in float64, from the float32 values the kernel receives; ``adamw_ema_emul32`` is the same step in
float32 in the kernel's operation order, a stand-in for "any fp32-correct implementation" that is used only to size the
bound; ``STEP_MUTANTS`` / ``NORM_MUTANTS`` are plausible kernel mistakes that the bound has to tell apart from the reference."""
from collections import namedtuple

import numpy as np

U = 2.0 ** -24  # one fp32 rounding unit (half an ulp of 1.0)

Hyper = namedtuple("Hyper", "lrs wd b1 b2 eps decay max_norm")
# the reference's defaults (main.py: lr 5e-5, lr_backbone 1e-5, text_encoder_lr 5e-5, weight_decay 1e-4, ema_decay 0.9998,
# clip_max_norm 0.1); the fourth rate belongs to group 3, which the Python side never uses
DEFAULT = Hyper((5e-5, 1e-5, 5e-5, 2e-5), 1e-4, 0.9, 0.999, 1e-8, 0.9998, 0.1)
# every term of the update is far above fp32 resolution: four distinct rates, decay 1 - lr*wd = 1 - 1e-3 .. 1 - 2e-3
RESOLVING = Hyper((1e-2, 3e-3, 2e-2, 7e-3), 0.1, 0.9, 0.999, 1e-8, 0.9, 0.5)
HYPERS = {"default": DEFAULT, "resolving": RESOLVING}
STEPS = (1, 3, 1000)  # the value of the step counter DURING the update (td_grad_norm_clip has already incremented it)


def f32(x):
    """Round to float32, widen to float64: the value a ``float`` argument of the C ABI carries."""
    return np.asarray(x, dtype=np.float32).astype(np.float64)


# ------------------------------------------------------------------------------------------------------------- layouts
def _seg32():
    lens = [2 * ((7 * k) % 23) + 139 for k in range(32)]  # 32 unequal odd lengths, 139 .. 183
    segs, at = [], 0
    for k, ln in enumerate(lens):
        segs.append((at, at + ln, k % 4, 0 if k % 5 == 2 else 1))
        at += ln
    return at, segs


BIG_N = 8192 * 256 * 4 + 1024 + 1  # past td_adamw_ema_step's 8192-workgroup cap, 4+ sweeps of the norm kernel's 2048
LAYOUTS = {
    # float4 straddles: [4,8) holds g0 active | g1 active | g2 inactive | g1 active; [256,260) active | inactive;
    # [1028,1032) is the scalar tail (1028 inactive, 1029-1030 active in another group than the last vector)
    "straddle": (1031, [(0, 5, 0, 1), (5, 6, 1, 1), (6, 7, 2, 0), (7, 258, 1, 1), (258, 1029, 3, 0), (1029, 1031, 2, 1)]),
    "n1": (1, [(0, 1, 2, 1)]),
    "n3": (3, [(0, 1, 0, 1), (1, 2, 1, 0), (2, 3, 3, 1)]),
    "n4": (4, [(0, 3, 1, 1), (3, 4, 0, 1)]),
    "n5": (5, [(0, 2, 3, 1), (2, 4, 0, 0), (4, 5, 1, 1)]),
    "seg32": _seg32(),
    "big": (BIG_N, [(0, 2097153, 1, 1), (2097153, 2097153 + 4194305, 2, 0), (2097153 + 4194305, BIG_N, 3, 1)]),
}
SMALL_LAYOUTS = [k for k in LAYOUTS if k != "big"]


def seg_arrays(n, segs):
    """-> (group[n] int, active[n] bool)."""
    group, active = np.zeros(n, np.int64), np.zeros(n, bool)
    for b, e, g, a in segs:
        group[b:e], active[b:e] = g, bool(a)
    return group, active


def straddle_elements(n, segs):
    """Indices of active elements that the kernels reach inside a float4 (vector body) holding more than one group."""
    group, active = seg_arrays(n, segs)
    nv = n // 4
    gv = group[: nv * 4].reshape(nv, 4)
    mixed = (gv != gv[:, :1]).any(axis=1)
    idx = np.nonzero(np.repeat(mixed, 4))[0]
    return idx[active[idx]]


# -------------------------------------------------------------------------------------------------------------- states
def make_state(name, step, seed=0):
    """fp32 inputs of one update at step counter ``step``: p, g, m, v, ema (numpy float32) for layout ``name``.
    |g| spans 1e-8 .. 1 (so that sqrt(v) is comparable with eps = 1e-8 on some elements and far above it on others) and is
    scaled to an L2 norm of 1 (3e-8 at step 1000) over the active elements; p cycles through exactly 0, ~1e-3 and ~1 so that both the terms
    relative to p and the ones relative to the update are resolvable somewhere; step 1 is a fresh optimizer (m = v = 0).
    Inactive gradient slots hold NaN / Inf: a parameter without a gradient leaves its slice of the flat buffer stale."""
    n, segs = LAYOUTS[name]
    rng = np.random.default_rng(1000 * seed + step + 7 * len(name))
    group, active = seg_arrays(n, segs)
    sign = lambda: rng.choice([-1.0, 1.0], n)
    g = sign() * 10.0 ** rng.uniform(-8, 0, n)
    if active.any():
        g[np.nonzero(active)[0][0]] = 1.0  # the span's top end is present however short the layout
    # steps 1 and 3: norm 1, clipped; step 1000: vanished gradients of norm 3e-8, unclipped, sqrt(v) ~ eps everywhere
    g = g / np.sqrt((g[active] ** 2).sum()) * (3e-8 if step == 1000 else 1.0)
    pat = (np.arange(n) + STEPS.index(step) if step in STEPS else np.arange(n)) % 3
    p = sign() * np.where(pat == 0, 0.0, np.where(pat == 1, 1e-3, 1.0)) * rng.uniform(0.5, 2.0, n)
    if step == 1:
        m, v = np.zeros(n), np.zeros(n)
    else:
        m = sign() * np.abs(g) * rng.uniform(0.0, 2.0, n)
        v = g * g * rng.uniform(0.25, 4.0, n)
    ema = p + 0.25 * sign()
    g = g.astype(np.float32)
    bad = np.array([np.nan, np.inf, -np.inf], np.float32)
    g[~active] = bad[np.arange(n)[~active] % 3]
    return tuple(x.astype(np.float32) for x in (p, g, m, v, ema))


# ---------------------------------------------------------------------------------------------------------- references
def norm_clip_ref64(g, segs, max_norm, count_inactive=False):
    """-> (L2 norm over the active elements, clip coefficient min(1, max_norm / (norm + 1e-6)); 1 when max_norm <= 0)."""
    _, active = seg_arrays(len(g), segs)
    use = np.ones_like(active) if count_inactive else active
    norm = float(np.sqrt((g.astype(np.float64)[use] ** 2).sum()))
    mx = float(f32(max_norm))
    clip = min(1.0, mx / (norm + float(f32(1e-6)))) if mx > 0 else 1.0
    return norm, clip


def _step64(p, g, m, v, ema, segs, lrs, clip, step, hp, mut=None):
    n = len(p)
    group, active = seg_arrays(n, segs)
    p, m, v = (x.astype(np.float64) for x in (p, m, v))
    g = np.where(active | (mut == "inactive_updated"), np.where(np.isfinite(g), g, 0.0), 0.0).astype(np.float64)
    e = None if ema is None else ema.astype(np.float64)
    b1, b2, eps, wd, decay, clip = (float(f32(x)) for x in (hp.b1, hp.b2, hp.eps, hp.wd, hp.decay, clip))
    lr = f32(lrs)[(group + 1) % 4 if mut == "neighbour_group_lr" else group]
    t = step - 1 if mut == "bias_step_minus_1" else step
    with np.errstate(divide="ignore", invalid="ignore"):
        bc1 = 1.0 - b1 ** t
        bc2s = 1.0 if mut == "no_bias2_sqrt" else np.sqrt(1.0 - b2 ** t)
        gg = g if mut == "no_clip" else g * clip
        dec = 1.0 - lr * wd
        p1 = p if mut in ("no_weight_decay", "decay_after_update") else p * dec
        m1 = m + (gg - m) * (1.0 - b1)
        v1 = v * b2 + (1.0 - b2) * gg * gg
        denom = np.sqrt(v1 + eps) / bc2s if mut == "eps_inside_sqrt" else np.sqrt(v1) / bc2s + eps
        p2 = p1 - (lr / bc1) * (m1 / denom)
        if mut == "decay_after_update":
            p2 = p2 * dec
    upd = np.ones(n, bool) if mut == "inactive_updated" else active
    out = {"param": np.where(upd, p2, p), "exp_avg": np.where(upd, m1, m), "exp_avg_sq": np.where(upd, v1, v), "ema": None}
    if e is not None:
        src = p if mut == "ema_from_old_param" else out["param"]
        out["ema"] = e * decay + (1.0 - decay) * src
        if mut == "ema_skips_inactive":
            out["ema"] = np.where(active, out["ema"], e)
    return out


def adamw_ema_ref64(p, g, m, v, ema, segs, lrs, clip, step, hp):
    """One td_adamw_ema_step in float64 from fp32 inputs -> {"param", "exp_avg", "exp_avg_sq", "ema"} (float64 arrays).
    Inactive elements keep param and both moments; their EMA follows update_ema: ema*decay + (1-decay)*param."""
    return _step64(p, g, m, v, ema, segs, lrs, clip, step, hp)


def adamw_ema_emul32(p, g, m, v, ema, segs, lrs, clip, step, hp):
    """The same step in numpy float32, one rounding per operation in adam_elem's order (no fused multiply-adds)."""
    F = np.float32
    n = len(p)
    group, active = seg_arrays(n, segs)
    g = np.where(active, g, F(0)).astype(F)
    b1, b2, eps, wd, decay, clip = (F(x) for x in (hp.b1, hp.b2, hp.eps, hp.wd, hp.decay, clip))
    lr = np.asarray(lrs, F)[group]
    one = F(1)
    bc1 = -np.expm1(F(step) * np.log1p(b1 - one))  # 1 - beta^t without the cancellation of 1.f - powf(beta, t)
    bc2s = np.sqrt(-np.expm1(F(step) * np.log1p(b2 - one)))
    assert bc1.dtype == F and bc2s.dtype == F
    gg = g * clip
    p1 = p * (one - lr * wd)
    m1 = m + (gg - m) * (one - b1)
    v1 = v * b2 + (one - b2) * gg * gg
    denom = np.sqrt(v1) / bc2s + eps
    p2 = p1 - (lr / bc1) * (m1 / denom)
    out = {"param": np.where(active, p2, p), "exp_avg": np.where(active, m1, m), "exp_avg_sq": np.where(active, v1, v), "ema": None}
    if ema is not None:
        out["ema"] = ema * decay + (one - decay) * out["param"]
    assert all(x is None or x.dtype == F for x in out.values())
    return out


# --------------------------------------------------------------------------------------------------------------- bound
# c = 4 x the worst err/unit of adamw_ema_emul32 against adamw_ema_ref64 over every layout, hyper-parameter set and step
# of this file (tests/test_optim_cpu.py recomputes the ratio and asserts 4 x worst <= C_BOUND <= 64).
MEASURED_WORST_RATIO = 3.72  # param 3.37, exp_avg 2.02, exp_avg_sq 3.72, ema 1.75 (printed by test_emulation_within_bound)
C_BOUND = 15.0  # 4 x 3.72 = 14.9


def units(p, g, m, v, ema, segs, lrs, clip, step, hp):
    """Per element and output, the sum of the magnitudes of the operands that are added or subtracted to form it (float64).
    Inactive elements: 0 for param / exp_avg / exp_avg_sq (they must not change at all)."""
    group, active = seg_arrays(len(p), segs)
    ref = adamw_ema_ref64(p, g, m, v, ema, segs, lrs, clip, step, hp)
    p, m, v = (np.abs(x.astype(np.float64)) for x in (p, m, v))
    gg = np.abs(np.where(active, g, 0.0).astype(np.float64)) * float(f32(clip))
    b1, b2, eps, decay = (float(f32(x)) for x in (hp.b1, hp.b2, hp.eps, hp.decay))
    lr = f32(lrs)[group]
    bc1, bc2s = 1.0 - b1 ** step, np.sqrt(1.0 - b2 ** step)
    denom = np.sqrt(ref["exp_avg_sq"]) / bc2s + eps
    u = {"param": np.where(active, p + (lr / bc1) * (m + gg) / denom, 0.0),  # NOT |p| + |dp|: m + (g-m)(1-b1) cancels
         "exp_avg": np.where(active, m + (1.0 - b1) * (gg + m), 0.0),
         "exp_avg_sq": np.where(active, b2 * v + (1.0 - b2) * gg * gg, 0.0), "ema": None}
    if ema is not None:
        u["ema"] = decay * np.abs(ema.astype(np.float64)) + (1.0 - decay) * np.where(active, u["param"], p)
    return u


def bound(p, g, m, v, ema, segs, lrs, clip, step, hp, c=C_BOUND):
    """Per-element error bound of each output: c * 2^-24 * units (0 where the output must be bit-identical to its input)."""
    return {k: (None if x is None else c * U * x) for k, x in units(p, g, m, v, ema, segs, lrs, clip, step, hp).items()}


def worst_ratio(got, ref, unit):
    """max over the elements of |got - ref| / (2^-24 * unit); an error where the unit is 0 counts as inf."""
    err = np.abs(got.astype(np.float64) - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err == 0, 0.0, err / (U * unit))
    return float(np.nanmax(np.where(np.isnan(r), np.inf, r))) if len(r) else 0.0


# ------------------------------------------------------------------------------------------------------------- mutants
# name -> (which elements it concerns: "active" / "inactive", what it stands for)
STEP_MUTANTS = {
    "bias_step_minus_1": ("active", "bias corrections computed with step-1"),
    "no_clip": ("active", "clip coefficient not applied to the gradient"),
    "no_weight_decay": ("active", "param *= 1 - lr*wd left out"),
    "decay_after_update": ("active", "weight decay applied after the Adam update"),
    "eps_inside_sqrt": ("active", "sqrt(v + eps) instead of sqrt(v) + eps"),
    "no_bias2_sqrt": ("active", "no sqrt(1 - beta2^t) correction of the denominator"),
    "neighbour_group_lr": ("active", "learning rate of group (k+1) % 4"),
    "ema_from_old_param": ("active", "EMA fed with the parameter before the update"),
    "ema_skips_inactive": ("inactive", "EMA not updated where there is no gradient"),
    "inactive_updated": ("inactive", "an element without a gradient decayed / updated"),
}
NORM_MUTANTS = {"inactive_in_norm": "an inactive element's (stale) gradient counted in the norm"}


def mutant_step(name, *args):
    assert name in STEP_MUTANTS
    return _step64(*args, mut=name)


# At the reference's defaults float32(1) - float32(lr)*float32(wd) == 1.0f for all three rates (lr*wd <= 5e-9 < 2^-25), in
# the kernel exactly as in torch's AdamW: a step without weight decay, or with the decay applied after the update, is
# the same fp32 computation, and against float64 it differs by lr*wd*|p| <= 0.1 rounding units of |p|.
NOT_SEPARABLE_AT_DEFAULTS = {
    "no_weight_decay": "1 - lr*wd == 1.0f: the decay is below fp32 resolution",
    "decay_after_update": "1 - lr*wd == 1.0f: the decay is below fp32 resolution, wherever it is applied",
}
# Separable in some segment kinds only, for a different reason: the EMA moves by (1-decay) * dp = 2e-4 * lr * O(1) <= 1e-8,
# under 10 x bound of an EMA that is >= 0.25 away from 0 unless dp is large against the EMA's magnitude.
PARTLY_SEPARABLE_AT_DEFAULTS = {"ema_from_old_param": "(1 - ema_decay) * lr * O(1) <= 1e-8 against |ema| >= 0.25"}
