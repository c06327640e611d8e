"""The cases of tests/optim_ref.py are well posed (no GPU): a float32 implementation of the documented step stays within
``bound`` at every layout, hyper-parameter set and step, while every mutant - a plausible kernel mistake - leaves it by more
than a factor of 10 somewhere in every kind of segment it concerns.  That is the proof that
tests/test_optim_kernels_gpu.py, which compares the kernels with the same reference under the same bound, can fail."""
import numpy as np
import pytest

import optim_ref as R


def _args(layout, hp_name, step):
    n, segs = R.LAYOUTS[layout]
    hp = R.HYPERS[hp_name]
    p, g, m, v, ema = R.make_state(layout, step)
    _, clip = R.norm_clip_ref64(g, segs, hp.max_norm)
    return (p, g, m, v, ema, segs, hp.lrs, np.float32(clip), step, hp)


def test_layouts_are_what_the_kernels_need():
    n, segs = R.LAYOUTS["straddle"]
    assert n % 4 == 3 and {4, 5, 7, 256, 257}.issubset(set(R.straddle_elements(n, segs).tolist()))
    assert [R.LAYOUTS[k][0] for k in ("n1", "n3", "n4", "n5")] == [1, 3, 4, 5]
    n32, s32 = R.LAYOUTS["seg32"]
    assert len(s32) == 32 and 4900 < n32 < 5300 and len({e - b for b, e, _, _ in s32}) > 8 and all((e - b) % 2 for b, e, _, _ in s32)
    assert {g for _, _, g, a in s32 if a} == {0, 1, 2, 3} and any(not a for *_, a in s32)
    nb, sb = R.LAYOUTS["big"]
    assert nb // 4 > 8192 * 256 and nb // 4 > 4 * 2048 * 256 and nb % 4 == 1 and all(b % 4 for b, _, _, _ in sb[1:])
    for n, segs in R.LAYOUTS.values():
        assert segs[0][0] == 0 and segs[-1][1] == n and all(a[1] == b[0] for a, b in zip(segs, segs[1:]))


def test_states_span_eps():
    """sqrt(v) comparable with eps on some elements, far above it on others; inactive gradients are NaN / Inf."""
    p, g, m, v, ema = R.make_state("straddle", 3)
    _, act = R.seg_arrays(*R.LAYOUTS["straddle"])
    s = np.sqrt(v[act].astype(np.float64))
    assert (s < 1e-7).any() and (s > 1e-3).any() and not np.isfinite(g[~act]).any() and np.isfinite(g[act]).all()
    assert (p == 0).any() and (np.abs(p) > 0.5).any() and np.abs(ema - p).min() > 0.2
    p, g, m, v, ema = R.make_state("n1", 1)
    assert not m.any() and not v.any()


def test_emulation_within_bound():
    worst = {k: 0.0 for k in ("param", "exp_avg", "exp_avg_sq", "ema")}
    for layout in R.SMALL_LAYOUTS:
        for hp_name in R.HYPERS:
            for step in R.STEPS:
                a = _args(layout, hp_name, step)
                ref, emu, unit = R.adamw_ema_ref64(*a), R.adamw_ema_emul32(*a), R.units(*a)
                _, act = R.seg_arrays(*R.LAYOUTS[layout])
                for k in worst:
                    worst[k] = max(worst[k], R.worst_ratio(emu[k], ref[k], unit[k]))
                    assert (np.abs(emu[k].astype(np.float64) - ref[k]) <= R.bound(*a)[k]).all(), (layout, hp_name, step, k)
                for k, x in zip(("param", "exp_avg", "exp_avg_sq"), (a[0], a[2], a[3])):
                    assert np.array_equal(emu[k][~act], x[~act]) and np.array_equal(ref[k][~act], x[~act].astype(np.float64))
    print("worst err/unit of the float32 emulation:", {k: round(x, 2) for k, x in worst.items()})
    top = max(worst.values())
    assert abs(top - R.MEASURED_WORST_RATIO) < 0.05, "update MEASURED_WORST_RATIO in optim_ref.py"
    assert 4 * top <= R.C_BOUND <= 4 * R.MEASURED_WORST_RATIO + 0.2 and R.C_BOUND <= 64


def _separated(layout, hp_name, name):
    """-> {kind: True/False}: is there, in some state of the set, an element of that kind where the mutant is > 10 x bound
    away from the reference on some output.  Kinds: ("active", group), "inactive", and "straddle" for the group-rate mutant."""
    n, segs = R.LAYOUTS[layout]
    group, active = R.seg_arrays(n, segs)
    concerns = R.STEP_MUTANTS[name][0]
    kinds = {}
    if concerns == "active":
        for gr in sorted({g for _, _, g, a in segs if a}):
            kinds[("active", gr)] = active & (group == gr)
        if name == "neighbour_group_lr" and len(R.straddle_elements(n, segs)):
            sel = np.zeros(n, bool)
            sel[R.straddle_elements(n, segs)] = True
            kinds["straddle"] = sel
    elif (~active).any():
        kinds["inactive"] = ~active
    seen = {k: False for k in kinds}
    for step in R.STEPS:
        a = _args(layout, hp_name, step)
        ref, mut, bnd = R.adamw_ema_ref64(*a), R.mutant_step(name, *a), R.bound(*a)
        far = np.zeros(n, bool)
        for k in ref:
            far |= ~(np.abs(mut[k] - ref[k]) <= 10 * bnd[k])  # (a NaN / Inf mutant output is far)
        for k, sel in kinds.items():
            seen[k] = seen[k] or bool((far & sel).any())
    return seen


@pytest.mark.parametrize("name", list(R.STEP_MUTANTS))
def test_mutant_is_separated_at_resolving_hyper_parameters(name):
    for layout in R.SMALL_LAYOUTS:
        seen = _separated(layout, "resolving", name)
        assert all(seen.values()), (name, layout, seen)
    if name == "neighbour_group_lr":
        assert _separated("straddle", "resolving", name)["straddle"]


def test_norm_mutant_is_separated():
    """A stale finite gradient in an inactive slot, counted in the norm, moves it by far more than the GPU test's 1e-6."""
    for layout in R.SMALL_LAYOUTS:
        n, segs = R.LAYOUTS[layout]
        _, act = R.seg_arrays(n, segs)
        if act.all():
            continue
        g = R.make_state(layout, 3)[1]
        g[~act] = 0.5
        norm, clip = R.norm_clip_ref64(g, segs, R.RESOLVING.max_norm)
        bad_norm, bad_clip = R.norm_clip_ref64(g, segs, R.RESOLVING.max_norm, count_inactive=True)
        assert abs(bad_norm - norm) > 1e-5 * norm and abs(bad_clip - clip) > 1e-5 * clip and clip < 1
    assert list(R.NORM_MUTANTS) == ["inactive_in_norm"]


def test_mutants_not_separable_at_defaults_are_listed():
    F = np.float32
    for lr in R.DEFAULT.lrs[:3]:
        assert F(1) - F(lr) * F(R.DEFAULT.wd) == F(1)  # the reason: the decay factor rounds to 1.0f
    for lr in R.RESOLVING.lrs:
        assert F(1) - F(lr) * F(R.RESOLVING.wd) < F(1) - F(1e-4)
    hidden = set()
    for name in R.STEP_MUTANTS:
        ok = all(all(_separated(layout, "default", name).values()) for layout in ("straddle", "seg32"))
        if not ok:
            hidden.add(name)
    assert hidden == set(R.NOT_SEPARABLE_AT_DEFAULTS) | set(R.PARTLY_SEPARABLE_AT_DEFAULTS), hidden
    for name in R.NOT_SEPARABLE_AT_DEFAULTS:  # ... and not merely in one kind: nowhere, in no state
        for layout in R.SMALL_LAYOUTS:
            assert not any(_separated(layout, "default", name).values()), (name, layout)


def test_norm_clip_ref():
    n, segs = R.LAYOUTS["n5"]
    g = np.array([3, 4, np.nan, np.inf, 12], np.float32)
    norm, clip = R.norm_clip_ref64(g, segs, 6.5)
    assert norm == 13.0 and abs(clip - 6.5 / (13 + float(np.float32(1e-6)))) < 1e-15
    assert R.norm_clip_ref64(g, segs, 0.0)[1] == 1.0 and R.norm_clip_ref64(g, segs, -1.0)[1] == 1.0 and R.norm_clip_ref64(g, segs, 14.0)[1] == 1.0
