#!/usr/bin/env python3
"""Jump-diffusion scenario sets and fused Greeks on the device, measured in one session by the library's own launch timer
(olmc_profile_enable / olmc_kernel_time: device events around each launch):

1. oljs_greeks_fd (ONE launch of jump_scenarios_kernel, 14 contracts, two jump groups) against the sum of the 14 literal launches of the
   same contracts by the one-contract kernels -- olmc_jump_diffusion (jump_kernel) plain, oljd_price European with antithetic
   (jump_path_kernel) -- at 2^14 and 2^17 paths x 252 steps, Merton and Kou, plain and antithetic.  Every rep takes the fused launch and
   then the 14 literal ones, so the two share the device's state; `literal_over_fused` is the ratio of the medians.
2. a 16-scenario, 16-group Kou set (jump_scenarios_kernel at the bound of 16) against its 16 literal launches, the same way.
3. the prices of 1. by both routes: the fused launch must give the literal prices to rounding.
4. (--sections groups) 16 Kou scenarios spread over g = 1, 2, 3, 4, 5, 8, 16 jump groups, the fused launch alone: what a group costs, and
   what the instantiated group bounds (2, 4, 16: the smallest that holds g) buy -- g = 4 runs at the bound of 4, g = 5 at the bound of 16.

    python tools/jump_scenarios_timing.py [--reps 7] [--out FILE.jsonl] [--sections greeks,sixteen,agreement | groups]

One JSON line per measurement; times are the median (ms) and the extremes (ms_min, ms_max)."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from optionslab_amd import _hip  # noqa: E402
from tests import jump_scenario_cases as jc  # noqa: E402
from tools.heston_surface_timing import summary  # noqa: E402

S, K, T, R, Q, SIGMA = jc.S, jc.K, jc.T, jc.R, jc.Q, jc.SIGMA
STEPS = 252
PATHS = (1 << 14, 1 << 17)
KOU = (True, 1.0, 0.4, 10.0, 5.0)          # the everyday Kou law: a jump a year (jc.KOU, 60 a year, is the stress case: measured too)


def one_launch_ms(call):
    _hip.profile_reset()
    call()
    n, t = _hip.kernel_time()
    assert n == 1, n
    return t


def literal(sc, N, n, seed, anti):
    if anti:
        return _hip.jd_price(*sc[:7], sc[7:], _hip.JD_EUROPEAN, 0.0, N, n, seed, True)
    return _hip.jump_diffusion(*sc[:7], *sc[7:], N, n, seed)


def fused_against_literal(fused, scenarios, N, n, seed, anti, reps):
    """(summary of the fused launch, summary of the SUM of the literal launches), rep by rep in turn after one warm-up of each."""
    fused()
    for sc in scenarios:
        literal(sc, N, n, seed, anti)
    one, many = [], []
    for _ in range(reps):
        one.append(one_launch_ms(fused))
        many.append(sum(one_launch_ms(lambda sc=sc: literal(sc, N, n, seed, anti)) for sc in scenarios))
    return summary(one), summary(many)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    ap.add_argument("--sections", default="greeks,sixteen,agreement")
    a = ap.parse_args()
    sections = a.sections.split(",")
    out = open(a.out, "w") if a.out else sys.stdout

    def emit(row):
        out.write(json.dumps(row) + "\n")
        out.flush()

    seed, n = 1, STEPS
    _hip.profile_enable(True)
    for name, model in (("merton", jc.MERTON), ("kou", KOU), ("kou-60", jc.KOU)) if "greeks" in sections else ():
        scenarios = jc.greeks_set(model)
        for N in PATHS:
            for anti in (False, True):
                fused = lambda: _hip.jd_greeks_fd(S, K, T, R, SIGMA, Q, True, model, N, n, seed, anti, True, want_evals=False)      # noqa: E731
                one, many = fused_against_literal(fused, scenarios, N, n, seed, anti, a.reps)
                emit(dict(kernel_time="greeks_fd", model=name, antithetic=anti, paths=N, steps=n, contracts=len(scenarios), groups=2,
                          fused=one, literal_sum=many, literal_over_fused=many["ms"] / one["ms"]))
    # 2. sixteen scenarios, sixteen groups (Kou, lambda from 0.5 to 8 a year)
    sixteen = [jc.scenario(95.0 + i, 90.0 + i, T, R, 0.15 + 0.01 * i, Q, i % 2 == 0, (True, 0.5 * (i + 1), 0.4, 10.0, 5.0)) for i in range(16)]
    assert _hip.jd_scenario_layout(sixteen)[0] == 16
    for N in PATHS if "sixteen" in sections else ():
        for anti in (False, True):
            fused = lambda: _hip.jd_scenarios(sixteen, N, n, seed, anti)      # noqa: E731
            one, many = fused_against_literal(fused, sixteen, N, n, seed, anti, a.reps)
            emit(dict(kernel_time="scenarios", model="kou", antithetic=anti, paths=N, steps=n, contracts=16, groups=16,
                      fused=one, literal_sum=many, literal_over_fused=many["ms"] / one["ms"]))
    # 4. what a group costs: the same 16 contracts over g laws (scenario i takes law i % g), every g in turn within a repetition
    if "groups" in sections:
        ladder = {g: [(*sc[:7], *sixteen[i % g][7:]) for i, sc in enumerate(sixteen)] for g in (1, 2, 3, 4, 5, 8, 16)}
        assert all(_hip.jd_scenario_layout(sc)[0] == g for g, sc in ladder.items())
        for N in PATHS:
            for anti in (False, True):
                calls = {g: (lambda sc=sc: _hip.jd_scenarios(sc, N, n, seed, anti)) for g, sc in ladder.items()}
                for call in calls.values():
                    call()
                ms = {g: [] for g in calls}
                for _ in range(a.reps):
                    for g, call in calls.items():
                        ms[g].append(one_launch_ms(call))
                for g in calls:
                    emit(dict(kernel_time="scenarios_by_groups", model="kou", antithetic=anti, paths=N, steps=n, contracts=16, groups=g,
                              bound=2 if g <= 2 else 4 if g <= 4 else 16, fused=summary(ms[g])))
    _hip.profile_enable(False)
    # 3. the same numbers by both routes
    for name, model in (("merton", jc.MERTON), ("kou", KOU)) if "agreement" in sections else ():
        N = PATHS[0]
        _vals, evals = _hip.jd_greeks_fd(S, K, T, R, SIGMA, Q, True, model, N, n, seed, True, True)
        worst = max(abs(st.price / literal(sc, N, n, seed, True).price - 1.0) for st, sc in zip(evals, jc.greeks_set(model)))
        emit(dict(agreement="greeks_fd", model=name, paths=N, steps=n, worst_relative_price_difference=worst))
    if a.out:
        out.close()


if __name__ == "__main__":
    main()
