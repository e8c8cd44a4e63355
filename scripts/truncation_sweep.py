"""The reference's summation-truncation study (examples/sensitivity/truncation/sensitivity_analysis.py) in one launch.

Grid: Ding2003 with fatigue, final_time 1, RK4 x 10, pulse modes single / doublet / triplet, n_stim = 1..max_stim
evenly spaced pulses, truncation = 1..n_stim: 3 max_stim (max_stim + 1) / 2 trains (15,150 at the default 100), each
with its own n_shooting by the stimulation-time LCM rule.  Every train is an ordinary ``IvpFes``; ``IvpSweep``
integrates them together.  Prints the wall time of building the IvpFes objects, of packing (IvpSweep) and of the
launch (host arrays in, final states back) separately, then, for a seeded sample of trains with truncation <= 32, the
largest difference to a per-train ``IvpFes.integrate`` and the time that loop took.

    python scripts/truncation_sweep.py [--max-stim 100] [--sample 200] [--seed 0] [--device 0]
"""

from __future__ import annotations

import argparse
import contextlib
import io
import json
import pathlib
import sys
import time

import numpy as np

sys.path.insert(0, str(pathlib.Path(__file__).resolve().parent.parent))

MODES = ("single", "doublet", "triplet")
STATES = ("Cn", "F", "A", "Tau1", "Km")


def grid(max_stim):
    return [(mode, n, T) for mode in MODES for n in range(1, max_stim + 1) for T in range(1, n + 1)]


def make_ivp(mode, n_stim, truncation):
    from cocofest_amd import DingModelFrequencyWithFatigue, IvpFes, OdeSolver

    model = DingModelFrequencyWithFatigue(stim_time=[round(i / n_stim, 3) for i in range(n_stim)],
                                          sum_stim_truncation=truncation)
    return IvpFes({"model": model, "pulse_mode": mode},
                  {"final_time": 1, "ode_solver": OdeSolver.RK4(n_integration_steps=10)})


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--max-stim", type=int, default=100)
    ap.add_argument("--sample", type=int, default=200, help="trains compared with a per-train IvpFes.integrate")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--device", type=int, default=0)
    args = ap.parse_args()

    from cocofest_amd import IvpSweep

    cases = grid(args.max_stim)
    t0 = time.perf_counter()
    with contextlib.redirect_stdout(io.StringIO()):  # the n_shooting warning of the LCM rule, once per train
        ivps = [make_ivp(*c) for c in cases]
    t_build = time.perf_counter() - t0
    t0 = time.perf_counter()
    sweep = IvpSweep(ivps, device=args.device)
    t_pack = time.perf_counter() - t0
    sweep.sweep()  # library object and device context, outside the timed launches
    sweep.integrate()  # first launch: code object load
    t0 = time.perf_counter()
    res = sweep.integrate()
    t_launch = time.perf_counter() - t0
    out = {"trains": len(cases), "max_pulses": sweep.max_pulses, "max_shooting": sweep.max_shooting,
           "build_ivpfes_s": t_build, "pack_s": t_pack, "launch_s": t_launch}
    print(f"{len(cases)} trains, up to {sweep.max_pulses} pulses, n_shooting up to {sweep.max_shooting}")
    print(f"IvpFes construction {t_build:.3f} s, packing {t_pack:.3f} s, launch {t_launch * 1e3:.3f} ms")

    eligible = [i for i, c in enumerate(cases) if c[2] <= 32]
    rng = np.random.default_rng(args.seed)
    sample = rng.choice(eligible, size=min(args.sample, len(eligible)), replace=False)
    worst, t_loop = 0.0, 0.0
    for i in sample:
        t0 = time.perf_counter()
        with contextlib.redirect_stdout(io.StringIO()):
            ivp = make_ivp(*cases[i])
        single = ivp.integrate(return_time=False)
        t_loop += time.perf_counter() - t0
        ivp.close()
        for name in STATES:
            ref = single[name][0]
            worst = max(worst, abs(res[name][i] - ref[-1]) / np.max(np.abs(ref)))
    if len(sample):
        out.update(sample=len(sample), sample_loop_s=t_loop, loop_scaled_to_grid_s=t_loop / len(sample) * len(cases),
                   max_scaled_difference=worst)
        print(f"per-train IvpFes(...).integrate() over {len(sample)} sampled trains: {t_loop:.3f} s "
              f"({t_loop / len(sample) * len(cases):.1f} s scaled to the grid); largest difference of a final state, "
              f"scaled by the state's largest magnitude: {worst:.3e}")
    print(json.dumps(out))
    sweep.close()


if __name__ == "__main__":
    main()
