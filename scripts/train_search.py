"""Search the stimulation train that follows a target force: every candidate scored on the device in one launch.

Grid: Ding2003 with fatigue, frequencies fmin..fmax Hz x single / doublet / triplet trains (x the given truncations),
each with its own n_shooting by the stimulation-time LCM rule.  Target: a plateau (a ramp to ``--plateau`` N over the
first 0.2 s, held to the end).  ``TrainSearch`` packs the grid without building an ``IvpFes`` per candidate and
``IvpSweep.score`` (``cfx_sweep_score``) returns the final states and six metrics per candidate.  Prints the ranked
head of the table, the best candidate under a bound on the final Km, and the wall-clock times of packing, of the
``score`` launch and of the old route on the same grid: ``integrate(nodes=True)`` plus the numpy reduction around
its NaN padding.

    python scripts/train_search.py [--fmin 10] [--fmax 60] [--final-time 1] [--truncations 10] [--head 10]
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


def reduce_nodes(nodes, final_time, y, sample_dt):
    """track, impulse and peak from the node forces (B, N_max + 1), NaN past an instance's own n_shooting."""
    F, n = nodes["F"], nodes["n_shooting"]
    k = np.arange(F.shape[1])
    dt = final_time / n
    inside = k[None, :] <= n[:, None]
    target = np.interp(k[None, :] * dt[:, None], np.arange(len(y)) * sample_dt, y)
    Fz = np.where(inside, F, 0.0)
    err = np.where(inside, F - target, 0.0)
    last = F[np.arange(len(n)), n]
    return {"track": dt * np.sum(err * err, axis=1), "impulse": dt * (Fz.sum(axis=1) - 0.5 * F[:, 0] - 0.5 * last),
            "peak": np.nanmax(F, axis=1)}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--fmin", type=int, default=10)
    ap.add_argument("--fmax", type=int, default=60)
    ap.add_argument("--final-time", type=float, default=1.0)
    ap.add_argument("--truncations", type=int, nargs="+", default=[10])
    ap.add_argument("--plateau", type=float, default=150.0)
    ap.add_argument("--head", type=int, default=10)
    ap.add_argument("--device", type=int, default=0)
    args = ap.parse_args()

    from cocofest_amd import DingModelFrequencyWithFatigue, OdeSolver, TrainSearch, load_library

    load_library()  # libcfx (and torch's HIP runtime) once, outside the timed packing
    tf = args.final_time
    sample_dt = 0.1
    y = np.minimum(np.arange(int(round(tf / sample_dt)) + 1) * sample_dt / 0.2, 1.0) * args.plateau
    model = DingModelFrequencyWithFatigue(stim_time=[0.0], sum_stim_truncation=args.truncations[0])
    t0 = time.perf_counter()
    with contextlib.redirect_stdout(io.StringIO()):  # the n_shooting warning of the LCM rule, once per candidate
        search = TrainSearch(model, final_time=tf, frequencies=range(args.fmin, args.fmax + 1), pulse_modes=MODES,
                             truncations=args.truncations, ode_solver=OdeSolver.RK4(n_integration_steps=10),
                             device=args.device)
    t_pack = time.perf_counter() - t0
    sweep = search.sweep
    sweep.sweep()  # library object and device context, outside the timed launches
    search.run(y, sample_dt)  # first launch: code object load
    t0 = time.perf_counter()
    result = search.run(y, sample_dt)
    t_score = time.perf_counter() - t0
    sweep.integrate(nodes=True)
    t0 = time.perf_counter()
    nodes = sweep.integrate(nodes=True)
    t_nodes = time.perf_counter() - t0
    t0 = time.perf_counter()
    old = reduce_nodes(nodes, tf, y, sample_dt)
    t_reduce = time.perf_counter() - t0
    node_bytes = (sweep.max_shooting + 1) * model.nb_state * sweep.batch * 8

    print(f"{sweep.batch} candidates, up to {sweep.max_pulses} pulses, n_shooting up to {sweep.max_shooting}")
    print(f"{'rank':>4} {'Hz':>4} {'mode':>8} {'T':>3} {'track':>12} {'impulse':>10} {'peak':>9} {'end_error':>10} "
          f"{'Km':>8}")
    for rank, i in enumerate(result.ranking("track")[: args.head]):
        r = result.row(i)
        print(f"{rank:4d} {r['frequency']:4d} {r['pulse_mode']:>8} {r['sum_stim_truncation']:3d} {r['track']:12.4f} "
              f"{r['impulse']:10.4f} {r['peak']:9.3f} {r['end_error']:10.3f} {r['Km']:8.5f}")
    km_cap = float(np.median(result["Km"]))
    best = result.best("track", subject_to={"Km": (None, km_cap)})
    print(f"best with final Km <= {km_cap:.5f}: {best['frequency']} Hz {best['pulse_mode']}, track {best['track']:.4f}")
    worst = max(float(np.max(np.abs(old[k] - result[k]) / np.maximum(np.abs(result[k]), 1e-300))) for k in old)
    print(f"packing {t_pack:.3f} s; score launch {t_score * 1e3:.3f} ms; "
          f"nodes route {(t_nodes + t_reduce) * 1e3:.3f} ms "
          f"(integrate(nodes=True) {t_nodes * 1e3:.3f} ms for {node_bytes / 1e6:.1f} MB of nodes + numpy reduction "
          f"{t_reduce * 1e3:.3f} ms); largest relative difference of track / impulse / peak between the routes: "
          f"{worst:.2e}")
    print(json.dumps({"candidates": sweep.batch, "max_pulses": sweep.max_pulses, "max_shooting": sweep.max_shooting,
                      "pack_s": t_pack, "score_launch_s": t_score, "nodes_integrate_s": t_nodes,
                      "nodes_reduce_s": t_reduce, "node_bytes": node_bytes, "routes_max_rel_diff": worst}))
    search.close()


if __name__ == "__main__":
    main()
