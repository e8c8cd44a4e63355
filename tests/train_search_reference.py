"""Reference side of the train-search tests (cfx_sweep_score / IvpSweep.score / TrainSearch).

The target rule and the six metrics of include/cfx.h restated in python floats: the target's fma is evaluated exactly
on Fractions and rounded once, the sums go through ``math.fsum``.  ``metrics_of`` reduces any row of node forces
(the numpy rollout of tests/sweep_reference.py, the oracle's, or ``IvpSweep.integrate(nodes=True)``'s) the same way.
"""

import math
from fractions import Fraction

import numpy as np

from tests import sweep_reference as R

METRICS = ("track", "impulse", "peak", "peak_node", "end_error", "mean_force")

# The target of the parity tests: 8 samples every 0.1 s, a ramp to a plateau and a release.  The table ends at
# 0.7 s: shorter than final_time = 1 (the last sample is held), longer than 0.3 and 0.5; with final_time = 1 and
# N = 10 or 20 node times fall on samples.
TARGET_Y = (0.0, 40.0, 90.0, 150.0, 150.0, 150.0, 120.0, 100.0)
TARGET_DT = 0.1


def target_at(y, sample_dt, t):
    """y(t) by the rule of cfx_sweep_score: u = t * (1 / sample_dt), j = floor(u); one sample, or j past the last
    interval: the last sample; otherwise fma(u - j, y[j+1] - y[j], y[j])."""
    n = len(y)
    if n == 1:
        return float(y[0])
    u = t * (1.0 / sample_dt)
    j = math.floor(u)
    if j >= n - 1:
        return float(y[n - 1])
    a, b, c = u - j, float(y[j + 1]) - float(y[j]), float(y[j])
    return float(Fraction(a) * Fraction(b) + Fraction(c))  # fma: one rounding


def node_targets(y, sample_dt, n_shooting, final_time):
    dt = final_time / n_shooting
    return np.array([target_at(y, sample_dt, k * dt) for k in range(n_shooting + 1)])


def metrics_of(force, final_time, y, sample_dt):
    """The six metrics of the node forces F_0..F_N of one instance, and the node targets."""
    F = [float(f) for f in force]
    N = len(F) - 1
    dt = final_time / N
    yk = node_targets(y, sample_dt, N, final_time)
    track = dt * math.fsum((f - t) ** 2 for f, t in zip(F, yk))
    impulse = dt * math.fsum([0.5 * F[0]] + F[1:N] + [0.5 * F[N]])
    peak = max(F)
    return {"track": track, "impulse": impulse, "peak": peak, "peak_node": F.index(peak),
            "end_error": F[N] - float(yk[N]), "mean_force": impulse / final_time}, yk


def metric_scales(force, final_time, yk):
    """The scale of every metric's error: track by dt sum (|F_k| + |y_k|)^2, impulse by dt sum |F_k| (mean_force: that
    over final_time), peak and end_error by max(|F|, |y|) over the nodes.  A scale of zero (no force at all) leaves
    the error absolute."""
    F = np.abs(np.asarray(force, dtype=np.float64))
    dt = final_time / (len(F) - 1)
    top = max(float(F.max()), float(np.abs(yk).max()))
    scales = {"track": dt * float(np.sum((F + np.abs(yk)) ** 2)), "impulse": dt * float(F.sum()), "peak": top,
              "end_error": top, "mean_force": dt * float(F.sum()) / final_time}
    return {k: (v if v > 0.0 else 1.0) for k, v in scales.items()}


def scaled_metric_error(got, ref, scales):
    """Largest scaled error over the five real-valued metrics (peak_node is compared exactly by the caller)."""
    return max(abs(float(got[k]) - ref[k]) / scales[k] for k in scales)


def top_two_gap(force):
    """Relative gap between the two largest node forces (inf for a single node)."""
    F = np.sort(np.asarray(force, dtype=np.float64))
    if len(F) < 2:
        return math.inf
    return float(F[-1] - F[-2]) / max(abs(float(F[-1])), abs(float(F[-2])), np.finfo(float).tiny)


# ---- the batch of the GPU tests: the mixed batch plus three edge instances -----------------------------------------
def _edge(stim, N, tf, seed):
    return {"stim_time": stim, "pulse_mode": "single", "truncation": 3, "n_shooting": N, "final_time": tf,
            "varying": False, "seed": seed}


# a pulse after final_time is never visible: an instance with zero pulses.  N = 4: track is five fma steps and one
# product, at most 6 roundings of 2^-53 relative on a sum of non-negative terms, below the 1e-15 it is held to.
ZERO_PULSE = _edge([2.0], 4, 1.0, 11)
ONE_INTERVAL = _edge([0.0], 1, 0.01, 12)
# starts at F = 2000 N, far above any tetanic force of the models, and decays at dt = 25 ms for ten intervals before
# the first pulse: no later node comes near the start force
PEAK_AT_START = _edge([0.25, 0.3, 0.35], 20, 0.5, 13)
START_FORCE = 2000.0


def score_cases():
    """The 70 mixed trains and the three edge instances (indices 70, 71, 72)."""
    return tuple(R.mixed_cases()) + (ZERO_PULSE, ONE_INTERVAL, PEAK_AT_START)


def score_x0(name):
    """(73, nx) start states: the rest state, except the last instance's force."""
    from oracle import fes_oracle as O

    x0 = np.tile(np.asarray(O.rest_values(name, O.model_constants(name)), dtype=np.float64), (73, 1))
    x0[72, 1] = START_FORCE
    return x0


def train_dict(name, case):
    """The case as a train dict of ``IvpSweep.from_trains``."""
    train = {"stim_time": list(case["stim_time"]), "final_time": case["final_time"],
             "n_shooting": case["n_shooting"], "pulse_mode": case["pulse_mode"],
             "sum_stim_truncation": case["truncation"]}
    train.update(R.case_values(name, case))
    return train
