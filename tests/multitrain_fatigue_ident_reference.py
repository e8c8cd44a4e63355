"""Reference side of the multi-train fatigue-parameter identification tests (cfx_idfm_* /
FesMultiTrainFatigueIdentification) — TEST INFRASTRUCTURE ONLY (CPU, torch float64 and numpy).

``TrainFatigueSetup`` is the exact-autodiff rollout of a fatigue model on ONE train as the kernel is given it (a
``pack_train`` dict: pulse times, activation nodes, truncation, N, final_time, per-pulse values).  The stimulation
rows and the interval controls are rebuilt from the activation nodes with the sweep's window semantics
(``tests.sweep_reference.window_rows`` / ``interval_controls``: pulses with act_node <= k, the last ``truncation`` of
them); the rollout itself is ``FatigueSetup.trajectory``: ``oracle.fes_autodiff.rhs`` and ``_step`` unchanged from
the fatigue rest state, differentiated with ``jacfwd``.  ``forces``, ``forces_and_sens``, ``normal`` are
``tests/ident_reference.py``'s on this rollout, the joint normal equations ``multitrain_ident_reference.joint_normal``
and the comparator of the fits ``lm_reference``, all unchanged.

``python -m tests.multitrain_fatigue_ident_reference`` prints the rollout's own noise (jacfwd against jacrev) on the
test shapes.
"""

from __future__ import annotations

import functools

import numpy as np

from oracle import fes_autodiff as AD
from oracle import fes_oracle as O
from tests import multitrain_ident_reference as M
from tests import sweep_reference as SR
from tests.fatigue_ident_reference import FATIGUE_KEYS, FatigueSetup, lm_reference, scaled_errors  # noqa: F401
from tests.multitrain_ident_reference import joint_normal  # noqa: F401  (re-exported for the tests)

SCHEMES = ("RK1", "RK2", "RK4")
MODELS = ("ding2003_with_fatigue", "ding2007_with_fatigue", "hmed2018_with_fatigue")
SUBSET = ["tau_fat", "alpha_tau1"]

# E = 3: N = 10, 13, 8 (the NaN fill of the two shorter ones), final_time 1 / 1.3 / 0.4, truncation 3 / larger than
# the pulse count (20 > 8) / 1, a doublet train whose second pulses fall between two nodes, a first pulse after t = 0
# (an empty window at first; one width / intensity for that train: IvpFes has no per-pulse width before the first
# pulse), per-pulse widths / intensities elsewhere (seeded).
MIXED = (
    M._case([0.0, 0.1, 0.2, 0.3, 0.4, 0.5, 0.6], "single", 3, 10, 1.0, 201),
    M._case([0.0, 0.3, 0.6, 0.9], "doublet", 20, 13, 1.3, 202),
    M._case([0.1, 0.2, 0.3], "single", 1, 8, 0.4, 203, varying=False),
)


class TrainFatigueSetup(FatigueSetup):
    """One train of a fatigue model, from its ``pack_train`` dict."""

    def __init__(self, name, train, scheme, m):  # noqa: super().__init__ builds the oracle's own table: not wanted
        if not name.endswith("with_fatigue"):
            raise ValueError(f"{name} has no fatigue states")
        self.name, self.scheme, self.m = name, scheme, m
        self.N, self.T = train["n_shooting"], train["truncation"]
        self.final_time, self.dt = train["final_time"], train["final_time"] / train["n_shooting"]
        self.c = O.model_constants(name)
        self.rows = AD._t(SR.window_rows(train))
        u = SR.interval_controls(name, train)  # (nu, N)
        self.controls = None if u.size == 0 else AD._t(np.ascontiguousarray(u.T))


def packed_train(name, case):
    return M.packed_train(name, case)


def setup_of(name, case, scheme, m):
    return TrainFatigueSetup(name, packed_train(name, case), scheme, m)


def pack(name, cases, targets=None, weights=None):
    """cfx_idm_trains arrays of the cases, in the order given (``multitrain_ident_reference.pack``)."""
    return M.pack(name, cases, targets, weights)


def theta_of(name, keys, B, seed):
    """(n_id, B) within +-20 % of the model defaults."""
    return M.theta_of(name, keys, B, seed)


@functools.lru_cache(maxsize=None)
def reference(name, scheme, m, subset, B=70):
    """(keys, theta, [forces (N_e + 1, B)], [sens (N_e + 1, n_id, B)]) of ``MIXED`` by exact autodiff, once per case."""
    keys = SUBSET if subset else FATIGUE_KEYS
    theta = theta_of(name, keys, B, seed=61 + int(subset))
    theta.setflags(write=False)
    Fs, Ss = [], []
    for case in MIXED:
        F, S = setup_of(name, case, scheme, m).forces_and_sens(keys, theta)
        F.setflags(write=False)
        S.setflags(write=False)
        Fs.append(F)
        Ss.append(S)
    return keys, theta, tuple(Fs), tuple(Ss)


def reference_noise(name, scheme, m, B=8):
    """The rollout's own noise on the test shapes: jacfwd against jacrev, as the scaled error of the sensitivities
    (largest over the trains and the columns)."""
    theta = theta_of(name, FATIGUE_KEYS, B, seed=61)
    worst = 0.0
    for case in MIXED:
        st = setup_of(name, case, scheme, m)
        F, Sf = st.forces_and_sens(FATIGUE_KEYS, theta)
        _, Sr = st.forces_and_sens(FATIGUE_KEYS, theta, mode="rev")
        worst = max(worst, float(scaled_errors(F, Sf, F, Sr)[1].max()))
    return worst


# ---- the end-to-end recovery protocol ----------------------------------------------------------------------------
# Three recordings: 25 Hz for FIT_BURST seconds, a rest gap, 25 Hz for FIT_TEST seconds.  Every pulse is on the 0.04 s
# grid, so the LCM rule gives dt = 0.04 s; RK4 x 2 makes h = 0.02 s (for the calcium row, the fastest of the five,
# h / tauc is 1.0 with Ding2003 and Hmed2018 and 1.82 with Ding2007: inside RK4's stability interval 2.78).  One width
# (4e-4 s) / intensity (60 mA) per recording.
FIT_PERIOD, FIT_BURST, FIT_TEST, FIT_GAPS = 0.04, 5.0, 1.0, (10.0, 30.0, 60.0)
FIT_SCHEME, FIT_M, FIT_TRUNCATION = "RK4", 2, 20


def fit_cases():
    out = []
    for e, gap in enumerate(FIT_GAPS):
        n0, n1 = round(FIT_BURST / FIT_PERIOD), round((FIT_BURST + gap) / FIT_PERIOD)
        n2 = round((FIT_BURST + gap + FIT_TEST) / FIT_PERIOD)
        stim = [round(i * FIT_PERIOD, 2) for i in list(range(n0)) + list(range(n1, n2))]
        out.append(M._case(stim, "single", FIT_TRUNCATION, None, FIT_BURST + gap + FIT_TEST, 300 + e, varying=False))
    return out


def fit_bounds(name):
    """(true, lower, upper) of the four keys: FesFatigueIdentification's defaults."""
    c = O.model_constants(name)
    true = np.array([c[k] for k in FATIGUE_KEYS], dtype=float)
    return true, np.minimum(0.01 * true, 100.0 * true), np.maximum(0.01 * true, 100.0 * true)


def reference_fit(name, starts=None, max_iter=100):
    """The CPU comparator of the end-to-end fit: ``lm_reference`` on the exact-AD joint normal equations of the three
    recordings, targets generated at the model defaults by the same rollouts, the product's 64 starts
    (``multitrain_ident_reference.fit_starts``) or the ones of ``starts``.  About 5,900 RK4 steps per evaluation
    (see ``reference_fit_parallel``, which is what the command line runs):
    ``python -m tests.multitrain_fatigue_ident_reference fit NAME`` prints the figures DESIGN section 7e and the GPU
    test record."""
    setups = [setup_of(name, case, FIT_SCHEME, FIT_M) for case in fit_cases()]
    true, lower, upper = fit_bounds(name)
    targets = [st.forces(FATIGUE_KEYS, true[:, None])[:, 0] for st in setups]
    weights = [np.ones(st.N + 1) for st in setups]
    th0 = M.fit_starts(true, lower, upper)
    if starts is not None:
        th0 = th0[:, list(starts)]
    rep = lambda a: np.repeat(a[:, None], th0.shape[1], 1)  # noqa: E731
    theta, cost, iters, status, hist = lm_reference(joint_normal(setups, FATIGUE_KEYS, targets, weights), th0,
                                                    rep(lower), rep(upper), max_iter=max_iter)
    return {"theta": theta, "cost": cost, "iterations": iters, "status": status, "history": hist, "true": true,
            "n_shooting": [st.N for st in setups]}


_WORKER = {}


def _worker_init(name, e):
    import torch

    torch.set_num_threads(1)
    st = setup_of(name, fit_cases()[e], FIT_SCHEME, FIT_M)
    true = fit_bounds(name)[0]
    y = st.forces(FATIGUE_KEYS, true[:, None])[:, 0]
    _WORKER["fn"], _WORKER["N"] = st.normal(FATIGUE_KEYS, y, np.ones(st.N + 1)), st.N


def _worker_normal(theta):
    if theta is None:
        return _WORKER["N"]
    return tuple(t.numpy() for t in _WORKER["fn"](AD._t(theta)))


def reference_fit_parallel(name, starts=None, max_iter=100):
    """``reference_fit`` with one process per recording (the recordings are independent; a rollout costs about 28 ms
    per RK4 step whatever the number of starts): the same sums in the same order, so the same figures."""
    import multiprocessing as mp

    ctx = mp.get_context("spawn")
    pools = [ctx.Pool(1, initializer=_worker_init, initargs=(name, e)) for e in range(len(FIT_GAPS))]

    def normal(theta):
        jobs = [p.apply_async(_worker_normal, (theta.numpy(),)) for p in pools]
        parts = [[AD._t(a) for a in j.get()] for j in jobs]
        c, g, H = parts[0]
        for c2, g2, H2 in parts[1:]:
            c, g, H = c + c2, g + g2, H + H2
        return c, g, H

    true, lower, upper = fit_bounds(name)
    th0 = M.fit_starts(true, lower, upper)
    if starts is not None:
        th0 = th0[:, list(starts)]
    rep = lambda a: np.repeat(a[:, None], th0.shape[1], 1)  # noqa: E731
    try:
        n_shooting = [p.apply(_worker_normal, (None,)) for p in pools]
        theta, cost, iters, status, hist = lm_reference(normal, th0, rep(lower), rep(upper), max_iter=max_iter)
    finally:
        for p in pools:
            p.terminate()
    return {"theta": theta, "cost": cost, "iterations": iters, "status": status, "history": hist, "true": true,
            "n_shooting": n_shooting}


def report(name, out):
    rel = np.abs(out["theta"] / out["true"][:, None] - 1)
    print(name, "n_shooting", out["n_shooting"], "status counts", np.bincount(out["status"], minlength=4),
          "iterations max", int(out["iterations"].max()))
    print("cost: final max %.3e, initial min %.3e, monotone %s" % (
        out["cost"].max(), out["history"][0].min(), bool(np.all(np.diff(out["history"], axis=0) <= 0))))
    print("largest relative errors:", {k: float("%.3g" % rel[j].max()) for j, k in enumerate(FATIGUE_KEYS)})


if __name__ == "__main__":
    import sys

    if len(sys.argv) > 2 and sys.argv[1] == "fit":
        n_ = int(sys.argv[3]) if len(sys.argv) > 3 else 64
        report(sys.argv[2], reference_fit_parallel(sys.argv[2], starts=range(n_)))
        sys.exit(0)
    for name_ in MODELS:
        for scheme_ in SCHEMES:
            for m_ in (1, 5):
                print(f"{name_} {scheme_} x {m_}: jacfwd against jacrev {reference_noise(name_, scheme_, m_):.2e}")
