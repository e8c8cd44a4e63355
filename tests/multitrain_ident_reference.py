"""Reference side of the multi-train identification tests (cfx_idm_* / FesMultiTrainIdentification) — TEST
INFRASTRUCTURE ONLY (CPU, torch float64 and numpy).

One ``tests.ident_reference.Setup`` per train (imported, not edited): forces and sensitivities by exact autodiff; the
joint normal equations are the sum, in the order given, of every Setup's ``normal``.  ``idm_rollout`` restates in
numpy the rollout the kernel performs from what it is given (pulse times, activation nodes, truncation, N,
final_time, per-pulse values): the window is cut from the activation nodes, the forcing is the factorised
cs = E (G0 + (r0 - 1) G1) with its tangents, the force row's partials are written out.
"""

import functools

import numpy as np

from tests import ident_reference as R
from tests import sweep_reference as SR

SCHEMES = ("RK1", "RK2", "RK4")
SUBSET = {"ding2003": ["tau2", "a_rest"], "ding2007": ["pdt", "km_rest"], "hmed2018": ["Is", "km_rest"]}
SLOTS = {"ding2003": ["a_rest", "km_rest", "tau1_rest", "tau2"],
         "ding2007": ["a_scale", "km_rest", "tau1_rest", "tau2", "pd0", "pdt"],
         "hmed2018": ["a_rest", "km_rest", "tau1_rest", "tau2", "ar", "bs", "Is", "cr"]}


def _case(stim, mode, T, N, tf, seed, varying=True):
    return {"stim_time": [float(t) for t in stim], "pulse_mode": mode, "truncation": T, "n_shooting": N,
            "final_time": tf, "varying": varying, "seed": seed}


# E = 4: N in {5, 10, 20}, final_time in {0.5, 1, 2}, 3..12 pulses, truncation 1 / 3 / 5 / larger than the pulse
# count, a doublet train, a duplicated pulse time, a first pulse after t = 0 (one width / intensity for that train:
# IvpFes has no per-pulse width before the first pulse), per-pulse widths / intensities elsewhere (seeded, so they
# differ within and between trains).
MIXED = (
    _case([0.0, 0.1, 0.1, 0.2, 0.3, 0.4, 0.5], "single", 3, 10, 1.0, 101),
    _case([0.0, 0.4, 0.8, 1.2, 1.6], "doublet", 20, 20, 2.0, 102),
    _case([0.1, 0.2, 0.3], "single", 1, 5, 0.5, 103, varying=False),
    _case([round(0.05 * i, 2) for i in range(12)], "single", 5, 20, 1.0, 104),
)
# a train no cfx_create handle could carry (truncation > 32), next to a short one
LONG = (
    _case([round(0.025 * i, 3) for i in range(40)], "single", 40, 40, 1.0, 105),
    _case([0.0, 0.1, 0.2, 0.3], "single", 2, 10, 1.0, 106),
)


def setup_of(name, case, scheme, m):
    v = SR.case_values(name, case)
    return R.Setup(name, SR.expanded_times(case), case["final_time"], case["n_shooting"], case["truncation"], scheme,
                   m, pulse_width=v.get("pulse_width"), pulse_intensity=v.get("pulse_intensity"))


def packed_train(name, case):
    """What ``cocofest_amd.ivp.pack_train`` gives for the case (the kernel's input of one train)."""
    from cocofest_amd.ivp import pack_train

    return pack_train(SR.make_ivp(name, case))


def pack(name, cases, targets=None, weights=None):
    """cfx_idm_trains arrays of the cases, in the order given (train-minor SoA)."""
    trains = [packed_train(name, c) for c in cases]
    E, P, nn = len(trains), max(len(t["times"]) for t in trains), max(t["n_shooting"] for t in trains) + 1
    out = {"times": np.zeros((P, E)), "act_node": np.zeros((P, E), dtype=np.int32),
           "value": None if trains[0]["value"] is None else np.zeros((P, E)),
           "n_pulses": np.array([len(t["times"]) for t in trains], dtype=np.int32),
           "truncation": np.array([t["truncation"] for t in trains], dtype=np.int32),
           "n_shooting": np.array([t["n_shooting"] for t in trains], dtype=np.int32),
           "final_time": np.array([t["final_time"] for t in trains])}
    if targets is not None:
        out["target"], out["weight"] = np.full((nn, E), np.nan), np.full((nn, E), np.nan)  # past N: never read
    for e, t in enumerate(trains):
        n = len(t["times"])
        out["times"][:n, e], out["act_node"][:n, e] = t["times"], t["act_node"]
        if out["value"] is not None:
            out["value"][:n, e] = t["value"]
        if targets is not None:
            out["target"][: t["n_shooting"] + 1, e] = targets[e]
            out["weight"][: t["n_shooting"] + 1, e] = weights[e]
    return out, P, nn - 1


def theta_of(name, keys, B, seed):
    """(n_id, B) within +-20 % of the model defaults."""
    from oracle import fes_oracle as O

    c = O.model_constants(name)
    d = np.array([c[k] for k in keys], dtype=float)
    return d[:, None] * (1 + 0.2 * np.random.default_rng(seed).uniform(-1, 1, (len(keys), B)))


@functools.lru_cache(maxsize=None)
def reference(name, scheme, m, subset, which="mixed", B=70):
    """(keys, theta, [forces (N_e + 1, B)], [sens (N_e + 1, n_id, B)]) by exact autodiff, computed once per case."""
    cases = MIXED if which == "mixed" else LONG
    keys = SUBSET[name] if subset else R.FULL_KEYS[name]
    theta = theta_of(name, keys, B, seed=41 + int(subset))
    theta.setflags(write=False)
    Fs, Ss = [], []
    for case in cases:
        F, S = setup_of(name, case, scheme, m).forces_and_sens(keys, theta)
        F.setflags(write=False)
        S.setflags(write=False)
        Fs.append(F)
        Ss.append(S)
    return keys, theta, tuple(Fs), tuple(Ss)


def joint_normal(setups, keys, targets, weights):
    """theta (n, B) tensor -> cost (B,), grad (B, n), H (B, n, n) of the joint fit: the sum over the trains, in the
    order given, of every Setup's exact-AD normal equations (each with its own dt)."""
    fns = [st.normal(keys, y, w) for st, y, w in zip(setups, targets, weights)]

    def fn(theta):
        c, g, H = fns[0](theta)
        for f in fns[1:]:
            c2, g2, H2 = f(theta)
            c, g, H = c + c2, g + g2, H + H2
        return c, g, H

    return fn


# ---- the kernel's formulation, restated ----------------------------------------------------------------------------
def idm_rollout(name, c, train, keys, theta, scheme, m):
    """Forces (N + 1, B) and sensitivities (N + 1, n_id, B) by the formulation of cfx_idm.h, in numpy float64.
    ``train``: a ``pack_train`` dict; theta (n_id, B)."""
    slots = SLOTS[name]
    B = theta.shape[1]
    th = {k: np.full(B, float(c[k])) for k in slots}
    for j, k in enumerate(keys):
        th[k] = theta[j].astype(float)
    D = len(slots)
    ix = {k: i for i, k in enumerate(slots)}
    A_key = slots[0]
    tauc, mult = c["tauc"], 1.0
    N, T, tf = train["n_shooting"], train["truncation"], train["final_time"]
    times, act, value = train["times"], train["act_node"], train["value"]
    dt = tf / N
    h = dt / m
    eh2 = np.exp(-(h / 2) / tauc)
    r0m1 = th["km_rest"] + c["r0_km_relationship"] - 1.0
    hmed, d07 = name == "hmed2018", name == "ding2007"
    cn, F = np.zeros(B), np.zeros(B)
    cnd, Fd = np.zeros((D, B)), np.zeros((D, B))
    out_F, out_S = [F.copy()], [Fd.copy()]
    nv = 0
    for k in range(N):
        while nv < len(times) and act[nv] <= k:
            nv += 1
        lo = max(0, nv - T)
        tk = k * dt
        g0, g1 = np.zeros(B), np.zeros(B)
        a0, a1 = np.zeros((4, B)), np.zeros((4, B))
        for i in range(lo, nv):
            w0 = np.exp(-(tk - times[i]) / tauc)
            w1 = 0.0 if i == lo else np.exp(-(times[i] - times[i - 1]) / tauc) * w0
            if hmed:
                di = value[i] - th["Is"]
                tnh = np.tanh(th["bs"] * di)
                sech2 = 1.0 - tnh * tnh
                lam = th["ar"] * (tnh + th["cr"])
                dl = np.stack([tnh + th["cr"], th["ar"] * sech2 * di, -th["ar"] * th["bs"] * sech2, th["ar"]])
                g0, g1 = g0 + lam * w0, g1 + lam * w1
                a0, a1 = a0 + dl * w0, a1 + dl * w1
            else:
                g0, g1 = g0 + w0, g1 + w1
        G = g0 + r0m1 * g1
        Gd = np.zeros((D, B))
        Gd[ix["km_rest"]] = g1
        if hmed:
            Gd[4:8] = a0 + r0m1 * a1
        amp, dE4, dE5 = np.ones(B), np.zeros(B), np.zeros(B)
        if d07 and times:
            pw = value[max(nv - 1, 0)]
            z = (pw - th["pd0"]) / th["pdt"]
            ex = np.exp(-z)
            amp, dE4, dE5 = 1.0 - ex, -ex / th["pdt"], -ex * z / th["pdt"]

        def rhs(es, cn, F, cnd, Fd):
            km, tau1, tau2, A0 = th["km_rest"], th["tau1_rest"], th["tau2"], th[A_key]
            kcn = (es * G - cn) / tauc
            kcnd = (es * Gd - cnd) / tauc
            A = A0 * amp
            d1 = km + cn
            d2 = tau1 * d1 + tau2 * cn
            s1, t2 = cn / d1, d1 / d2
            kF = mult * (A * s1 - F * t2)
            W0 = A / d1**2 + F * tau2 / d2**2
            g_cn, g_F = mult * km * W0, -mult * t2
            kFd = g_F * Fd + g_cn * cnd
            kFd[0] += mult * s1 * amp
            kFd[1] += -cn * mult * W0
            kFd[2] += mult * F * t2 * t2
            kFd[3] += mult * F * t2 * cn / d2
            if d07:
                kFd[4] += mult * s1 * A0 * dE4
                kFd[5] += mult * s1 * A0 * dE5
            return kcn, kF, kcnd, kFd

        ea = 1.0
        for j in range(m):
            eb = np.exp(-((j + 1) * h) / tauc)
            x = (cn, F, cnd, Fd)
            k1 = rhs(ea, *x)
            step = lambda kk, a: tuple(xi + a * ki for xi, ki in zip(x, kk))  # noqa: E731
            if scheme == "RK1":
                x = step(k1, h)
            elif scheme == "RK2":
                x = step(rhs(ea * eh2, *step(k1, h / 2)), h)
            else:
                k2 = rhs(ea * eh2, *step(k1, h / 2))
                k3 = rhs(ea * eh2, *step(k2, h / 2))
                k4 = rhs(eb, *step(k3, h))
                x = tuple(xi + h / 6 * (p + 2 * q + 2 * r + s) for xi, p, q, r, s in zip(x, k1, k2, k3, k4))
            cn, F, cnd, Fd = x
            ea = eb
        out_F.append(F.copy())
        out_S.append(Fd.copy())
    S = np.stack(out_S)  # (N + 1, D, B)
    return np.stack(out_F), S[:, [ix[k] for k in keys], :]


# ---- the end-to-end fits ---------------------------------------------------------------------------------------------
TRAIN_THEN_REST = [round(0.05 * i, 2) for i in range(10)]  # ten pulses at 20 Hz, then 0.5 s of rest; N = 20
FIT_SCHEME, FIT_M, FIT_STARTS, FIT_SPREAD, FIT_SEED = "RK4", 5, 64, 0.2, 0


def fit_problem(which):
    """(model name, keys, per-train control values) of the two end-to-end fits: Ding2007 under three constant pulse
    widths, Hmed2018 under three intensity ramps spanning 30..100 mA (different per train and per pulse)."""
    if which == "ding2007":
        return "ding2007", R.FULL_KEYS["ding2007"], [2e-4, 3.5e-4, 6e-4]
    ramps = ((30.0, 66.0), (45.0, 100.0), (95.0, 50.0))
    return "hmed2018", R.FULL_KEYS["hmed2018"], [[lo + (hi - lo) * i / 9 for i in range(10)] for lo, hi in ramps]


def fit_starts(true, lower, upper):
    """FesMultiTrainIdentification.starts() for the guess true x 1.15 / x 0.87 alternating, restated."""
    guess = np.clip(true * np.array([1.15 if j % 2 == 0 else 0.87 for j in range(len(true))]), lower, upper)
    z = np.random.default_rng(FIT_SEED).uniform(-1.0, 1.0, size=(len(true), FIT_STARTS))
    z[:, 0] = 0.0
    return np.clip(guess[:, None] * np.exp(FIT_SPREAD * z), lower[:, None], upper[:, None])


def reference_fit(which, max_iter=100, starts=None):
    """The CPU comparator of an end-to-end fit: ``lm_reference`` on the exact-AD joint normal equations, targets
    generated at the model defaults by the same Setups.  ``starts``: the indices of the starts to run (default all 64;
    the starts are independent, so chunks can run in separate processes).  Run by hand to calibrate the GPU tests
    (``python -m tests.multitrain_ident_reference ding2007|hmed2018 [max_iter]`` prints the recorded figures), not by
    any test: 12 to 40 s per LM iteration on 8 CPU cores, so 2 minutes for Ding2007 (9 iterations) and a quarter of
    an hour for Hmed2018 at the 25 iterations its test uses."""
    from cocofest_amd.identification import DEFAULT_VALUES

    name, keys, values = fit_problem(which)
    kw = "pulse_width" if name == "ding2007" else "pulse_intensity"
    setups = [R.Setup(name, TRAIN_THEN_REST, 1.0, 20, 10, FIT_SCHEME, FIT_M, **{kw: v}) for v in values]
    true = setups[0].defaults(keys)
    targets = [st.forces(keys, true[:, None])[:, 0] for st in setups]
    weights = [np.ones(21) for _ in setups]
    lower = np.array([DEFAULT_VALUES[name][k][1] for k in keys], dtype=float)
    upper = np.array([DEFAULT_VALUES[name][k][2] for k in keys], dtype=float)
    th0 = fit_starts(true, lower, upper)
    if starts is not None:
        th0 = th0[:, list(starts)]
    rep = lambda a: np.repeat(a[:, None], th0.shape[1], 1)  # noqa: E731
    theta, cost, iters, status, hist = R.lm_reference(joint_normal(setups, keys, targets, weights), th0, rep(lower),
                                                      rep(upper), max_iter=max_iter)
    return {"theta": theta, "cost": cost, "iterations": iters, "status": status, "history": hist, "true": true}


def report(which, out):
    """The figures DESIGN section 7d and tests/test_multitrain_ident_gpu.py record of a reference fit."""
    _, keys, _ = fit_problem(which)
    hist, cost, status, true = out["history"], out["cost"], out["status"], out["true"]
    ratio = cost / hist[0]
    print(which, "status counts", np.bincount(status, minlength=4), "iterations max", out["iterations"].max())
    print("cost: final max %.3e, initial min %.3e, monotone %s" % (cost.max(), hist[0].min(),
                                                                 bool(np.all(np.diff(hist, axis=0) <= 0))))
    print("starts with status 0:", np.flatnonzero(status == 0).tolist())
    slow = np.flatnonzero(~(ratio < 1e-3))
    print("starts with final / initial cost >= 1e-3:", [(int(b), float("%.3g" % ratio[b])) for b in slow])
    print("largest final / initial cost of the others: %.3e" % np.max(np.delete(ratio, slow), initial=0.0))
    rel = np.abs(out["theta"] / true[:, None] - 1)
    print("largest relative errors:", {k: float("%.3g" % rel[j].max()) for j, k in enumerate(keys)})


if __name__ == "__main__":
    import sys

    report(sys.argv[1], reference_fit(sys.argv[1], max_iter=int(sys.argv[2]) if len(sys.argv) > 2 else 100))
