"""CPU reference of the implicit collocation integrator (cfx_integrate on a collocation handle) — test helper.

Every interval's FULL d nx defect system is solved at once by Newton in float64: the residual is the defect formula
of ``oracle.fes_collocation`` (sum_i C[i][j] x^i - dt f(t_k + tau_j dt, x^j, u)) over ``oracle.fes_oracle.rhs``, the
Jacobian is exact, ``torch.func.jacfwd`` of the same rows over ``oracle.fes_autodiff.rhs``, and the linear solves are
LAPACK's.  Nothing of the kernel's reduction (constant calcium / fatigue inverses, a Newton on the force alone) is
shared: all unknowns are solved together.

    integrate(pb, X0, U, start)     trajectory (B, N (d+1) + 1, nx) in cfx_integrate's sample order and a per-instance
                                    convergence flag; start = "copy" (node state copied to every point) or "euler"
                                    (explicit-Euler predictor x^0 + tau_j dt f(t_k, x^0, u))
    reference(...)                  the cached trajectory of a named test case with eps_ref, the largest difference
                                    between the two starts scaled per state by its trajectory maximum: the reference's
                                    own noise
"""

from __future__ import annotations

import functools

import numpy as np
import torch
from torch.func import jacfwd, vmap

from oracle import fes_autodiff as A
from oracle import fes_collocation as CO
from oracle import fes_oracle as O
from tests import cases

STEP_TOL = 1e-14  # Newton stops once every scaled update is below this; the next iterate's error is its square
MAX_ITER = 40


def col_problem(name, stims, final_time, truncation, n_shooting, degree, method, intensity_params=False):
    base = cases.oracle_problem(name, stims, final_time, truncation, scheme="RK1", m=1, n_shooting=n_shooting,
                                intensity_params=intensity_params)
    return CO.ColProblem(**{f: getattr(base, f) for f in base.__dataclass_fields__}, degree=degree, method=method)


def _residual(pb, tau, C, k, x0, Z, Uk):
    """Defect rows of interval k, (B, d, nx): fes_collocation.eval_g's formula over fes_oracle.rhs."""
    B, d = x0.shape[0], pb.degree
    XC = np.concatenate([x0[:, None, :], Z], axis=1)
    rows = np.tile(pb.rows[k][:, None], (1, B))
    out = []
    for j in range(1, d + 1):
        t = k * pb.dt + tau[j] * pb.dt
        f = O.rhs(pb.name, pb.c, t, XC[:, j, :].T, Uk.T if pb.nu else None, rows)
        out.append(np.einsum("i,bir->br", C[:, j], XC) - pb.dt * f.T)
    return np.stack(out, axis=1)


def _jacobian(pb, tau, C, k, x0, Z, Uk):
    """d residual / d Z, (B, d nx, d nx): the block (j, i) is C[i][j] I - [i == j] dt df/dx(t_k + tau_j dt, x^j, u),
    with df/dx exact, forward-mode AD of fes_autodiff.rhs at every point."""
    B, d, nx = Z.shape[0], pb.degree, pb.nx
    row = A._t(pb.rows[k])
    t = A._t(np.tile(k * pb.dt + tau[1:] * pb.dt, B))
    x = A._t(Z.reshape(B * d, nx))
    if pb.nu:
        u = A._t(np.repeat(Uk, d, axis=0))
        fx = vmap(jacfwd(lambda xx, tt, uu: A.rhs(pb.name, pb.c, tt, xx, uu, row)))(x, t, u)
    else:
        fx = vmap(jacfwd(lambda xx, tt: A.rhs(pb.name, pb.c, tt, xx, None, row)))(x, t)
    fx = fx.numpy().reshape(B, d, nx, nx)
    J = np.einsum("ij,rc->jric", C[1:, 1:], np.eye(nx))[None].repeat(B, axis=0)  # (B, j, r, i, c)
    for j in range(d):
        J[:, j, :, j, :] -= pb.dt * fx[:, j]
    return J.reshape(B, d * nx, d * nx)


def integrate(pb, X0, U, start="copy"):
    """X0 (B, nx), U (B, N, nu) -> (traj (B, N (d+1) + 1, nx), converged (B,) bool)."""
    tau, C, D = CO.coefficients(pb.degree, pb.method)
    B, N, d, nx = X0.shape[0], pb.n_shooting, pb.degree, pb.nx
    x = np.array(X0, dtype=np.float64)
    samples = []
    converged = np.ones(B, dtype=bool)
    for k in range(N):
        Uk = U[:, k, :] if pb.nu else None
        if start == "copy":
            Z = np.repeat(x[:, None, :], d, axis=1)
        else:
            rows = np.tile(pb.rows[k][:, None], (1, B))
            f0 = O.rhs(pb.name, pb.c, k * pb.dt, x.T, Uk.T if pb.nu else None, rows).T
            Z = x[:, None, :] + tau[1:, None][None] * pb.dt * f0[:, None, :]
        step = np.full(B, np.inf)
        for _ in range(MAX_ITER):
            R = _residual(pb, tau, C, k, x, Z, Uk).reshape(B, -1)
            J = _jacobian(pb, tau, C, k, x, Z, Uk)
            dZ = np.linalg.solve(J, -R[:, :, None])[:, :, 0].reshape(B, d, nx)
            Z = Z + dZ
            scale = np.maximum(np.abs(Z).max(axis=1), np.abs(x)) + 1e-300
            step = (np.abs(dZ).max(axis=1) / scale).max(axis=1)
            if np.all(step <= STEP_TOL):
                break
        converged &= step <= STEP_TOL
        XC = np.concatenate([x[:, None, :], Z], axis=1)
        samples.append(XC)
        x = np.einsum("i,bir->br", D, XC)
    return np.concatenate(samples + [x[:, None, :]], axis=1), converged


def scaled_error(got, ref):
    """max |got - ref| with every state scaled by its largest |ref| over the trajectory (per instance)."""
    scale = np.abs(ref).max(axis=1, keepdims=True) + 1e-300
    return float((np.abs(got - ref) / scale).max())


# ---- the shared test inputs ---------------------------------------------------------------------------------------
B_MAX = 70  # one full wave and a partial one


def random_inputs(pb, B, seed):
    """Per-instance start states and controls around the defaults: pulse widths >= pd0, intensities above the
    minimum pulse intensity."""
    r = np.random.default_rng(seed)
    c = pb.c
    X0 = np.zeros((B, pb.nx))
    X0[:, 0] = r.uniform(0.0, 0.3, B)
    X0[:, 1] = r.uniform(0.0, 50.0, B)
    if pb.nx == 5:
        a0 = c["a_scale"] if pb.name.startswith("ding2007") else c["a_rest"]
        X0[:, 2] = a0 * r.uniform(0.8, 1.0, B)
        X0[:, 3] = c["tau1_rest"] * r.uniform(1.0, 1.3, B)
        X0[:, 4] = c["km_rest"] * r.uniform(1.0, 1.3, B)
    kind = O.control_kind(pb.name)
    if kind == "pulse_width":
        U = r.uniform(c["pd0"], 6e-4, (B, pb.n_shooting, 1))
    elif kind == "pulse_intensity":
        U = r.uniform(max(20.0, 1.05 * O.min_pulse_intensity(c)), 130.0, (B, pb.n_shooting, pb.nu))
    else:
        U = np.zeros((B, pb.n_shooting, 0))
    return X0, U


SAME_ROOT = 1e-10  # two starts that differ by more than this did not reach the same solution
FIRST_SEED, SEED_TRIES = 11, 8


@functools.lru_cache(maxsize=None)
def reference(name, method, degree, n_shooting):
    """Ten pulses at 10 Hz over 1 s, truncation 10, B_MAX seeded instances: (pb, X0, U, traj, converged, eps_ref).

    The defect equations of the fatigue models have further, non-physical solutions (negative Tau1 / Km), and at the
    stiff step the plain Newton from the explicit-Euler predictor reaches one of them for about one instance in a
    thousand.  That is a different solution, not noise of the reference, so such a draw is not a usable input: the
    WHOLE input set is redrawn with the next seed (no instance is ever dropped) until both starts converge on every
    instance to the same trajectory.  Deterministic: the seeds are tried in order from FIRST_SEED."""
    pb = col_problem(name, cases.TEN_PULSES, 1.0, 10, n_shooting, degree, method)
    for seed in range(FIRST_SEED, FIRST_SEED + SEED_TRIES):
        X0, U = random_inputs(pb, B_MAX, seed)
        traj, conv = integrate(pb, X0, U, "copy")
        traj2, conv2 = integrate(pb, X0, U, "euler")
        eps = scaled_error(traj2, traj)
        if conv.all() and conv2.all() and eps <= SAME_ROOT:
            for a in (X0, U, traj):
                a.setflags(write=False)
            return pb, X0, U, traj, conv & conv2, eps
    raise AssertionError(f"no input set in {SEED_TRIES} draws on which both Newton starts agree: {name} {method} "
                         f"d={degree} N={n_shooting}")
