"""Exact-AD reference of the force-parameter identification — TEST INFRASTRUCTURE ONLY (CPU, torch float64).

The single-shooting trajectory from the rest state is rolled out as a function of the identified parameters theta
with ``oracle.fes_autodiff.rhs`` and ``_step`` unchanged (``rhs`` takes the constants as a dict whose values may be
tensors), and differentiated with ``torch.func.jacfwd`` (``jacrev`` for the reference-noise measurement): no step
size, so the sensitivities are exact to rounding.  ``lm_reference`` is a plain Levenberg-Marquardt with the update
rule of ``cocofest_amd.identification.lm_solve``, written out on its own on dense matrices, as the CPU comparator
of the fits.
"""

from __future__ import annotations

import numpy as np
import torch
from torch.func import jacfwd, jacrev, vmap

from oracle import fes_autodiff as AD
from oracle import fes_oracle as O

F64 = torch.float64

# the models' identifiable parameters, in the order the tests use as "the full valid set"
FULL_KEYS = {
    "ding2003": ["a_rest", "km_rest", "tau1_rest", "tau2"],
    "ding2007": ["a_scale", "km_rest", "tau1_rest", "tau2", "pd0", "pdt"],
    "hmed2018": ["a_rest", "km_rest", "tau1_rest", "tau2", "ar", "bs", "Is", "cr"],
}


class Setup:
    """One experiment: model, pulse train, grid, scheme, controls (interval-major [N][nu]) and default constants."""

    def __init__(self, name, stims, final_time, n_shooting, truncation, scheme, m, pulse_width=None,
                 pulse_intensity=None):
        self.name, self.scheme, self.m, self.N, self.T = name, scheme, m, n_shooting, truncation
        self.final_time, self.dt = final_time, final_time / n_shooting
        self.c = O.model_constants(name)
        self.table = O.stim_table(stims, n_shooting, final_time, truncation)
        self.rows = AD._t(self.table.rows)
        u = O.ivp_controls(name, self.table, n_shooting, truncation, pulse_width, pulse_intensity)
        self.controls = None if u is None or np.size(u) == 0 else AD._t(np.asarray(u, dtype=float).reshape(n_shooting, -1))

    def defaults(self, keys):
        return np.array([self.c[k] for k in keys], dtype=float)

    def trajectory(self, keys):
        """theta (n_id,) -> node forces (N + 1,)."""
        h = self.dt / self.m

        def traj(theta):
            c = dict(self.c)
            for j, k in enumerate(keys):
                c[k] = theta[j]
            x = torch.zeros(2, dtype=F64) + 0.0 * theta[0]
            out = [x[1]]
            for k in range(self.N):
                u = None if self.controls is None else self.controls[k]
                row = self.rows[k]
                f = lambda t, xx: AD.rhs(self.name, c, t, xx, u, row)  # noqa: E731
                for j in range(self.m):
                    x = AD._step(self.scheme, f, k * self.dt + j * h, h, x)
                out.append(x[1])
            return torch.stack(out)

        return traj

    def forces(self, keys, theta):
        """theta (n_id, B) numpy -> forces (N + 1, B)."""
        with torch.no_grad():
            return vmap(self.trajectory(keys))(AD._t(theta.T)).T.numpy()

    def forces_and_sens(self, keys, theta, mode="fwd"):
        """theta (n_id, B) numpy -> forces (N + 1, B), sensitivities (N + 1, n_id, B)."""
        traj = self.trajectory(keys)
        jac = jacfwd if mode == "fwd" else jacrev
        th = AD._t(theta.T)
        F = vmap(traj)(th)
        S = vmap(jac(traj))(th)  # (B, N + 1, n_id)
        return F.T.numpy(), S.permute(1, 2, 0).numpy()

    def normal(self, keys, target, weight):
        """theta (n, B) tensor -> cost (B,), grad (B, n), H (B, n, n) of dt sum_k w_k (F_k - y_k)^2 (Gauss-Newton)."""
        traj = self.trajectory(keys)
        y, w = AD._t(target), AD._t(weight)

        def fn(theta):
            F = vmap(traj)(theta.T)
            S = vmap(jacfwd(traj))(theta.T)
            r = F - y
            cost = self.dt * (w * r * r).sum(dim=1)
            grad = 2 * self.dt * torch.einsum("k,bk,bkj->bj", w, r, S)
            H = 2 * self.dt * torch.einsum("k,bki,bkj->bij", w, S, S)
            return cost, grad, H

        return fn


def lm_reference(normal, theta0, lo, hi, max_iter=100, gtol=1e-8, xtol=1e-10, mu0=1e-3):
    """Levenberg-Marquardt with the product's update rule (identification.lm_solve), on the CPU.  theta0, lo, hi:
    (n, B) numpy.  Returns theta (n, B), cost (B,), iterations (B,), status (B,), cost history (its + 1, B)."""
    th0 = AD._t(theta0)
    n, B = th0.shape
    s = th0.abs().clamp_min(1e-300).T  # (B, n)
    x, xl, xu = th0.T / s, AD._t(lo).T / s, AD._t(hi).T / s

    def ev(xx):
        c, g, H = normal((xx * s).T)
        return c, g * s, H * (s[:, :, None] * s[:, None, :])

    c, g, H = ev(x)
    c0 = c.clone()
    mu, nu = torch.full((B,), mu0, dtype=F64), torch.full((B,), 2.0, dtype=F64)
    status, iters = torch.zeros(B, dtype=torch.int32), torch.zeros(B, dtype=torch.int32)
    hist = [c.clone()]
    for _ in range(max_iter):
        active = ((x <= xl) & (g > 0)) | ((x >= xu) & (g < 0))
        pg = torch.where(active, torch.zeros_like(g), g)
        status[(status == 0) & (pg.abs().amax(dim=1) <= gtol * c0.clamp_min(1.0))] = 1
        live = status == 0
        if not bool(live.any()):
            break
        free = (~active).to(F64)
        Hf = H * free[:, :, None] * free[:, None, :]
        d = torch.diagonal(Hf, dim1=1, dim2=2)
        damp = mu[:, None] * (d + 1e-12 * d.amax(dim=1, keepdim=True) + 1e-300) + (1.0 - free)
        dx = torch.linalg.solve_ex(Hf + torch.diag_embed(damp), -pg[:, :, None])[0][:, :, 0]
        dx = torch.where(torch.isfinite(dx), dx, torch.zeros_like(dx))
        xt = torch.minimum(torch.maximum(x + dx, xl), xu)
        dx = xt - x
        ct, gt, Ht = ev(xt)
        pred = -((g * dx).sum(dim=1) + 0.5 * torch.einsum("bi,bij,bj->b", dx, H, dx))
        rho = (c - ct) / pred.clamp_min(1e-300)
        ok = live & torch.isfinite(ct) & (rho > 1e-4) & (ct <= c)
        small = live & (dx.abs().amax(dim=1) <= xtol)
        x = torch.where(ok[:, None], xt, x)
        g = torch.where(ok[:, None], gt, g)
        H = torch.where(ok[:, None, None], Ht, H)
        c = torch.where(ok, ct, c)
        shrink = (1.0 - (2.0 * rho - 1.0) ** 3).clamp(min=1.0 / 3.0)
        mu = torch.where(ok, mu * shrink, torch.where(live, mu * nu, mu)).clamp(1e-15, 1e15)
        nu = torch.where(ok, torch.full_like(nu, 2.0), torch.where(live, nu * 2.0, nu))
        iters = iters + live.to(torch.int32)
        status[small & ok] = 2
        status[small & ~ok] = 3  # stalled: small only because rejected trials inflated the damping
        hist.append(c.clone())
    return (x * s).T.numpy(), c.numpy(), iters.numpy(), status.numpy(), torch.stack(hist).numpy()


def scaled_errors(force, sens, ref_force, ref_sens):
    """Per instance: force error over its max |F| over the nodes; column j of the sensitivities over that column's
    max |S| over the nodes.  Returns (largest force error, (n_id,) largest error of every column)."""
    ef = np.max(np.max(np.abs(force - ref_force), axis=0) / np.max(np.abs(ref_force), axis=0))
    es = np.max(np.max(np.abs(sens - ref_sens), axis=0) / np.max(np.abs(ref_sens), axis=0), axis=1)
    return float(ef), es
