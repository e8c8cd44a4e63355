"""Automatic-differentiation oracle for the FES NLP callbacks — TEST INFRASTRUCTURE ONLY (CPU, torch float64).

Nothing in the product imports this module.  It restates, in torch float64 on the CPU, what ``fes_oracle`` and
``fes_collocation`` state in numpy: the right-hand sides of the six models (same reference lines, divisions written
as the reference writes them), the RK1/RK2/RK4 sub-stepping, the sliding-window rows, the quadratic objective terms
and the collocation defect / continuity rows.  The basis matrices, collocation points and stimulation tables are
taken from the numpy oracle as plain constants (they are not differentiated).

Why it exists: the numpy oracle's first derivatives are complex-step and exact to rounding, but its Hessian is a
Richardson-extrapolated central difference of those gradients, accurate to about 1e-9 .. 1e-7.  ``torch.func``
differentiates the same recursion twice with no step size, so the second-order reference is exact to rounding too.

    eval_g(pb, v), eval_jac_g(pb, v)            the numpy oracle's structure and order
    hessian_values(pb, v, obj_factor, lam)      packed order of ``hess_structure``: second-order AD of every
                                                interval's lam_k^T Phi_k (collocation: of its weighted rows) plus
                                                the objective diagonal
    hessian_scale(pb, v, obj_factor, lam)       sum_r |lam_r| |d2 Phi_r / dz_i dz_j| + |obj_factor| |d2 f|: the
                                                rounding scale of every entry, so that an entry that is small by
                                                cancellation between rows is judged against its summands
    hessian_error(pb, got, ref, scale)          max |got - ref| / max(scale, 1e-6 * largest |ref| of the entry's
                                                interval block): the comparison the tests use

``pb`` is an ``fes_oracle.Problem`` or a ``fes_collocation.ColProblem``.  ``mode`` selects how the second derivative
is taken: "fr" forward-over-reverse (default), "ff" forward-over-forward, "rr" reverse-over-reverse; the gap between
"ff" and "rr" is the reference's own rounding noise (tests/test_autodiff_oracle.py measures it).

Musculoskeletal problems are out of scope of this module: their oracle (``fes_msk``: rigid-body dynamics and muscle
geometry) is restated in ``msk_autodiff``, which reuses ``rhs`` (its ``fl`` / ``fv`` / ``fp`` / ``legacy`` arguments
exist for it; the defaults leave every result here bit-identical) and ``_step`` from this module.
"""

from __future__ import annotations

import numpy as np
import torch
from torch.func import grad, jacfwd, jacrev, jvp, vmap

from . import fes_collocation as CO
from . import fes_oracle as O

F64 = torch.float64


def _t(a):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=F64)


# --------------------------------------------------------------------------------------
# right-hand sides (x: (nx,), u: (nu,) or None, row: (T,), t: scalar; vmap adds the batch)
# --------------------------------------------------------------------------------------


def cn_sum(c, t, row, lam=None, legacy_skip_first=False):
    """ding2003.py:200-252 (ri_fun, exp_time_fun, cn_sum_fun); r0 = km_rest + 1.04 (268-272).
    ``legacy_skip_first`` as fes_oracle.cn_sum: once a window holds more than one real pulse its first term is left
    out (a 0 / 1 weight computed from the row, so that vmap goes through)."""
    r0 = c["km_rest"] + c["r0_km_relationship"]
    total = 0.0
    T = row.shape[-1]
    if legacy_skip_first:
        n_real = (row > -1e6).sum(dim=-1, keepdim=True)
        keep = torch.where((torch.arange(T) == T - n_real) & (n_real > 1), 0.0, 1.0).to(F64)
    for i in range(T):
        ri = 1.0 if i == 0 else 1 + (r0 - 1) * torch.exp(-(row[..., i] - row[..., i - 1]) / c["tauc"])
        term = ri * torch.exp(-(t - row[..., i]) / c["tauc"])
        if legacy_skip_first:
            term = term * keep[..., i]
        total = total + (term if lam is None else term * lam[i])
    return total


def lambda_i(c, intensity):
    """hmed2018.py:169-180."""
    return c["ar"] * (torch.tanh(c["bs"] * (intensity - c["Is"])) + c["cr"])


def a_calculation(c, a_scale, pulse_width):
    """ding2007.py:172-188."""
    return a_scale * (1 - torch.exp(-(pulse_width - c["pd0"]) / c["pdt"]))


def rhs(name, c, t, x, u, row, fl=1.0, fv=1.0, fp=0.0, legacy=False):
    """system_dynamics of the six models: ding2003.py:153-198, ding2003_with_fatigue.py:138-240,
    ding2007.py:121-170, ding2007_with_fatigue.py:133-241, hmed2018.py:119-167, hmed2018_with_fatigue.py:124-229.
    ``fl`` / ``fv`` / ``fp``: the Hill coefficients of the musculoskeletal model (1, 1, 0 without one); ``legacy``: the
    stored reaching-task revision's conventions, both as fes_oracle.rhs."""
    fatigue = name.endswith("with_fatigue")
    cn, f = x[0], x[1]
    lam = None
    if name.startswith("hmed2018"):
        lam = [lambda_i(c, u[i]) for i in range(row.shape[-1])]
    cs = cn_sum(dict(c, km_rest=x[4]) if (legacy and fatigue) else c, t, row, lam, legacy)
    cn_dot = (1 / c["tauc"]) * cs - (cn / c["tauc"])  # ding2003.py:254-266
    if fatigue:
        a, tau1, km = x[2], x[3], x[4]
    else:
        a = c["a_scale"] if name.startswith("ding2007") else c["a_rest"]
        tau1, km = c["tau1_rest"], c["km_rest"]
    if name.startswith("ding2007"):
        a = a_calculation(c, a, u[0])
    s = cn / (km + cn)
    # ding2003.py:274-311; with the defaults the factor is the float 1.0 and the product is exact
    f_dot = (a * s - (f / (tau1 + c["tau2"] * s))) * (fl * fv + fp)
    parts = [cn_dot, f_dot]
    if fatigue:
        a_rest = c["a_scale"] if name.startswith("ding2007") else c["a_rest"]
        parts.append(-(x[2] - a_rest) / c["tau_fat"] + c["alpha_a"] * f)
        parts.append(-(tau1 - c["tau1_rest"]) / c["tau_fat"] + c["alpha_tau1"] * f)
        parts.append(-(km - c["km_rest"]) / c["tau_fat"] + c["alpha_km"] * f)
    return torch.stack(parts)


def _step(scheme, f, t, h, x):
    """One sub-step: RK1 explicit Euler, RK2 explicit midpoint, RK4 classic (fes_oracle._step)."""
    if scheme == "RK1":
        return x + h * f(t, x)
    if scheme == "RK2":
        k1 = f(t, x)
        return x + h * f(t + h / 2, x + h / 2 * k1)
    if scheme == "RK4":
        k1 = f(t, x)
        k2 = f(t + h / 2, x + h / 2 * k1)
        k3 = f(t + h / 2, x + h / 2 * k2)
        k4 = f(t + h, x + h * k3)
        return x + h / 6 * (k1 + 2 * k2 + 2 * k3 + k4)
    raise ValueError(f"unknown scheme {scheme}")


# --------------------------------------------------------------------------------------
# the nonlinear rows of one interval as a function of its own variables z_k
# --------------------------------------------------------------------------------------


def _is_col(pb):
    return isinstance(pb, CO.ColProblem)


def _nzk(pb):
    """Variables of one interval: (x_k, u_k), or (x_k^0 .. x_k^d, u_k) under collocation."""
    return pb.nzc if _is_col(pb) else pb.nx + pb.nu


def _ngk(pb):
    return pb.ngk if _is_col(pb) else pb.nx + pb.n_slide


def _n_rows(pb):
    """Rows of one interval that ``_interval_rows`` returns (everything but the sliding-window rows)."""
    return (pb.degree + 1) * pb.nx if _is_col(pb) else pb.nx


def _interval_rows(pb):
    """rows(z, t0, row): shooting: Phi_m(x_k, u_k) (nx,); collocation: the d defect blocks and the continuity
    block's sum_i D[i] x_k^i ((d+1) nx,).  The -x_{k+1} of the continuity rows is added by the callers."""
    nx, nu, name, c, dt = pb.nx, pb.nu, pb.name, pb.c, pb.dt
    if not _is_col(pb):
        scheme, m = pb.scheme, pb.n_steps
        h = dt / m

        def phi(z, t0, row):
            x, u = z[:nx], (z[nx:] if nu else None)
            f = lambda t, xx: rhs(name, c, t, xx, u, row)  # noqa: E731
            for j in range(m):
                x = _step(scheme, f, t0 + j * h, h, x)
            return x

        return phi
    d = pb.degree
    tau, C, D = CO.coefficients(d, pb.method)

    def rows(z, t0, row):
        xc = [z[i * nx: (i + 1) * nx] for i in range(d + 1)]
        u = z[(d + 1) * nx:] if nu else None
        out = []
        for j in range(1, d + 1):
            poly = sum(float(C[i, j]) * xc[i] for i in range(d + 1))
            out.append(poly - dt * rhs(name, c, t0 + float(tau[j]) * dt, xc[j], u, row))
        out.append(sum(float(D[i]) * xc[i] for i in range(d + 1)))
        return torch.cat(out)

    return rows


def _interval_inputs(pb, v):
    """z (L, nzk), t0 (L,), stim rows (L, T) of every (instance, interval), L = B * N."""
    B, N, nzk = v.shape[0], pb.n_shooting, _nzk(pb)
    z = _t(v[:, : N * nzk]).reshape(B * N, nzk)
    t0 = _t(np.tile(np.arange(N) * pb.dt, B))
    rows = _t(np.tile(pb.rows[:N], (B, 1)))
    return z, t0, rows


def sliding_window(pb, P, k):
    """custom_constraints.py:102-119 (fes_oracle.sliding_window) on a torch P (B, n_params): (B, T)."""
    idx = pb.last_stim_idx[k]
    cols = [P[:, i] for i in range(idx + 1)]
    while len(cols) < pb.nu:
        cols.insert(0, torch.full((P.shape[0],), float(pb.intensity_floor), dtype=F64))
    return torch.stack(cols[len(cols) - pb.nu:], dim=1)


# --------------------------------------------------------------------------------------
# g and J_g
# --------------------------------------------------------------------------------------


def eval_g(pb, v):
    """Constraint vector in the numpy oracle's order (fes_oracle.eval_g / fes_collocation.eval_g)."""
    v = np.asarray(v, dtype=np.float64)
    B, N, nx, nr = v.shape[0], pb.n_shooting, pb.nx, _n_rows(pb)
    z, t0, rows = _interval_inputs(pb, v)
    r = vmap(_interval_rows(pb))(z, t0, rows).reshape(B, N, nr)
    vt = _t(v)
    nxt = torch.stack([vt[:, pb.x_off(k + 1): pb.x_off(k + 1) + nx] for k in range(N)], dim=1)
    r = torch.cat([r[:, :, : nr - nx], r[:, :, nr - nx:] - nxt], dim=2)
    if pb.n_slide:
        P = vt[:, pb.p_off:]
        U = torch.stack([vt[:, pb.u_off(k): pb.u_off(k) + pb.nu] for k in range(N)], dim=1)
        slide = torch.stack([U[:, k, :] - sliding_window(pb, P, k) for k in range(N)], dim=1)
        r = torch.cat([r, slide], dim=2)
    return r.reshape(B, -1).numpy()


def jac_dense(pb, v):
    """Dense J_g (B, ng, nv): forward-mode AD of every interval's rows; the -1 on x_{k+1} and the +1 / -1 of
    the (linear) sliding-window rows are entered directly."""
    v = np.asarray(v, dtype=np.float64)
    B, N, nx, nu, nr, nzk, ngk = v.shape[0], pb.n_shooting, pb.nx, pb.nu, _n_rows(pb), _nzk(pb), _ngk(pb)
    z, t0, rows = _interval_inputs(pb, v)
    blocks = vmap(jacfwd(_interval_rows(pb)))(z, t0, rows).reshape(B, N, nr, nzk).numpy()
    J = np.zeros((B, pb.ng, pb.nv))
    for k in range(N):
        g0 = k * ngk
        J[:, g0: g0 + nr, k * nzk: (k + 1) * nzk] = blocks[:, k]
        for r in range(nx):
            J[:, g0 + nr - nx + r, pb.x_off(k + 1) + r] += -1.0
        if pb.n_slide:
            first = pb.last_stim_idx[k] + 1 - nu
            for j in range(nu):
                J[:, g0 + nr + j, pb.u_off(k) + j] = 1.0
                if 0 <= first + j <= pb.last_stim_idx[k]:
                    J[:, g0 + nr + j, pb.p_off + first + j] = -1.0
    return J


def _mod(pb):
    return CO if _is_col(pb) else O


def eval_jac_g(pb, v):
    """J_g values in the numpy oracle's ``jac_structure`` order, (B, nnz)."""
    r, c = _mod(pb).jac_structure(pb)
    return jac_dense(pb, v)[:, r, c]


# --------------------------------------------------------------------------------------
# objective (quadratic tracking terms, fes_oracle.Objective)
# --------------------------------------------------------------------------------------


def _objective(pb):
    """f(v) of one instance as a torch function: sum of weight * c_k * (v[off] - target_k)^2."""
    offs, ws, tgts = [], [], []
    for ob in pb.objectives:
        scale = pb.dt if ob.kind == "lagrange" else 1.0
        kind, idx = ob.var
        for k in ob.nodes:
            offs.append((pb.x_off(k) if kind == "x" else pb.u_off(k)) + idx)
            ws.append(ob.weight * scale)
            tgts.append(float(ob.target[k]))
    offs = torch.tensor(offs, dtype=torch.int64)
    ws, tgts = torch.tensor(ws, dtype=F64), torch.tensor(tgts, dtype=F64)

    def f(v):
        return (ws * (v[offs] - tgts) ** 2).sum() if len(offs) else (v * 0.0).sum()

    return f


def eval_f(pb, v):
    return vmap(_objective(pb))(_t(v)).numpy()


def eval_grad_f(pb, v):
    return vmap(grad(_objective(pb)))(_t(v)).numpy()


def objective_hessian_diagonal(pb, v):
    """(B, nv): the objective is a sum of squares of single variables, so its Hessian is diagonal and equals
    Hess(f) @ 1, one forward derivative of the reverse gradient."""
    gf = grad(_objective(pb))
    return vmap(lambda x: jvp(gf, (x,), (torch.ones_like(x),))[1])(_t(v)).numpy()


# --------------------------------------------------------------------------------------
# Lagrangian Hessian
# --------------------------------------------------------------------------------------

_MODES = {"fr": (jacfwd, jacrev), "ff": (jacfwd, jacfwd), "rr": (jacrev, jacrev)}


def _row_weights(pb, lam):
    """The multipliers of every interval's nonlinear rows (L, nr); the sliding-window rows are linear."""
    B, N = lam.shape[0], pb.n_shooting
    return _t(np.asarray(lam, dtype=np.float64).reshape(B, N, _ngk(pb))[:, :, : _n_rows(pb)]).reshape(B * N, -1)


def hessian_blocks(pb, v, lam, mode="fr"):
    """(B, N, nzk, nzk): Hessian over z_k of lam_k^T rows_k(z_k), by second-order AD."""
    v = np.asarray(v, dtype=np.float64)
    outer, inner = _MODES[mode]
    fn = _interval_rows(pb)
    z, t0, rows = _interval_inputs(pb, v)
    w = _row_weights(pb, lam)
    scalar = lambda zz, ww, tt, rr: (ww * fn(zz, tt, rr)).sum()  # noqa: E731
    H = vmap(outer(inner(scalar)))(z, w, t0, rows)
    return H.reshape(v.shape[0], pb.n_shooting, _nzk(pb), _nzk(pb)).numpy()


def hessian_scale_blocks(pb, v, lam):
    """(B, N, nzk, nzk): sum_r |lam_r| |Hess(rows_r)|, from the per-row Hessians."""
    v = np.asarray(v, dtype=np.float64)
    z, t0, rows = _interval_inputs(pb, v)
    w = _row_weights(pb, lam)
    Hr = vmap(jacfwd(jacrev(_interval_rows(pb))))(z, t0, rows)  # (L, nr, nzk, nzk)
    S = torch.einsum("lr,lrij->lij", w.abs(), Hr.abs())
    return S.reshape(v.shape[0], pb.n_shooting, _nzk(pb), _nzk(pb)).numpy()


def hessian_block_index(pb):
    """Interval block of every packed Hessian entry: k for the entries of z_k, N for the x_N diagonal."""
    r, _ = _mod(pb).hess_structure(pb)
    return np.minimum(r // _nzk(pb), pb.n_shooting)


def _pack(pb, blocks, diag):
    """Dense interval blocks + the diagonal (B, nv) -> values in ``hess_structure`` order."""
    r, c = _mod(pb).hess_structure(pb)
    nzk, N = _nzk(pb), pb.n_shooting
    k = hessian_block_index(pb)
    assert np.all(c // nzk == r // nzk), "a Hessian entry couples two intervals"
    inner = k < N
    out = np.zeros((blocks.shape[0], r.size))
    out[:, inner] = blocks[:, k[inner], r[inner] - k[inner] * nzk, c[inner] - k[inner] * nzk]
    on_diag = r == c
    out[:, on_diag] += diag[:, r[on_diag]]
    return out


def hessian_values(pb, v, obj_factor, lam, mode="fr"):
    """obj_factor * Hess(f) + sum_r lam_r Hess(g_r) in the packed order of ``hess_structure``, (B, nnz)."""
    of = np.broadcast_to(np.asarray(obj_factor, dtype=np.float64), (np.shape(v)[0],))
    diag = of[:, None] * objective_hessian_diagonal(pb, v)
    return _pack(pb, hessian_blocks(pb, v, lam, mode), diag)


def hessian_scale(pb, v, obj_factor, lam):
    """sum_r |lam_r| |d2 g_r / dz_i dz_j| + |obj_factor| |d2 f / dz_i dz_j| in packed order, (B, nnz)."""
    of = np.broadcast_to(np.asarray(obj_factor, dtype=np.float64), (np.shape(v)[0],))
    diag = np.abs(of)[:, None] * np.abs(objective_hessian_diagonal(pb, v))
    return _pack(pb, hessian_scale_blocks(pb, v, lam), diag)


def hessian_error(pb, got, ref, scale, floor=1e-6):
    """max over entries of |got - ref| / max(scale, floor * largest |ref| of the entry's interval block).  A block
    whose reference is identically zero must be matched exactly."""
    got, ref, scale = np.asarray(got), np.asarray(ref), np.asarray(scale)
    k = hessian_block_index(pb)
    blockmax = np.zeros((ref.shape[0], pb.n_shooting + 1))
    for b in range(pb.n_shooting + 1):
        if np.any(k == b):
            blockmax[:, b] = np.max(np.abs(ref[:, k == b]), axis=1)
    s = np.maximum(scale, floor * blockmax[:, k]) + 1e-300
    return float(np.max(np.abs(got - ref) / s)) if ref.size else 0.0
