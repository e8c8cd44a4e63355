"""An independent first-order (KKT) certificate for what the interior-point solvers return.

Everything here is numpy and the float64 oracle (oracle.fes_oracle for shooting, oracle.fes_collocation for
collocation); nothing is imported from cocofest_amd.solver, and the check needs no knowledge of the path the solver
took.  Test infrastructure only.

Convention certified: at the returned (v, y, z_l, z_u) of   min f(v)  s.t.  g(v) = 0,  lb <= v <= ub

    grad f + J_g^T y - z_l + z_u = 0  on the free variables (lb != ub),   g = 0,
    (v - lb) z_l = 0,  (ub - v) z_u = 0,   z_l, z_u >= 0, exactly 0 at fixed variables and at infinite bounds,

with lb / ub relaxed by bound_relax_factor * max(1, |bound|), the problem the iteration works on.

Ipopt's scaled error (IpIpoptCalculatedQuantities::curr_nlp_error) is restated from the scalings up:

    d    variable scaling x = d x~: the bound range where it is finite and below 1, else 1 (range_scaling=False: 1)
    sf   min(1, max_gradient / max_i |d_i grad f_i|), at least nlp_scaling_min_value          ("none": 1)
    sg_k min(1, max_gradient / max_i |d_i J_ki|),     at least nlp_scaling_min_value          ("none": 1)
    y~ = sf y / sg,  z~ = sf d z,  s~ = (v - lb) / d
    rd~_i = sf d_i grad f_i + sum_k (sg_k d_i J_ki) y~_k - z~_l,i + z~_u,i
    s_d = max(s_max, (|y~|_1 + |z~_l|_1 + |z~_u|_1) / (2 nf + m)) / s_max,  s_c = max(s_max, (|z~_l|_1 + |z~_u|_1) / (2 nf)) / s_max
    error = max( max|rd~| / s_d,  max|sg g|,  max|s~ z~| / s_c )

sf and sg are evaluated at ``v_start`` with the fixed entries of ``v`` in place: Ipopt's gradient-based scaling
(IpGradientScaling) evaluates the user's starting point, before its iterate initialiser pushes that point from the
bounds (bound_push / bound_frac), and so do both solvers here.  The push does not enter sf or sg; callers pass the
start they gave the solver.

Rounding allowance: every residual is a sum whose terms reach 1e4 .. 1e7 at active pulse-width bounds and cancel, so
each carries  64 eps * (sum of the absolute values of the terms added)  rather than an absolute constant; ``gap``
entries are the same sums times an evaluation tolerance ``eval_rel`` (the project's GPU-vs-oracle parity tolerance on
g, J_g and grad f), for comparisons with numbers a GPU run reports.
"""

from __future__ import annotations

import numpy as np

from oracle import fes_collocation as CO
from oracle import fes_oracle as O

EPS = float(np.finfo(np.float64).eps)
ULPS = 64.0
SLACK_MOVE = EPS ** 0.75  # Ipopt's slack_move: a slack below eps min(1, mu) moves its bound out by this much


def _mod(pb):
    return CO if isinstance(pb, CO.ColProblem) else O


def dense_jacobian(pb, v):
    """J_g (B, ng, nv) from the oracle's triplets."""
    M = _mod(pb)
    r, c = M.jac_structure(pb)
    vals = np.asarray(M.eval_jac_g(pb, v), dtype=np.float64)
    J = np.zeros((vals.shape[0], pb.ng, pb.nv))
    for b in range(vals.shape[0]):
        np.add.at(J[b], (np.asarray(r, dtype=np.int64), np.asarray(c, dtype=np.int64)), vals[b])
    return J


def variable_scaling(lb, ub, options):
    """d (nv,): the bound range where finite and below 1 (free variables, range_scaling), else 1."""
    with np.errstate(invalid="ignore"):
        width = ub - lb
    small = np.isfinite(width) & (width < 1.0) & (lb != ub) & bool(options.range_scaling)
    return np.where(small, width, 1.0)


def relaxed_bounds(lb, ub, options):
    """The bounds of the problem the iteration works on: free ones moved out by bound_relax_factor max(1, |bound|)."""
    rel = float(options.bound_relax_factor)
    free = lb != ub
    lbr = np.where(free & np.isfinite(lb), lb - rel * np.maximum(np.abs(lb), 1.0), lb)
    ubr = np.where(free & np.isfinite(ub), ub + rel * np.maximum(np.abs(ub), 1.0), ub)
    return lbr, ubr


def function_scaling(pb, lb, ub, v_start, options):
    """(sf (B,), sg (B, ng)) of Ipopt's gradient-based rule at ``v_start``."""
    B = v_start.shape[0]
    if options.nlp_scaling_method == "none":
        return np.ones(B), np.ones((B, pb.ng))
    M = _mod(pb)
    free = lb != ub
    d = variable_scaling(lb, ub, options)
    gm, lo = float(options.nlp_scaling_max_gradient), float(options.nlp_scaling_min_value)
    grad = np.asarray(M.eval_grad_f(pb, v_start))
    J = dense_jacobian(pb, v_start)
    gmax = np.abs(grad[:, free] * d[free]).max(1)
    rmax = np.abs(J[:, :, free] * d[free]).max(2)
    with np.errstate(divide="ignore"):
        sf = np.maximum(np.minimum(1.0, gm / gmax), lo)
        sg = np.maximum(np.minimum(1.0, gm / rmax), lo)
    return sf, sg


def certificate(pb, lb, ub, v, y, z_l, z_u, v_start, options, eval_rel=1e-9):
    """First-order conditions of the unscaled NLP at (v, y, z_l, z_u), per instance (arrays of length B unless noted).

    ``options`` is read by attribute (bound_relax_factor, honor_original_bounds, range_scaling, nlp_scaling_method,
    nlp_scaling_max_gradient, nlp_scaling_min_value, s_max).  Keys: stationarity, feasibility, bound_violation,
    complementarity (each with its ``*_allow``), nonnegative / zero_where_no_bound / finite (bool), scaled_error with
    its parts e_d, e_p, e_c, scaled_allow and scaled_gap, the scalings d (nv,), sf, sg (B, ng), s_d, s_c, and the
    residual vectors r (B, nv) and g (B, ng)."""
    M = _mod(pb)
    lb, ub = np.asarray(lb, dtype=np.float64), np.asarray(ub, dtype=np.float64)
    v, y, z_l, z_u = (np.atleast_2d(np.asarray(a, dtype=np.float64)) for a in (v, y, z_l, z_u))
    B = v.shape[0]
    free = lb != ub
    nf, m = int(free.sum()), pb.ng
    hasL, hasU = free & np.isfinite(lb), free & np.isfinite(ub)
    start = np.array(np.atleast_2d(v_start), dtype=np.float64)
    start[:, ~free] = v[:, ~free]
    d = variable_scaling(lb, ub, options)
    sf, sg = function_scaling(pb, lb, ub, start, options)
    lbr, ubr = relaxed_bounds(lb, ub, options)

    grad = np.asarray(M.eval_grad_f(pb, v))
    g = np.asarray(M.eval_g(pb, v)).reshape(B, m)
    J = dense_jacobian(pb, v)
    aJ = np.abs(J)

    # unscaled stationarity on the free variables
    r = np.where(free, grad + np.einsum("bkj,bk->bj", J, y) - z_l + z_u, 0.0)
    r_terms = np.where(free, np.abs(grad) + np.einsum("bkj,bk->bj", aJ, np.abs(y)) + np.abs(z_l) + np.abs(z_u), 0.0)
    # g's terms: x_{k+1} - Phi(x_k, u_k) cancels quantities of the size |J| |v| (first order)
    g_terms = np.einsum("bkj,bj->bk", aJ, np.abs(v))
    # complementarity against the relaxed bounds
    with np.errstate(invalid="ignore"):
        sl = np.where(hasL, v - lbr, 0.0)
        su = np.where(hasU, ubr - v, 0.0)
    cl, cu = sl * np.where(hasL, z_l, 0.0), su * np.where(hasU, z_u, 0.0)
    c_terms = np.maximum(np.where(hasL, (np.abs(v) + np.abs(lbr)) * np.abs(z_l), 0.0),
                         np.where(hasU, (np.abs(v) + np.abs(ubr)) * np.abs(z_u), 0.0))
    # bound violation: original bounds under honor_original_bounds, else the relaxed ones.  A bound may have been moved
    # out by Ipopt's slack_move (in the scaled variable: max(d, |bound|) here) and v = d x~ rounds once
    lo_b, up_b = (lb, ub) if options.honor_original_bounds else (lbr, ubr)
    with np.errstate(invalid="ignore"):
        below = np.where(hasL, lo_b - v, -np.inf)
        above = np.where(hasU, v - up_b, -np.inf)
    viol = np.maximum(np.maximum(below, above), 0.0)
    b_allow = (SLACK_MOVE + 4 * EPS) * np.maximum(d, np.maximum(np.where(hasL, np.abs(lo_b), 0.0),
                                                               np.where(hasU, np.abs(up_b), 0.0)))
    excess = np.where(free, viol - b_allow, -np.inf)

    # structural facts
    nonneg = (z_l >= 0).all(1) & (z_u >= 0).all(1)
    zero = (z_l[:, ~hasL] == 0).all(1) & (z_u[:, ~hasU] == 0).all(1)
    finite = np.array([all(np.isfinite(a[b]).all() for a in (v, y, z_l, z_u)) for b in range(B)])

    # Ipopt's scaled error, restated (module docstring)
    ys = sf[:, None] * y / sg
    zls = np.where(hasL, sf[:, None] * d * z_l, 0.0)
    zus = np.where(hasU, sf[:, None] * d * z_u, 0.0)
    gF = sf[:, None] * d * grad
    jv = J * d[None, None, :] * sg[:, :, None]
    rds = np.where(free, gF + np.einsum("bkj,bk->bj", jv, ys) - zls + zus, 0.0)
    rds_terms = np.where(free, np.abs(gF) + np.einsum("bkj,bk->bj", np.abs(jv), np.abs(ys)) + np.abs(zls) + np.abs(zus),
                         0.0)
    s_max = float(options.s_max)
    zsum = np.abs(zls).sum(1) + np.abs(zus).sum(1)
    s_d = np.maximum(s_max, (zsum + np.abs(ys).sum(1)) / (2 * nf + m)) / s_max
    s_c = np.maximum(s_max, zsum / (2 * nf)) / s_max
    cs = np.maximum(np.abs(sl / d * zls), np.abs(su / d * zus))
    e_d = np.abs(rds).max(1) / s_d
    e_p = np.abs(g * sg).max(1) if m else np.zeros(B)
    e_c = cs.max(1) / s_c
    cs_terms = sf[:, None] * c_terms

    def spread(k):
        # |max a - max b| <= max |a - b|: the largest per-entry term sum bounds the error of each maximum
        p = (g_terms * sg).max(1) if m else np.zeros(B)
        return k * np.maximum(np.maximum(rds_terms.max(1) / s_d, p), cs_terms.max(1) / s_c)

    return dict(
        stationarity=np.abs(r).max(1), stationarity_allow=ULPS * EPS * r_terms.max(1),
        feasibility=np.abs(g).max(1) if m else np.zeros(B), feasibility_allow=ULPS * EPS * g_terms.max(1, initial=0.0),
        bound_violation=np.maximum(excess.max(1), 0.0), bound_violation_raw=viol.max(1),
        complementarity=np.maximum(np.abs(cl).max(1), np.abs(cu).max(1)),
        complementarity_allow=ULPS * EPS * c_terms.max(1),
        nonnegative=nonneg, zero_where_no_bound=zero, finite=finite,
        scaled_error=np.maximum(np.maximum(e_d, e_p), e_c), e_d=e_d, e_p=e_p, e_c=e_c,
        scaled_allow=spread(ULPS * EPS),
        # a GPU run's g, J_g and grad f are within eval_rel of the oracle's; sf and sg are themselves quotients of such
        # values, so every product above carries at most three such factors
        scaled_gap=spread(3.0 * eval_rel),
        d=d, sf=sf, sg=sg, s_d=s_d, s_c=s_c, r=r, g=g, lb_relaxed=lbr, ub_relaxed=ubr)


def assert_certified(c, tol, what=""):
    """The assertions that follow from  scaled error <= tol  at the returned point (``c`` from certificate()):

    * scaled error: the solver stopped on err <= tol computed from its own evaluations; recomputed in float64 from the
      oracle's it may differ by rounding:  <= tol + scaled_allow.
    * feasibility: max_k |sg_k g_k| <= tol, so |g_k| <= tol / sg_k <= tol / min(sg), plus g's rounding.
    * complementarity: s~ z~ = ((v - lb) / d) (sf d z) = sf (v - lb) z, and max|s~ z~| / s_c <= tol, so
      (v - lb) z_l <= tol s_c / sf (likewise the upper side), plus the products' rounding.
    * bounds: the iterate stays strictly inside the (relaxed, possibly slack-moved) bounds.
    * structure: z >= 0; exactly 0 where there is no bound to be active (fixed variables, infinite bounds); finite.
    Every instance is checked."""
    B = c["scaled_error"].shape[0]
    for b in range(B):
        tag = f"{what} instance {b}"
        assert c["finite"][b] and c["nonnegative"][b] and c["zero_where_no_bound"][b], tag
        assert c["scaled_error"][b] <= tol + c["scaled_allow"][b], \
            (tag, c["scaled_error"][b], c["e_d"][b], c["e_p"][b], c["e_c"][b], c["scaled_allow"][b])
        assert c["feasibility"][b] <= tol / c["sg"][b].min(initial=1.0) + c["feasibility_allow"][b], \
            (tag, c["feasibility"][b])
        assert c["bound_violation"][b] == 0.0, (tag, c["bound_violation_raw"][b])
        assert c["complementarity"][b] <= tol * c["s_c"][b] / c["sf"][b] + c["complementarity_allow"][b], \
            (tag, c["complementarity"][b])


def describe(c):
    """One line per instance, for -s runs and failure messages."""
    return "; ".join(f"[{b}] err {c['scaled_error'][b]:.2e} (d {c['e_d'][b]:.1e} p {c['e_p'][b]:.1e} c {c['e_c'][b]:.1e}"
                     f" allow {c['scaled_allow'][b]:.1e} gap {c['scaled_gap'][b]:.1e}) stat {c['stationarity'][b]:.1e} "
                     f"feas {c['feasibility'][b]:.1e} compl {c['complementarity'][b]:.1e} sf {c['sf'][b]:.2e} "
                     f"sg_min {c['sg'][b].min(initial=1.0):.2e}" for b in range(c["scaled_error"].shape[0]))


def active_jacobian(pb, lb, ub, v, options, frac=1e-6):
    """For one instance (v (nv,)): the rows of J_g and the unit rows of the active bounds, over the free variables,
    and the boolean masks (active_lower, active_upper) over all variables.  A bound counts as active when the slack
    to the relaxed bound is below ``frac`` of the range (of max(1, |bound|) for one-sided bounds)."""
    free = lb != ub
    lbr, ubr = relaxed_bounds(lb, ub, options)
    with np.errstate(invalid="ignore"):
        rng = np.where(np.isfinite(ub - lb), ub - lb, np.maximum(1.0, np.minimum(np.abs(lb), np.abs(ub))))
        actL = free & np.isfinite(lb) & (v - lbr <= frac * rng)
        actU = free & np.isfinite(ub) & (ubr - v <= frac * rng)
    J = dense_jacobian(pb, v[None])[0][:, free]
    E = np.eye(lb.size)[actL | actU][:, free]
    return np.vstack([J, E]), actL, actU
