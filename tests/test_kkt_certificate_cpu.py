"""The interior point's executable specification (BatchedIpm on the CPU: oracle callbacks, dense band solver)
certified by tests/kkt_certificate.py: what it returns — v, y and the bound multipliers — satisfies the first-order
conditions of the unscaled NLP, checked in numpy from the oracle alone.

What is asserted follows from the solver's stopping rule, scaled error <= tol (kkt_certificate.assert_certified has
the derivation line by line):

    recomputed scaled error <= tol + rounding,          max|g| <= tol / min(sg) + rounding,
    (v - lb) z_l, (ub - v) z_u <= tol s_c / sf + rounding,   no bound violated,
    z_l, z_u >= 0 and exactly 0 at fixed variables and infinite bounds, everything finite,

with `rounding` = 64 eps * (sum of the absolute values of the terms of the residual in question).  No instance is
left out.  The mutation controls show the certificate is not vacuous: each wrong convention a solver could ship
(a scale applied twice, swapped or negated multipliers, a dropped multiplier) moves the recomputed error of the
ding2007 result above 100 tol."""

import functools

import numpy as np
import pytest

from tests import cases
from tests.kkt_certificate import assert_certified, certificate, describe
from tests.oracle_handle import DenseBandSolver, OracleHandle, oracle_problem_from_ocp

TOL = 1e-8
T11 = np.linspace(0, 1, 11)
FOUR = [0.0, 0.05, 0.1, 0.15]
SCALINGS = [(True, "gradient-based"), (False, "gradient-based"), (True, "none"), (False, "none")]


def four_pulse_cfg(name, scheme="RK1", m=5):
    return dict(name=name, stims=FOUR, final_time=0.2, truncation=4, scheme=scheme, m=m,
                objective={"force_tracking": [T11, 40 * T11]}, n_shooting=None)


@functools.lru_cache(maxsize=None)
def problem(kind):
    """(product ocp, oracle problem) of a named case."""
    if kind in ("ding2007", "hmed2018"):
        cfg = four_pulse_cfg(kind)
    elif kind == "fatigue":
        cfg = four_pulse_cfg("ding2007_with_fatigue", "RK4", 3)
    elif kind == "cfg2":
        cfg = cases.cfg2(n_shooting=None)
    elif kind == "collocation":
        ocp = cases.product_collocation_ocp("ding2007", FOUR, 0.2, 4, degree=3, method="legendre",
                                            objective={"force_tracking": [T11, 40 * T11]})
        return ocp, oracle_problem_from_ocp(ocp)
    else:
        raise KeyError(kind)
    return cases.product_ocp(**cfg), cases.oracle_problem(**cfg)


def starts(ocp, B, seed, spread=10.0):
    """The problem's initial guess, every instance but the first moved by a random part of each range."""
    v0 = np.tile(ocp.initial_guess_vector(), (B, 1))
    rng = np.random.default_rng(seed)
    lb, ub = ocp.bounds_vector()
    free = lb != ub
    step = rng.uniform(0, 1, (B, free.sum())) * np.minimum(ub[free] - lb[free], spread)
    step[0] = 0.0
    v0[:, free] = np.clip(v0[:, free] + step, lb[free], ub[free])
    return v0


def specification(kind, v0, **opts):
    """BatchedIpm on the CPU: (result, z_l, z_u, options)."""
    from cocofest_amd.solver import BatchedIpm, IpmOptions

    ocp, pb = problem(kind)
    B = v0.shape[0]
    options = IpmOptions(**opts)
    ipm = BatchedIpm(ocp, batch=B, options=options, handle=OracleHandle(pb, B), torch_device="cpu",
                     band=DenseBandSolver())
    res = ipm.solve(v0)
    z_l, z_u = ipm.last_bound_multipliers
    return res, z_l, z_u, options


@functools.lru_cache(maxsize=None)
def _certified(kind, range_scaling, method, relax=0.0):
    ocp, pb = problem(kind)
    lb, ub = ocp.bounds_vector()
    v0 = starts(ocp, 2, 11)
    res, z_l, z_u, options = specification(kind, v0, tol=TOL, max_iter=300, range_scaling=range_scaling,
                                           nlp_scaling_method=method, bound_relax_factor=relax)
    c = certificate(pb, lb, ub, res.v, res.y, z_l, z_u, v0, options)
    return ocp, pb, v0, res, z_l, z_u, options, c


@pytest.mark.parametrize("range_scaling,method", SCALINGS)
@pytest.mark.parametrize("kind", ["ding2007", "hmed2018", "cfg2", "collocation"])
def test_specification_returns_a_kkt_point(kind, range_scaling, method):
    ocp, pb, v0, res, z_l, z_u, options, c = _certified(kind, range_scaling, method)
    print(kind, range_scaling, method, "iterations", res.iterations, describe(c))
    assert (res.status == 0).all(), (res.status, res.kkt_error)
    assert z_l.shape == z_u.shape == res.v.shape
    assert_certified(c, TOL, what=kind)
    # the number the solver reports is the recomputed one (same evaluations here: the oracle's), to rounding
    assert np.all(res.kkt_error <= TOL)
    assert np.all(np.abs(res.kkt_error - c["scaled_error"]) <= c["scaled_allow"]), (res.kkt_error, c["scaled_error"])


@pytest.mark.parametrize("kind", ["ding2007", "hmed2018"])
def test_specification_with_relaxed_bounds(kind):
    """bound_relax_factor = 1e-8 (Ipopt's default): certified against the relaxed bounds, the problem iterated on."""
    ocp, pb, v0, res, z_l, z_u, options, c = _certified(kind, True, "gradient-based", 1e-8)
    print(kind, "relaxed", describe(c))
    assert (res.status == 0).all()
    assert_certified(c, TOL, what=kind)


def _mutations(c, y, z_l, z_u, lb, ub, v):
    """The wrong conventions: name -> (y, z_l, z_u)."""
    free = lb != ub
    d = c["d"]
    # an active bound: the largest multiplier of the first instance
    zz = np.where(free, np.maximum(z_l[0], z_u[0]), 0.0)
    i = int(np.argmax(zz))
    zl0, zu0 = z_l.copy(), z_u.copy()
    zl0[:, i] = 0.0
    zu0[:, i] = 0.0
    return {"y scaled by sg once more": (y * c["sg"], z_l, z_u),
            "z_l and z_u swapped": (y, z_u, z_l),
            "z multiplied by d": (y, z_l * d, z_u * d),
            "y negated": (-y, z_l, z_u),
            "one active z set to 0": (y, zl0, zu0)}, i


@pytest.mark.parametrize("mutation", ["y scaled by sg once more", "z_l and z_u swapped", "z multiplied by d",
                                      "y negated", "one active z set to 0"])
def test_mutation_controls_fail_the_certificate(mutation):
    """Each wrong convention drives the recomputed scaled error of the ding2007 result (gradient-based scaling and
    range scaling on: d, sf and sg all differ from 1) above 100 tol, in every instance."""
    ocp, pb, v0, res, z_l, z_u, options, c = _certified("ding2007", True, "gradient-based")
    lb, ub = ocp.bounds_vector()
    assert_certified(c, TOL)
    assert np.all(c["sf"] < 1) and np.all(c["sg"].min(1) < 1) and c["d"].min() < 1  # the mutations change something
    muts, i = _mutations(c, res.y, z_l, z_u, lb, ub, res.v)
    assert max(z_l[0, i], z_u[0, i]) * c["sf"][0] * c["d"][i] > 1e3 * TOL  # the dropped multiplier is an active one
    y, zl, zu = muts[mutation]
    bad = certificate(pb, lb, ub, res.v, y, zl, zu, v0, options)
    print(mutation, "scaled error", bad["scaled_error"])
    assert np.all(bad["scaled_error"] > 100 * TOL), bad["scaled_error"]
