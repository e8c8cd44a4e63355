"""Force-parameter identification on the GPU: cfx_id_forces / cfx_id_normal against the exact-AD reference
(tests/ident_reference.py) and the batched Levenberg-Marquardt fits of ``FesIdentification``.

Shapes: ten pulses at 10 Hz over 1 s, N = 10, m in {1, 5}, truncation 10 (Ding) / 4 (Hmed), B = 70 (a live tail
wave), theta per instance within +-20 % of the model defaults (seeded).  Tolerance 1e-9 on errors scaled per
instance by max |F| over the nodes (force) and by the column's max |S| over the nodes (sensitivities): the
project's figure for kernel against exact-AD parity; the reference's own noise (jacfwd against jacrev,
tests/test_identification_cpu.py) is below 4e-15 on these shapes.
"""

import functools

import numpy as np
import pytest

from tests import cases
from tests import ident_reference as R

pytestmark = pytest.mark.gpu

TOL = 1e-9
B = 70
MODELS = {"ding2003": (10, {}), "ding2007": (10, {"pulse_width": 0.0003}), "hmed2018": (4, {"pulse_intensity": 50})}
SUBSET = {"ding2003": ["tau2", "a_rest"], "ding2007": ["km_rest", "a_scale"], "hmed2018": ["tau1_rest", "km_rest"]}
GRID = [(n, s, m) for n in MODELS for s in ("RK1", "RK2", "RK4") for m in (1, 5)]


def _theta(st, keys, seed):
    return st.defaults(keys)[:, None] * (1 + 0.2 * np.random.default_rng(seed).uniform(-1, 1, (len(keys), B)))


@functools.lru_cache(maxsize=None)
def _reference(name, scheme, m, subset):
    """(setup, keys, theta, reference forces, reference sensitivities), computed once per case."""
    T, kw = MODELS[name]
    st = R.Setup(name, cases.TEN_PULSES, 1.0, 10, T, scheme, m, **kw)
    keys = SUBSET[name] if subset else R.FULL_KEYS[name]
    theta = _theta(st, keys, seed=11 + int(subset))
    F, S = st.forces_and_sens(keys, theta)
    for a in (theta, F, S):
        a.setflags(write=False)
    return st, keys, theta, F, S


def _handle(name, scheme, m, batch=B, layout="soa"):
    from cocofest_amd import IvpFes, ModelMaker, OdeSolver

    T, kw = MODELS[name]
    model = ModelMaker.create_model(name, stim_time=list(cases.TEN_PULSES), sum_stim_truncation=T)
    ivp = IvpFes({"model": model, **kw},
                 {"final_time": 1.0, "ode_solver": getattr(OdeSolver, scheme)(n_integration_steps=m)})
    u = ivp.controls.T.reshape(-1).copy()
    return ivp.handle(batch=batch, layout=layout), (u if u.size else None)


def _ids(keys):
    from cocofest_amd import _cfx

    return [_cfx.PARAM_IDS[k] for k in keys]


@pytest.mark.parametrize("subset", [False, True], ids=["full", "subset"])
@pytest.mark.parametrize("name, scheme, m", GRID)
def test_forces_and_sensitivities_match_the_autodiff_reference(name, scheme, m, subset):
    st, keys, theta, F, S = _reference(name, scheme, m, subset)
    h, u = _handle(name, scheme, m)
    force, sens = h.id_forces(_ids(keys), theta, u=u, n_data=1, with_sens=True)
    only, none = h.id_forces(_ids(keys), theta, u=u, n_data=1)
    h.close()
    ef, es = R.scaled_errors(force, sens, F, S)
    print(f"{name} {scheme} x {m} {'subset' if subset else 'full'}: force {ef:.2e} sens {es.max():.2e}")
    assert ef < TOL and np.all(es < TOL), (ef, es)
    assert none is None and only.tobytes() == force.tobytes()  # sens = NULL: the same force bits
    assert np.all(force[0] == 0.0) and np.all(sens[0] == 0.0)  # the rest state does not depend on theta


@pytest.mark.parametrize("name, scheme, m", GRID)
def test_normal_equations_equal_the_sums_over_the_trajectory(name, scheme, m):
    """cost, grad and gn against the same sums formed in float64 from cfx_id_forces outputs; zero weights on a subset
    of the nodes; one shared experiment (n_data = 1) bit-identical to the same data replicated per instance."""
    T, kw = MODELS[name]
    st = R.Setup(name, cases.TEN_PULSES, 1.0, 10, T, scheme, m, **kw)
    rng = np.random.default_rng(23)
    for keys in (R.FULL_KEYS[name], SUBSET[name]):
        n = len(keys)
        theta = _theta(st, keys, seed=29)
        h, u = _handle(name, scheme, m)
        force, sens = h.id_forces(_ids(keys), theta, u=u, n_data=1, with_sens=True)
        y = force[:, 3] * (1 + 0.1 * rng.uniform(-1, 1, 11))
        w = rng.uniform(0.5, 2.0, 11)
        w[[0, 4, 9]] = 0.0
        cost, grad, gn = h.id_normal(_ids(keys), theta, y, w, u=u, n_data=1)
        rep = lambda a: None if a is None else np.repeat(np.asarray(a)[:, None], B, 1)  # noqa: E731
        cost_b, grad_b, gn_b = h.id_normal(_ids(keys), theta, rep(y), rep(w), u=rep(u), n_data=B)
        h.close()
        r = force - y[:, None]
        dt = 1.0 / 10
        ref_c = dt * np.sum(w[:, None] * r * r, axis=0)
        ref_g = 2 * dt * np.einsum("k,kb,kjb->jb", w, r, sens)
        full = 2 * dt * np.einsum("k,kib,kjb->ijb", w, sens, sens)
        ref_h = np.stack([full[i, j] for i in range(n) for j in range(i + 1)])
        # scales: the sums of the absolute summands (a gradient entry is a cancelling sum over the nodes)
        sc_g = 2 * dt * np.einsum("k,kb,kjb->jb", w, np.abs(r), np.abs(sens))
        sc_h = np.sqrt(np.stack([full[i, i] * full[j, j] for i in range(n) for j in range(i + 1)]))
        assert np.max(np.abs(cost - ref_c) / ref_c) < TOL
        assert np.max(np.abs(grad - ref_g) / sc_g) < TOL
        assert np.max(np.abs(gn - ref_h) / sc_h) < TOL
        assert cost_b.tobytes() == cost.tobytes() and grad_b.tobytes() == grad.tobytes()
        assert gn_b.tobytes() == gn.tobytes()


def test_device_buffers_and_handle_checks():
    """CUDA tensors are used in place and give the host call's bits; n_data, NULL buffers and unsupported handle
    kinds are refused with their messages before anything is launched."""
    import ctypes as C

    import torch

    from cocofest_amd import CfxError, _cfx

    st, keys, theta, F, S = _reference("ding2007", "RK2", 1, False)
    h, u = _handle("ding2007", "RK2", 1)
    force, sens = h.id_forces(_ids(keys), theta, u=u, with_sens=True)
    dev = lambda a: torch.as_tensor(np.ascontiguousarray(a), device="cuda")  # noqa: E731
    f_d, s_d = h.id_forces(_ids(keys), dev(theta), u=dev(u), with_sens=True)
    torch.cuda.synchronize()
    assert f_d.cpu().numpy().tobytes() == force.tobytes() and s_d.cpu().numpy().tobytes() == sens.tobytes()
    ids = np.asarray(_ids(keys), dtype=np.int32)
    idp = ids.ctypes.data_as(C.POINTER(C.c_int32))
    buf = np.zeros(11 * 6 * B)
    p = buf.ctypes.data

    def err(rc, code, msg):
        assert rc == code and msg in h.lib.cfx_last_error(h.h).decode(), h.lib.cfx_last_error(h.h).decode()

    lib = h.lib
    err(lib.cfx_id_forces(h.h, 6, idp, p, p, 2, p, None, 0), _cfx.EINVAL, "n_data must be 1 or the batch size")
    err(lib.cfx_id_forces(h.h, 6, idp, None, p, 1, p, None, 0), _cfx.EINVAL, "cfx_id_forces: theta is NULL")
    err(lib.cfx_id_forces(h.h, 6, idp, p, None, 1, p, None, 0), _cfx.EINVAL, "this model needs the controls u")
    err(lib.cfx_id_forces(h.h, 6, idp, p, p, 1, None, None, 0), _cfx.EINVAL, "cfx_id_forces: force is NULL")
    err(lib.cfx_id_forces(h.h, 9, idp, p, p, 1, p, None, 0), _cfx.EINVAL, "cfx_id_forces: n_id must be in [1, 8]")
    err(lib.cfx_id_normal(h.h, 6, idp, p, p, None, p, 1, p, p, p, 0), _cfx.EINVAL, "target or weight is NULL")
    err(lib.cfx_id_normal(h.h, 6, idp, p, p, p, p, 1, p, None, p, 0), _cfx.EINVAL, "cost, grad or gn is NULL")
    ids[1] = ids[0]
    err(lib.cfx_id_normal(h.h, 6, idp, p, p, p, p, 1, p, p, p, 0), _cfx.EINVAL, "cfx_id_normal: duplicate parameter")
    with pytest.raises(CfxError, match="n_data = 3"):
        h.id_forces(_ids(keys), theta, u=u, n_data=3)
    with pytest.raises(CfxError, match="theta: 5 elements"):
        h.id_forces(_ids(keys), np.zeros(5), u=u)
    h.close()
    # unsupported handle kinds
    ocp = cases.product_collocation_ocp("ding2003", cases.TEN_PULSES, 1.0, 10)
    hc = ocp.nlp(batch=64, layout="soa")
    with pytest.raises(CfxError, match="not available for a collocation transcription") as exc:
        hc.id_forces([0], np.ones((1, 64)))
    assert exc.value.code == _cfx.EUNSUPPORTED
    hc.close()
    ht = cases.product_ocp("ding2003", cases.TEN_PULSES, 1.0, 10).nlp(batch=64, layout="tiled64")
    with pytest.raises(CfxError, match="not available with CFX_LAYOUT_TILED64") as exc:
        ht.id_forces([0], np.ones((1, 64)))
    assert exc.value.code == _cfx.EUNSUPPORTED
    ht.close()
    hf = cases.product_ocp("ding2003_with_fatigue", cases.TEN_PULSES, 1.0, 10).nlp(batch=64, layout="soa")
    with pytest.raises(CfxError, match="not available for the fatigue models") as exc:
        hf.id_forces([0], np.ones((1, 64)))
    assert exc.value.code == _cfx.EUNSUPPORTED
    hf.close()


# ---- fits -------------------------------------------------------------------------------------------------
TRAIN_THEN_REST = [round(0.05 * i, 2) for i in range(10)]  # ten pulses at 20 Hz, then 0.5 s of rest; N = 20
FIT_SPREAD = 0.5


def _generated_curve(name, **fes):
    """Noise-free node forces of the product's own IvpFes at the model's default constants (RK4 x 5)."""
    from cocofest_amd import IvpFes, ModelMaker, OdeSolver

    model = ModelMaker.create_model(name, stim_time=list(TRAIN_THEN_REST), sum_stim_truncation=10)
    ivp = IvpFes({"model": model, **fes}, {"final_time": 1.0, "ode_solver": OdeSolver.RK4(n_integration_steps=5)})
    out = ivp.integrate(return_time=False)["F"][0][::5]
    ivp.close()
    return [float(v) for v in out]


def _fit(name, keys, spread=FIT_SPREAD, **ctl):
    """64 seeded starts around an initial guess that is NOT the generating point: every generating value times 1.15
    (even positions in ``keys``) or 0.87 (odd); start 0 is that guess, the others log-uniform within exp(spread)
    of it.  So no start begins at the solution, and the truth is recovered only if the solver works."""
    from cocofest_amd import FesIdentification, ModelMaker, OdeSolver

    fes = {k: v["fixed"] for k, v in ctl.items()}
    model = ModelMaker.create_model(name, stim_time=list(TRAIN_THEN_REST), sum_stim_truncation=10)
    true = dict(model.identifiable_parameters)
    guess = {k: true[k] * (1.15 if j % 2 == 0 else 0.87) for j, k in enumerate(keys)}
    ident = FesIdentification(model, final_time=1.0, force_tracking=_generated_curve(name, **fes),
                              key_parameter_to_identify=keys, ode_solver=OdeSolver.RK4(n_integration_steps=5),
                              initial_guess=guess, n_starts=64, seed=0, start_spread=spread, **ctl)
    assert ident.n_shooting == 20
    theta0 = ident.starts()
    off = np.abs(theta0 / np.array([true[k] for k in keys])[:, None] - 1)
    assert np.all(off.max(axis=0) > 0.05)  # every start is off the generating point by more than 5 % somewhere
    res = ident.solve()
    ident.close()
    return true, res


def _assert_converged_and_monotone(res):
    """Every start stops on the projected-gradient test (status 1): a step-size stop after an accepted step (2) did
    not occur in the CPU runs of these fits, and a stalled start (3) or one out of iterations (0) is a failure.
    Every start made progress, and no accepted iteration raised its cost."""
    from cocofest_amd.identification import CONVERGED_GRADIENT

    s = res["starts"]
    print("status", np.bincount(s["status"], minlength=4), "iterations max", s["iterations"].max(),
          "cost max %.3e" % s["cost"].max())
    assert np.all(s["status"] == CONVERGED_GRADIENT), s["status"]
    assert np.all(s["iterations"] >= 1) and np.all(s["cost"] < 1e-3 * s["cost_history"][0])
    assert np.all(np.diff(s["cost_history"], axis=0) <= 0.0)
    assert np.all(s["cost_history"][-1] == s["cost"])
    assert res["cost"] == s["cost"].min()


def _assert_every_start_recovers(res, true, keys):
    """The reference's tolerances (test_ocp_id.py:212-215), for EVERY start: the first key (a_rest) to 0 decimals,
    the others to 3 decimals."""
    theta = res["starts"]["theta"]
    for b in range(theta.shape[0]):
        np.testing.assert_almost_equal(theta[b, 0], true[keys[0]], decimal=0, err_msg=f"start {b}")
        np.testing.assert_almost_equal(theta[b, 1:], [true[k] for k in keys[1:]], decimal=3, err_msg=f"start {b}")
    np.testing.assert_almost_equal(res[keys[0]], true[keys[0]], decimal=0)
    for k in keys[1:]:
        np.testing.assert_almost_equal(res[k], true[k], decimal=3)


def test_ding2003_fit_recovers_the_generating_constants_from_every_start():
    """64 seeded starts log-uniform within a factor exp(0.5) = 1.65 of a guess 13-15 % off the generating values.
    The spread was chosen on the CPU: with it the reference LM of tests/ident_reference.py (same update rule,
    exact-AD normal equations) converges on the gradient test from every one of these 64 starts, in <= 10
    iterations, to |a_rest error| <= 1.9e-3 and the other errors <= 2.7e-7.  Here every start must converge and
    reproduce the constants to the reference's tolerances, and so must the best one."""
    keys = ["a_rest", "km_rest", "tau1_rest", "tau2"]
    true, res = _fit("ding2003", keys)
    _assert_converged_and_monotone(res)
    _assert_every_start_recovers(res, true, keys)


def test_ding2007_fit_converges_with_monotone_cost():
    """All six parameters.  The pulse width differs from pulse to pulse: with one width a_scale, pd0 and pdt enter
    only through the product a_scale E(pw; pd0, pdt) and cannot be told apart.  Spread 0.2 (a factor 1.22) around
    the perturbed guess: the CPU reference LM converges on the gradient test from all 64 of these starts (tau2 =
    0.001 s is barely visible in the curve and ends at its lower bound from some starts, hence no parameter
    assertion: convergence, progress and monotone cost only)."""
    _, res = _fit("ding2007", ["a_scale", "km_rest", "tau1_rest", "tau2", "pd0", "pdt"], spread=0.2,
                  pulse_width={"fixed": [0.0002 + 0.00004 * i for i in range(10)]})
    _assert_converged_and_monotone(res)


def test_hmed2018_fit_converges_with_monotone_cost():
    """The four force parameters under pulse-to-pulse intensities; spread 0.2 around the perturbed guess: the CPU
    reference LM converges from all 64 of these starts in <= 6 iterations, errors <= 2.6e-4 (a_rest) and 1.1e-8."""
    keys = ["a_rest", "km_rest", "tau1_rest", "tau2"]
    true, res = _fit("hmed2018", keys, spread=0.2, pulse_intensity={"fixed": [30.0 + 7 * i for i in range(10)]})
    _assert_converged_and_monotone(res)
    _assert_every_start_recovers(res, true, keys)
