"""Fatigue-parameter identification on the GPU: cfx_idf_forces / cfx_idf_normal against the exact-AD reference
(tests/fatigue_ident_reference.py), against cfx_integrate on the same handle, and the batched Levenberg-Marquardt
fits of ``FesFatigueIdentification``.

Shapes: ten pulses at 10 Hz over 1 s, N = 10, m in {1, 5}, truncation 10 (Ding) / 4 (Hmed), pulse width 0.0003,
intensity 50, B = 70 (a live tail wave), theta per instance within +-20 % of the model defaults (seeded).  Tolerance
1e-9 on errors scaled per instance by max |F| over the nodes (force) and by the column's max |S| over the nodes
(sensitivities): the project's figure for identification kernels against exact AD (tests/test_identification_gpu.py);
the reference's own noise (jacfwd against jacrev, tests/test_fatigue_identification_cpu.py) is <= 6.7e-14 on these
shapes.
"""

import functools

import numpy as np
import pytest

from tests import cases
from tests import fatigue_ident_reference as R

pytestmark = pytest.mark.gpu

TOL = 1e-9
B = 70
MODELS = {"ding2003_with_fatigue": (10, {}), "ding2007_with_fatigue": (10, {"pulse_width": 0.0003}),
          "hmed2018_with_fatigue": (4, {"pulse_intensity": 50})}
KEYS = R.FATIGUE_KEYS
SUBSET = ["tau_fat", "alpha_tau1"]  # two keys, not in slot order
GRID = [(n, s, m) for n in MODELS for s in ("RK1", "RK2", "RK4") for m in (1, 5)]


def _theta(st, keys, seed):
    return st.defaults(keys)[:, None] * (1 + 0.2 * np.random.default_rng(seed).uniform(-1, 1, (len(keys), B)))


@functools.lru_cache(maxsize=None)
def _reference(name, scheme, m, subset):
    """(setup, keys, theta, reference forces, reference sensitivities), computed once per case."""
    T, kw = MODELS[name]
    st = R.FatigueSetup(name, cases.TEN_PULSES, 1.0, 10, T, scheme, m, **kw)
    keys = SUBSET if subset else KEYS
    theta = _theta(st, keys, seed=11 + int(subset))
    F, S = st.forces_and_sens(keys, theta)
    for a in (theta, F, S):
        a.setflags(write=False)
    return st, keys, theta, F, S


def _handle(name, scheme, m, batch=B, layout="soa"):
    from cocofest_amd import IvpFes, ModelMaker, OdeSolver

    T, kw = MODELS.get(name, (10, {}))
    model = ModelMaker.create_model(name, stim_time=list(cases.TEN_PULSES), sum_stim_truncation=T)
    ivp = IvpFes({"model": model, **kw},
                 {"final_time": 1.0, "ode_solver": getattr(OdeSolver, scheme)(n_integration_steps=m)})
    u = ivp.controls.T.reshape(-1).copy()
    return ivp.handle(batch=batch, layout=layout), (u if u.size else None)


def _ids(keys):
    from cocofest_amd import _cfx

    return [_cfx.FATIGUE_PARAM_IDS[k] for k in keys]


@pytest.mark.parametrize("subset", [False, True], ids=["full", "subset"])
@pytest.mark.parametrize("name, scheme, m", GRID)
def test_forces_and_sensitivities_match_the_autodiff_reference(name, scheme, m, subset):
    st, keys, theta, F, S = _reference(name, scheme, m, subset)
    h, u = _handle(name, scheme, m)
    force, sens = h.idf_forces(_ids(keys), theta, u=u, n_data=1, with_sens=True)
    only, none = h.idf_forces(_ids(keys), theta, u=u, n_data=1)
    h.close()
    ef, es = R.scaled_errors(force, sens, F, S)
    print(f"{name} {scheme} x {m} {'subset' if subset else 'full'}: force {ef:.2e} sens {es.max():.2e}")
    assert np.all(np.abs(S).max(axis=(0, 2)) > 0)  # every column is a live one
    assert ef < TOL and np.all(es < TOL), (ef, es)
    assert none is None and only.tobytes() == force.tobytes()  # sens = NULL: the same force bits
    assert np.all(force[0] == 0.0) and np.all(sens[0] == 0.0)  # the rest state does not depend on theta


@pytest.mark.parametrize("name, scheme, m", GRID)
def test_forces_at_the_handles_constants_agree_with_cfx_integrate(name, scheme, m):
    """With theta = the handle's own fatigue constants (one key at a time, and all four), the node forces are the
    node samples of cfx_integrate on the same handle, to the tolerance and the scaling of tests/test_gpu_parity.py
    for kernels against the oracle."""
    from tests.test_gpu_parity import RTOL, _close

    T, kw = MODELS[name]
    st = R.FatigueSetup(name, cases.TEN_PULSES, 1.0, 10, T, scheme, m, **kw)
    h, u = _handle(name, scheme, m)
    traj = h.integrate(u=None if u is None else np.repeat(u[:, None], B, 1))
    ref = traj.reshape(10 * m + 1, 5, B)[::m, 1, :]
    for keys in (KEYS, ["alpha_km"]):
        force, _ = h.idf_forces(_ids(keys), np.repeat(st.defaults(keys)[:, None], B, 1), u=u, n_data=1)
        _close(force.T, ref.T, rtol=RTOL, what=f"{name} {scheme} x {m} {keys}")  # rows: one instance over the nodes
    h.close()
    assert RTOL == 1e-11 and np.all(np.isfinite(ref)) and np.all(ref[-1] != 0)


@pytest.mark.parametrize("name, scheme, m", GRID)
def test_normal_equations_equal_the_sums_over_the_trajectory(name, scheme, m):
    """cost, grad and gn against the same sums formed in float64 from cfx_idf_forces outputs; zero weights on a subset
    of the nodes; one shared experiment (n_data = 1) bit-identical to the same data replicated per instance."""
    T, kw = MODELS[name]
    st = R.FatigueSetup(name, cases.TEN_PULSES, 1.0, 10, T, scheme, m, **kw)
    rng = np.random.default_rng(23)
    for keys in (KEYS, SUBSET):
        n = len(keys)
        theta = _theta(st, keys, seed=29)
        h, u = _handle(name, scheme, m)
        force, sens = h.idf_forces(_ids(keys), theta, u=u, n_data=1, with_sens=True)
        y = force[:, 3] * (1 + 0.1 * rng.uniform(-1, 1, 11))
        w = rng.uniform(0.5, 2.0, 11)
        w[[0, 4, 9]] = 0.0
        cost, grad, gn = h.idf_normal(_ids(keys), theta, y, w, u=u, n_data=1)
        rep = lambda a: None if a is None else np.repeat(np.asarray(a)[:, None], B, 1)  # noqa: E731
        cost_b, grad_b, gn_b = h.idf_normal(_ids(keys), theta, rep(y), rep(w), u=rep(u), n_data=B)
        force_b, sens_b = h.idf_forces(_ids(keys), theta, u=rep(u), n_data=B if u is not None else 1, with_sens=True)
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
        assert force_b.tobytes() == force.tobytes() and sens_b.tobytes() == sens.tobytes()


def test_device_buffers_and_handle_checks():
    """CUDA tensors are used in place and give the host call's bits; n_data, NULL buffers and unsupported handle
    kinds are refused with their messages before anything is launched."""
    import ctypes as C

    import torch

    from cocofest_amd import CfxError, _cfx

    name = "ding2007_with_fatigue"
    st, keys, theta, F, S = _reference(name, "RK2", 1, False)
    h, u = _handle(name, "RK2", 1)
    force, sens = h.idf_forces(_ids(keys), theta, u=u, with_sens=True)
    y, w = F[:, 0].copy(), np.linspace(0.5, 1.5, 11)
    cost, grad, gn = h.idf_normal(_ids(keys), theta, y, w, u=u)
    dev = lambda a: torch.as_tensor(np.ascontiguousarray(a), device="cuda")  # noqa: E731
    f_d, s_d = h.idf_forces(_ids(keys), dev(theta), u=dev(u), with_sens=True)
    c_d, g_d, h_d = h.idf_normal(_ids(keys), dev(theta), dev(y), dev(w), u=dev(u))
    torch.cuda.synchronize()
    assert f_d.is_cuda and c_d.is_cuda
    assert f_d.cpu().numpy().tobytes() == force.tobytes() and s_d.cpu().numpy().tobytes() == sens.tobytes()
    assert c_d.cpu().numpy().tobytes() == cost.tobytes() and g_d.cpu().numpy().tobytes() == grad.tobytes()
    assert h_d.cpu().numpy().tobytes() == gn.tobytes()
    ids = np.asarray(_ids(keys), dtype=np.int32)
    idp = ids.ctypes.data_as(C.POINTER(C.c_int32))
    buf = np.zeros(11 * 4 * B)
    p = buf.ctypes.data

    def err(rc, code, msg):
        assert rc == code and msg in h.lib.cfx_last_error(h.h).decode(), h.lib.cfx_last_error(h.h).decode()

    lib = h.lib
    err(lib.cfx_idf_forces(h.h, 4, idp, p, p, 2, p, None, 0), _cfx.EINVAL, "n_data must be 1 or the batch size")
    err(lib.cfx_idf_forces(h.h, 4, idp, None, p, 1, p, None, 0), _cfx.EINVAL, "cfx_idf_forces: theta is NULL")
    err(lib.cfx_idf_forces(h.h, 4, idp, p, None, 1, p, None, 0), _cfx.EINVAL, "this model needs the controls u")
    err(lib.cfx_idf_forces(h.h, 4, idp, p, p, 1, None, None, 0), _cfx.EINVAL, "cfx_idf_forces: force is NULL")
    err(lib.cfx_idf_forces(h.h, 5, idp, p, p, 1, p, None, 0), _cfx.EINVAL, "cfx_idf_forces: n_id must be in [1, 4]")
    err(lib.cfx_idf_forces(h.h, 4, None, p, p, 1, p, None, 0), _cfx.EINVAL, "cfx_idf_forces: param_ids is NULL")
    err(lib.cfx_idf_normal(h.h, 4, idp, p, p, None, p, 1, p, p, p, 0), _cfx.EINVAL, "target or weight is NULL")
    err(lib.cfx_idf_normal(h.h, 4, idp, p, p, p, None, 1, p, p, p, 0), _cfx.EINVAL, "target or weight is NULL")
    err(lib.cfx_idf_normal(h.h, 4, idp, p, p, p, p, 1, p, None, p, 0), _cfx.EINVAL, "cost, grad or gn is NULL")
    err(lib.cfx_idf_normal(h.h, 4, idp, p, p, p, p, 3, p, p, p, 0), _cfx.EINVAL, "n_data must be 1 or the batch size")
    ids[1] = ids[0]
    err(lib.cfx_idf_normal(h.h, 4, idp, p, p, p, p, 1, p, p, p, 0), _cfx.EINVAL,
        "cfx_idf_normal: duplicate parameter id 0")
    ids[1] = 7
    err(lib.cfx_idf_forces(h.h, 4, idp, p, p, 1, p, None, 0), _cfx.EINVAL, "cfx_idf_forces: unknown parameter id 7")
    with pytest.raises(CfxError, match="n_data = 3"):
        h.idf_forces(_ids(keys), theta, u=u, n_data=3)
    with pytest.raises(CfxError, match="theta: 5 elements"):
        h.idf_forces(_ids(keys), np.zeros(5), u=u)
    h.close()
    # unsupported handle kinds
    hn, _ = _handle("ding2003", "RK4", 1, batch=64)
    with pytest.raises(CfxError, match="cfx_idf_forces: .*only available for the fatigue models") as exc:
        hn.idf_forces([0], np.ones((1, 64)))
    assert exc.value.code == _cfx.EUNSUPPORTED
    with pytest.raises(CfxError, match="cfx_idf_normal: .*only available for the fatigue models") as exc:
        hn.idf_normal([0], np.ones((1, 64)), np.zeros(11), np.ones(11))
    assert exc.value.code == _cfx.EUNSUPPORTED
    hn.close()
    ocp = cases.product_collocation_ocp("ding2003_with_fatigue", cases.TEN_PULSES, 1.0, 10)
    hc = ocp.nlp(batch=64, layout="soa")
    with pytest.raises(CfxError, match="not available for a collocation transcription") as exc:
        hc.idf_forces([0], np.ones((1, 64)))
    assert exc.value.code == _cfx.EUNSUPPORTED
    hc.close()
    ht = cases.product_ocp("ding2003_with_fatigue", cases.TEN_PULSES, 1.0, 10).nlp(batch=64, layout="tiled64")
    with pytest.raises(CfxError, match="not available with CFX_LAYOUT_TILED64") as exc:
        ht.idf_forces([0], np.ones((1, 64)))
    assert exc.value.code == _cfx.EUNSUPPORTED
    ht.close()


# ---- fits -------------------------------------------------------------------------------------------------
TRAIN_THEN_REST = [round(0.05 * i, 2) for i in range(10)]  # ten pulses at 20 Hz, then 0.5 s of rest; N = 20
RATES = ["alpha_a", "alpha_tau1", "alpha_km"]
FIT_CTL = {"ding2003_with_fatigue": {}, "ding2007_with_fatigue": {"pulse_width": {"fixed": 0.0003}},
           "hmed2018_with_fatigue": {"pulse_intensity": {"fixed": 50}}}
# Largest relative error of a recovered rate over the 64 starts of the CPU reference LM (tests/ident_reference.py's
# lm_reference on the exact-AD normal equations of the same problem, same starts), per model; the GPU fit is held to
# 100 x that.
# Those runs: every start stopped on the gradient test; Ding2003 <= 4 iterations, cost <= 5.8e-15; Ding2007 <= 5,
# cost <= 1.2e-11; Hmed2018 <= 5, cost <= 3.7e-13.
CPU_RATE_ERROR = {"ding2003_with_fatigue": 9.936e-7, "ding2007_with_fatigue": 1.625e-3, "hmed2018_with_fatigue": 4.422e-5}


def _generated_curve(name, **fes):
    """Noise-free node forces of the product's own IvpFes at the model's default constants (RK4 x 5)."""
    from cocofest_amd import IvpFes, ModelMaker, OdeSolver

    model = ModelMaker.create_model(name, stim_time=list(TRAIN_THEN_REST), sum_stim_truncation=10)
    ivp = IvpFes({"model": model, **fes}, {"final_time": 1.0, "ode_solver": OdeSolver.RK4(n_integration_steps=5)})
    out = ivp.integrate(return_time=False)["F"][0][::5]
    ivp.close()
    return [float(v) for v in out]


def _fit(name, keys):
    """64 seeded starts around an initial guess that is NOT the generating point: every generating value times 1.15
    (even positions in ``keys``) or 0.87 (odd); start 0 is that guess, the others log-uniform within exp(0.5) of it.
    So no start begins at the solution, and the truth is recovered only if the solver works."""
    from cocofest_amd import FesFatigueIdentification, ModelMaker, OdeSolver

    ctl = FIT_CTL[name]
    fes = {k: v["fixed"] for k, v in ctl.items()}
    model = ModelMaker.create_model(name, stim_time=list(TRAIN_THEN_REST), sum_stim_truncation=10)
    true = dict(model.identifiable_parameters)
    guess = {k: true[k] * (1.15 if j % 2 == 0 else 0.87) for j, k in enumerate(keys)}
    ident = FesFatigueIdentification(model, final_time=1.0, force_tracking=_generated_curve(name, **fes),
                                     key_parameter_to_identify=keys, ode_solver=OdeSolver.RK4(n_integration_steps=5),
                                     initial_guess=guess, n_starts=64, seed=0, start_spread=0.5, **ctl)
    assert ident.n_shooting == 20
    theta0 = ident.starts()
    off = np.abs(theta0 / np.array([true[k] for k in keys])[:, None] - 1)
    assert np.all(off.max(axis=0) > 0.05)  # every start is off the generating point by more than 5 % somewhere
    res = ident.solve()
    ident.close()
    return true, res


def _assert_monotone_progress(res):
    """Every start made progress, no accepted iteration raised its cost, and the bookkeeping is consistent."""
    s = res["starts"]
    print("status", np.bincount(s["status"], minlength=4), "iterations max", s["iterations"].max(),
          "cost max %.3e" % s["cost"].max(), "cost / cost0 max %.3e" % (s["cost"] / s["cost_history"][0]).max())
    assert np.all(np.isfinite(s["cost"]))
    assert np.all(s["iterations"] >= 1) and np.all(s["cost"] < 1e-3 * s["cost_history"][0])
    assert np.all(np.diff(s["cost_history"], axis=0) <= 0.0)
    assert np.all(s["cost_history"][-1] == s["cost"])
    assert res["cost"] == s["cost"].min()


@pytest.mark.parametrize("name", list(MODELS))
def test_fit_recovers_the_three_rates_from_every_start(name):
    """alpha_a, alpha_tau1, alpha_km with tau_fat fixed at the generating value: well posed.  Every start stops on
    the projected-gradient test, the cost never rises, and every start (and the best one) recovers the generating
    rates to 100 x the CPU reference LM's largest error on this model (CPU_RATE_ERROR)."""
    from cocofest_amd.identification import CONVERGED_GRADIENT

    true, res = _fit(name, RATES)
    _assert_monotone_progress(res)
    s = res["starts"]
    assert np.all(s["status"] == CONVERGED_GRADIENT), s["status"]
    rel = np.abs(s["theta"] / np.array([true[k] for k in RATES]) - 1)
    print(f"{name}: largest relative rate error {rel.max():.3e}")
    assert rel.max() <= 100 * CPU_RATE_ERROR[name], rel.max(axis=0)
    for k in RATES:
        assert abs(res[k] / true[k] - 1) <= 100 * CPU_RATE_ERROR[name]
    assert res["tau_fat"] == true["tau_fat"]  # not identified: the model's value


@pytest.mark.parametrize("name", list(MODELS))
def test_fit_of_all_four_parameters_makes_monotone_progress(name):
    """tau_fat (127 s) is not identifiable from 1 s of data: in the CPU reference runs it went to a bound and the
    three rates absorbed the difference (within 0.4 %), so no recovery is asserted.  No start may end NOT_CONVERGED
    or with a non-finite cost, every start makes progress and the cost never rises."""
    from cocofest_amd.identification import NOT_CONVERGED

    _, res = _fit(name, KEYS)
    _assert_monotone_progress(res)
    assert np.all(res["starts"]["status"] != NOT_CONVERGED), res["starts"]["status"]
