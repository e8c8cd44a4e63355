"""Multi-train fatigue-parameter identification on the GPU: cfx_idfm_forces / cfx_idfm_normal against exact autodiff
(tests/multitrain_fatigue_ident_reference.py), against cfx_idf_forces on a cfx_create handle (E = 1) and against
cfx_sweep_integrate (the model's own constants).

The mixed trains (``MF.MIXED``): E = 3 with N = 10 / 13 / 8 (the NaN fill), final_time 1 / 1.3 / 0.4, truncation 3 /
20 (more than the train's 8 pulses) / 1, a doublet train, a first pulse after t = 0, per-pulse widths and intensities;
B = 70 (one full wave and a 6-lane tail per train); n_steps in {1, 5}; theta within +-20 % of the defaults.  Tolerance
1e-9 on errors scaled per instance by max |F| over the nodes (force) and by the column's max |S| (sensitivities), as
tests/test_multitrain_ident_gpu.py; 1e-11 for the two parities, as tests/test_gpu_parity.py.  The reference's own
noise (jacfwd against jacrev) on these shapes is 2e-15 (tests/test_multitrain_fatigue_ident_cpu.py prints it).
"""

import ctypes as C

import numpy as np
import pytest

from tests import multitrain_fatigue_ident_reference as MF
from tests import sweep_reference as SR
from tests.test_multitrain_ident_gpu import _float64_sums

pytestmark = pytest.mark.gpu

TOL = 1e-9
PARITY_TOL = 1e-11
B = 70
GRID = [(n, s, m) for n in MF.MODELS for s in MF.SCHEMES for m in (1, 5)]
SCHEME_ID = {"RK1": 1, "RK2": 2, "RK4": 4}


def _ids(keys):
    from cocofest_amd import _cfx

    return [_cfx.FATIGUE_PARAM_IDS[k] for k in keys]


def _idfm(name, scheme, m, cases, batch=B, targets=None, weights=None):
    """(cfx_idfm object, packed trains) of the cases in the order given."""
    from cocofest_amd import _cfx
    from oracle import fes_oracle as O

    trains, P, Nmax = MF.pack(name, cases, targets, weights)
    c = dict(O.model_constants(name), fl=1.0, fv=1.0, fp=0.0)
    idfm = _cfx.Idfm(model_id=_cfx.MODEL_IDS[name], constants=c, scheme=SCHEME_ID[scheme], n_steps=m, batch=batch,
                     n_trains=len(cases), max_pulses=P, max_shooting=Nmax)
    return idfm, trains


@pytest.mark.parametrize("subset", [False, True], ids=["full", "subset"])
@pytest.mark.parametrize("name, scheme, m", GRID)
def test_forces_and_sensitivities_match_the_autodiff_reference(name, scheme, m, subset):
    """Largest measured on MI355X over the grid: see DESIGN section 7e."""
    keys, theta, Fs, Ss = MF.reference(name, scheme, m, subset)
    idfm, trains = _idfm(name, scheme, m, MF.MIXED)
    force, sens = idfm.forces(trains, _ids(keys), theta, with_sens=True)
    only, none = idfm.forces(trains, _ids(keys), theta)
    idfm.close()
    assert none is None and only.tobytes() == force.tobytes()  # sens = NULL: the same force bits
    worst_f, worst_s = 0.0, 0.0
    for e, case in enumerate(MF.MIXED):
        N = case["n_shooting"]
        assert np.all(np.isnan(force[e, N + 1:])) and np.all(np.isnan(sens[e, N + 1:]))
        assert np.all(force[e, 0] == 0.0) and np.all(sens[e, 0] == 0.0)  # the rest state
        assert np.all(np.isfinite(force[e, : N + 1])) and np.all(np.isfinite(sens[e, : N + 1]))
        assert np.all(np.max(np.abs(sens[e, : N + 1]), axis=0) > 0.0)  # every sensitivity column is nonzero
        ef, es = MF.scaled_errors(force[e, : N + 1], sens[e, : N + 1], Fs[e], Ss[e])
        worst_f, worst_s = max(worst_f, ef), max(worst_s, float(es.max()))
    print(f"idfm parity {name} {scheme} x {m} {'subset' if subset else 'full'}: force {worst_f:.2e} "
          f"sens {worst_s:.2e}")
    assert worst_f < TOL and worst_s < TOL, (worst_f, worst_s)


@pytest.mark.parametrize("name, scheme, m", [(n, s, m) for n in MF.MODELS for s, m in (("RK1", 1), ("RK2", 5),
                                                                                         ("RK4", 5))])
def test_single_train_agrees_with_cfx_idf_forces(name, scheme, m):
    """E = 1, truncation 3 (within the handle tables' reach): cfx_idf_forces on the equivalent cfx_create handle.  The
    bits differ (the handle's forcing comes from host tables, this one is folded on the device)."""
    case = MF.MIXED[0]
    for keys in (MF.FATIGUE_KEYS, MF.SUBSET):
        theta = MF.theta_of(name, keys, B, seed=31)
        ivp = SR.make_ivp(name, case, scheme, m)
        h = ivp.handle(batch=B, layout="soa")
        u = ivp.controls.T.reshape(-1).copy()
        F, S = h.idf_forces(_ids(keys), theta, u=u if u.size else None, with_sens=True)
        h.close()
        idfm, trains = _idfm(name, scheme, m, [case])
        force, sens = idfm.forces(trains, _ids(keys), theta, with_sens=True)
        idfm.close()
        ef, es = MF.scaled_errors(force[0], sens[0], F, S)
        print(f"idfm E = 1 against cfx_idf_forces {name} {scheme} x {m}: force {ef:.2e} sens {es.max():.2e}")
        assert ef < PARITY_TOL and es.max() < PARITY_TOL


@pytest.mark.parametrize("name, scheme, m", GRID)
def test_forces_at_the_model_constants_agree_with_the_sweep(name, scheme, m):
    """The F node states of cfx_sweep_integrate on the same trains."""
    from cocofest_amd import IvpSweep
    from oracle import fes_oracle as O

    c = O.model_constants(name)
    ivps = [SR.make_ivp(name, case, scheme, m) for case in MF.MIXED]
    sweep = IvpSweep(ivps)
    ref = sweep.integrate(nodes=True)["F"]  # (E, Nmax + 1)
    sweep.close()
    theta = np.repeat(np.array([[c[k]] for k in MF.FATIGUE_KEYS], dtype=float), B, axis=1)
    idfm, trains = _idfm(name, scheme, m, MF.MIXED)
    force, _ = idfm.forces(trains, _ids(MF.FATIGUE_KEYS), theta)
    idfm.close()
    worst = 0.0
    for e, case in enumerate(MF.MIXED):
        N = case["n_shooting"]
        assert np.all(force[e, : N + 1] == force[e, : N + 1, :1])  # the same theta: the same bits in every lane
        worst = max(worst, float(np.max(np.abs(force[e, : N + 1, 0] - ref[e, : N + 1])) / np.max(np.abs(ref[e, : N + 1]))))
    print(f"idfm against the sweep {name} {scheme} x {m}: {worst:.2e}")
    assert worst < PARITY_TOL


@pytest.mark.parametrize("name, scheme, m", [(n, s, m) for n in MF.MODELS for s, m in (("RK1", 1), ("RK2", 5),
                                                                                         ("RK4", 5))])
def test_normal_equations_equal_the_sums_over_the_trains(name, scheme, m):
    rng = np.random.default_rng(23)
    for keys in (MF.FATIGUE_KEYS, MF.SUBSET):
        theta = MF.theta_of(name, keys, B, seed=29)
        idfm, trains = _idfm(name, scheme, m, MF.MIXED)
        force, sens = idfm.forces(trains, _ids(keys), theta, with_sens=True)
        idfm.close()
        y, w = [], []
        for e, case in enumerate(MF.MIXED):
            N = case["n_shooting"]
            y.append(force[e, : N + 1, 3] * (1 + 0.1 * rng.uniform(-1, 1, N + 1)))
            w.append(rng.uniform(0.5, 2.0, N + 1))
            w[-1][[0, 2, N]] = 0.0
        idfm, trains = _idfm(name, scheme, m, MF.MIXED, targets=y, weights=w)  # NaN past every train's N
        cost, grad, gn, cpt = idfm.normal(trains, _ids(keys), theta, per_train=True)
        cost2, grad2, gn2, none = idfm.normal(trains, _ids(keys), theta)
        idfm.close()
        ref_c, ref_g, ref_h, sc_g, sc_h, ref_cpt = _float64_sums(force, sens, MF.MIXED, y, w)
        assert np.all(np.isfinite(cost)) and np.all(np.isfinite(grad)) and np.all(np.isfinite(gn))
        assert np.max(np.abs(cost - ref_c) / ref_c) < TOL
        assert np.max(np.abs(grad - ref_g) / sc_g) < TOL
        assert np.max(np.abs(gn - ref_h) / sc_h) < TOL
        assert np.max(np.abs(cpt - ref_cpt) / ref_cpt) < TOL
        assert np.max(np.abs(cpt.sum(axis=0) - cost) / cost) < 1e-12
        acc = cpt[0].copy()
        for e in range(1, len(MF.MIXED)):
            acc = acc + cpt[e]
        assert np.array_equal(acc, cost)  # the sum over the trains, in train order
        assert none is None and cost2.tobytes() == cost.tobytes() and grad2.tobytes() == grad.tobytes()
        assert gn2.tobytes() == gn.tobytes()


@pytest.mark.parametrize("name", MF.MODELS)
def test_position_independence(name):
    """A start alone, in the batch and in the reversed batch, and the trains in another order: identical bits."""
    keys = MF.FATIGUE_KEYS
    theta = MF.theta_of(name, keys, B, seed=37)
    idfm, trains = _idfm(name, "RK4", 5, MF.MIXED)
    force, sens = idfm.forces(trains, _ids(keys), theta, with_sens=True)
    perm = np.random.default_rng(3).permutation(B)
    rf, rs = idfm.forces(trains, _ids(keys), np.ascontiguousarray(theta[:, perm]), with_sens=True)
    idfm.close()
    assert np.array_equal(rf, force[:, :, perm], equal_nan=True) and np.array_equal(rs, sens[..., perm], equal_nan=True)
    one, trains1 = _idfm(name, "RK4", 5, MF.MIXED, batch=1)
    for b in (0, 63, 64, 69):
        f1, s1 = one.forces(trains1, _ids(keys), np.ascontiguousarray(theta[:, b: b + 1]), with_sens=True)
        assert np.array_equal(f1[:, :, 0], force[:, :, b], equal_nan=True)
        assert np.array_equal(s1[..., 0], sens[..., b], equal_nan=True)
    one.close()
    order = [2, 0, 1]
    idfm, trains = _idfm(name, "RK4", 5, [MF.MIXED[i] for i in order])
    pf, ps = idfm.forces(trains, _ids(keys), theta, with_sens=True)
    idfm.close()
    for j, i in enumerate(order):
        N = MF.MIXED[i]["n_shooting"]
        assert np.array_equal(pf[j, : N + 1], force[i, : N + 1]) and np.array_equal(ps[j, : N + 1], sens[i, : N + 1])


def test_device_buffers_give_the_host_bits():
    import torch

    name = "hmed2018_with_fatigue"
    keys = MF.FATIGUE_KEYS
    theta = MF.theta_of(name, keys, B, seed=43)
    y = [np.linspace(0, 50, c["n_shooting"] + 1) for c in MF.MIXED]
    w = [np.ones(c["n_shooting"] + 1) for c in MF.MIXED]
    idfm, trains = _idfm(name, "RK4", 5, MF.MIXED, targets=y, weights=w)
    force, sens = idfm.forces(trains, _ids(keys), theta, with_sens=True)
    host = idfm.normal(trains, _ids(keys), theta, per_train=True)
    dev = {k: (None if v is None else torch.as_tensor(v).cuda()) for k, v in trains.items()}
    dth = torch.as_tensor(theta).cuda()
    dforce, dsens = idfm.forces(dev, _ids(keys), dth, with_sens=True)
    dnorm = idfm.normal(dev, _ids(keys), dth, per_train=True)
    torch.cuda.synchronize()
    idfm.close()
    assert np.array_equal(dforce.cpu().numpy(), force, equal_nan=True)
    assert np.array_equal(dsens.cpu().numpy(), sens, equal_nan=True)
    for a, b in zip(dnorm, host):
        assert np.array_equal(a.cpu().numpy(), b)


def test_invalid_arguments_launch_nothing():
    from cocofest_amd import CfxError, _cfx
    from oracle import fes_oracle as O

    name = "ding2007_with_fatigue"
    keys = MF.FATIGUE_KEYS
    theta = MF.theta_of(name, keys, B, seed=47)
    y = [np.zeros(c["n_shooting"] + 1) for c in MF.MIXED]
    w = [np.ones(c["n_shooting"] + 1) for c in MF.MIXED]
    idfm, trains = _idfm(name, "RK2", 1, MF.MIXED, targets=y, weights=w)
    good, _ = idfm.forces(trains, _ids(keys), theta)
    ids = np.asarray(_ids(keys), dtype=np.int32)
    idp = ids.ctypes.data_as(C.POINTER(C.c_int32))
    E = len(MF.MIXED)
    for key, idx, value, message in (("times", (2, 0), -1.0, "train 0: pulse 2: time decreases"),
                                     ("act_node", (0, 2), 9, "train 2: pulse 0: activation node past n_shooting"),
                                     ("truncation", 1, 0, "train 1: truncation must be >= 1"),
                                     ("weight", (3, 1), -2.0, "train 1: node 3: weight must be finite")):
        bad = {k: (None if v is None else v.copy()) for k, v in trains.items()}
        bad[key][idx] = value
        st, keep = _cfx._idm_trains(bad, E, idfm.max_pulses, idfm.max_shooting, True)
        out = np.full((E, idfm.max_shooting + 1, B), -7.0)
        small = np.full((1 + 4 + 10, B), -7.0)
        if key != "weight":  # the forces call does not read the weights
            rc = idfm.lib.cfx_idfm_forces(idfm.h, C.byref(st), 4, idp, theta.ctypes.data, out.ctypes.data, None, 0,
                                          None)
            assert rc == _cfx.EINVAL and message in idfm.lib.cfx_idfm_last_error(idfm.h).decode()
        rc = idfm.lib.cfx_idfm_normal(idfm.h, C.byref(st), 4, idp, theta.ctypes.data, small[0:1].ctypes.data,
                                      small[1:5].ctypes.data, small[5:].ctypes.data, None, 0, None)
        assert rc == _cfx.EINVAL and message in idfm.lib.cfx_idfm_last_error(idfm.h).decode()
        assert np.all(out == -7.0) and np.all(small == -7.0)  # nothing was launched or copied back
        with pytest.raises(CfxError, match=message):
            idfm.normal(bad, _ids(keys), theta)
    with pytest.raises(CfxError, match="cfx_idfm_forces: duplicate parameter id"):
        idfm.forces(trains, [1, 1], theta[:2])
    again, _ = idfm.forces(trains, _ids(keys), theta)  # the handle still works
    idfm.close()
    assert np.array_equal(again, good, equal_nan=True)
    c = dict(O.model_constants("ding2007"), fl=1.0, fv=1.0, fp=0.0)
    with pytest.raises(CfxError, match="only available for the fatigue models") as exc:
        _cfx.Idfm(model_id=_cfx.MODEL_IDS["ding2007"], constants=c, scheme=4, n_steps=1, batch=B, n_trains=3,
                  max_pulses=8, max_shooting=13)
    assert exc.value.code == _cfx.EUNSUPPORTED


def test_class_forces_and_cost_per_train():
    """FesMultiTrainFatigueIdentification end to end at a small size: per-train forces in the caller's order equal the
    IvpSweep curves at the model's constants, and a solve from there stays there with cost_per_train summing to the
    cost."""
    from cocofest_amd import FesMultiTrainFatigueIdentification, IvpSweep, ModelMaker, OdeSolver

    name = "ding2003_with_fatigue"
    solver = OdeSolver.RK4(n_integration_steps=5)
    stims = ([0.0, 0.1, 0.2], [round(0.05 * i, 2) for i in range(10)])
    ivps = [SR.make_ivp(name, MF.M._case(s, "single", 10, None, 1.0, 0), "RK4", 5) for s in stims]
    sweep = IvpSweep(ivps)
    nodes = sweep.integrate(nodes=True)
    sweep.close()
    curves = [nodes["F"][e, : int(nodes["n_shooting"][e]) + 1] for e in range(2)]
    trains = [{"stim_time": list(s), "final_time": 1.0, "force_tracking": [float(v) for v in c],
               "sum_stim_truncation": 10} for s, c in zip(stims, curves)]
    model = ModelMaker.create_model(name, sum_stim_truncation=10)
    ident = FesMultiTrainFatigueIdentification(model, trains, key_parameter_to_identify=list(MF.FATIGUE_KEYS),
                                               ode_solver=solver, n_starts=70, seed=0, start_spread=0.0)
    assert ident.n_shooting == [10, 20] and list(ident.order) == [1, 0]
    F, S = ident.forces(ident.starts(), with_sensitivities=True)
    for e in range(2):
        assert F[e].shape == (len(curves[e]), 70) and S[e].shape == (len(curves[e]), 4, 70)
        assert np.max(np.abs(F[e] - curves[e][:, None])) < PARITY_TOL * np.max(curves[e])
    res = ident.solve(max_iter=3)
    ident.close()
    s = res["starts"]
    assert s["cost_per_train"].shape == (70, 2) and np.all(s["cost"] < 1e-18 * np.max(curves[1]) ** 2)
    np.testing.assert_allclose(s["cost_per_train"].sum(axis=1), s["cost"], rtol=1e-12, atol=1e-300)
    assert np.all(np.diff(s["cost_history"], axis=0) <= 0.0)


# ---- the end-to-end recovery protocol ---------------------------------------------------------------------------------
def _protocol_trains(name):
    """The three recordings of ``MF.fit_cases`` as train dicts, curves from IvpSweep at the model's constants."""
    from cocofest_amd import IvpSweep

    cases = MF.fit_cases()
    ivps = [SR.make_ivp(name, case, MF.FIT_SCHEME, MF.FIT_M) for case in cases]
    sweep = IvpSweep(ivps)
    nodes = sweep.integrate(nodes=True)
    sweep.close()
    trains = []
    for e, case in enumerate(cases):
        N = int(nodes["n_shooting"][e])
        trains.append({"stim_time": list(case["stim_time"]), "final_time": case["final_time"],
                       "sum_stim_truncation": MF.FIT_TRUNCATION,
                       "force_tracking": [float(v) for v in nodes["F"][e, : N + 1]],
                       **{k: {"fixed": v} for k, v in SR.case_values(name, case).items()}})
    return trains


# The CPU reference LM (MF.reference_fit_parallel(name): exact-AD joint normal equations, the same 64 starts) of every
# model: status, iterations, costs and largest relative error per parameter over the starts are in DESIGN section 7e.
# Every GPU start must recover each parameter to 100 x the reference's error.
REFERENCE_ERRORS = {
    "ding2003_with_fatigue": {"alpha_a": 1.89e-7, "alpha_tau1": 1.44e-7, "alpha_km": 1.22e-6, "tau_fat": 1.72e-7},
    "ding2007_with_fatigue": {"alpha_a": 4.40e-7, "alpha_tau1": 1.87e-7, "alpha_km": 2.55e-6, "tau_fat": 2.02e-8},
    "hmed2018_with_fatigue": {"alpha_a": 1.62e-6, "alpha_tau1": 4.72e-7, "alpha_km": 4.25e-6, "tau_fat": 1.83e-7},
}


def _recovery_fit(name):
    """Burst, rest gap of 10 / 30 / 60 s, test burst: all four parameters, tau_fat = 127 s included, from every one of
    64 starts, against the reference's figures."""
    from cocofest_amd import FesMultiTrainFatigueIdentification, ModelMaker, OdeSolver
    from cocofest_amd.identification import CONVERGED_GRADIENT

    solver = OdeSolver.RK4(n_integration_steps=MF.FIT_M)
    trains = _protocol_trains(name)
    model = ModelMaker.create_model(name, sum_stim_truncation=MF.FIT_TRUNCATION)
    keys = list(MF.FATIGUE_KEYS)
    true, lower, upper = MF.fit_bounds(name)
    guess = {k: true[j] * (1.15 if j % 2 == 0 else 0.87) for j, k in enumerate(keys)}
    ident = FesMultiTrainFatigueIdentification(model, trains, key_parameter_to_identify=keys, ode_solver=solver,
                                               initial_guess=guess, n_starts=MF.M.FIT_STARTS, seed=MF.M.FIT_SEED,
                                               start_spread=MF.M.FIT_SPREAD)
    assert ident.n_shooting == [400, 900, 1650]
    th0 = ident.starts()
    assert np.array_equal(th0, MF.M.fit_starts(true, lower, upper))  # the starts the CPU reference ran from
    assert np.all(np.abs(th0 / true[:, None] - 1).max(axis=0) > 0.05)  # no start begins at the generating point
    res = ident.solve()
    ident.close()
    s = res["starts"]
    rel = np.abs(s["theta"] / true - 1)
    print(name, "recovery protocol: status", np.bincount(s["status"], minlength=4), "iterations max",
          s["iterations"].max(), "cost max %.3e" % s["cost"].max(), "initial min %.3e" % s["cost_history"][0].min(),
          "rel err max", " ".join(f"{k} {rel[:, j].max():.2e}" for j, k in enumerate(keys)))
    assert np.all(s["status"] == CONVERGED_GRADIENT), s["status"]
    assert np.all(np.diff(s["cost_history"], axis=0) <= 0.0)  # the cost never rises
    assert s["cost_per_train"].shape == (64, 3)
    np.testing.assert_allclose(s["cost_per_train"].sum(axis=1), s["cost"], rtol=1e-12, atol=1e-300)
    for j, k in enumerate(keys):
        assert np.all(rel[:, j] <= 100 * REFERENCE_ERRORS[name][k]), (k, rel[:, j].max())
        assert abs(res[k] / true[j] - 1) <= 100 * REFERENCE_ERRORS[name][k]


def test_ding2003_recovery_protocol_identifies_all_four_fatigue_parameters():
    _recovery_fit("ding2003_with_fatigue")


def test_ding2007_recovery_protocol_identifies_all_four_fatigue_parameters():
    """One pulse width (4e-4 s) for every recording; the same design and step as Ding2003."""
    _recovery_fit("ding2007_with_fatigue")


def test_hmed2018_recovery_protocol_identifies_all_four_fatigue_parameters():
    """One intensity (60 mA) for every recording; the same design and step as Ding2003."""
    _recovery_fit("hmed2018_with_fatigue")
