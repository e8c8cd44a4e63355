"""Multi-train force-parameter identification on the GPU: cfx_idm_forces / cfx_idm_normal against exact autodiff
(tests/multitrain_ident_reference.py) and the joint Levenberg-Marquardt fits of ``FesMultiTrainIdentification``.

The mixed trains (``M.MIXED``): E = 4, B = 70 (one full and one partial wave per train), N in {5, 10, 20}, final_time
in {0.5, 1, 2}, 3..12 pulses, truncation 1 / 3 / 5 / larger than the pulse count, a doublet train, a duplicated pulse
time, a first pulse after t = 0, per-pulse widths and intensities; theta within +-20 % of the defaults.  Tolerance 1e-9
on errors scaled per instance by max |F| over the nodes (force) and by the column's max |S| (sensitivities), the
figure of tests/test_identification_gpu.py.
"""

import ctypes as C

import numpy as np
import pytest

from tests import ident_reference as R
from tests import multitrain_ident_reference as M

pytestmark = pytest.mark.gpu

TOL = 1e-9
B = 70
MODELS = ("ding2003", "ding2007", "hmed2018")
GRID = [(n, s, m) for n in MODELS for s in M.SCHEMES for m in (1, 5)]
SCHEME_ID = {"RK1": 1, "RK2": 2, "RK4": 4}


def _ids(keys):
    from cocofest_amd import _cfx

    return [_cfx.PARAM_IDS[k] for k in keys]


def _idm(name, scheme, m, cases, batch=B, targets=None, weights=None):
    """(cfx_idm object, packed trains) of the cases in the order given."""
    from cocofest_amd import _cfx
    from oracle import fes_oracle as O

    trains, P, Nmax = M.pack(name, cases, targets, weights)
    c = dict(O.model_constants(name), fl=1.0, fv=1.0, fp=0.0)
    idm = _cfx.Idm(model_id=_cfx.MODEL_IDS[name], constants=c, scheme=SCHEME_ID[scheme], n_steps=m, batch=batch,
                   n_trains=len(cases), max_pulses=P, max_shooting=Nmax)
    return idm, trains


def _parity(name, scheme, m, subset, which):
    cases = M.MIXED if which == "mixed" else M.LONG
    keys, theta, Fs, Ss = M.reference(name, scheme, m, subset, which)
    idm, trains = _idm(name, scheme, m, cases)
    force, sens = idm.forces(trains, _ids(keys), theta, with_sens=True)
    only, none = idm.forces(trains, _ids(keys), theta)
    idm.close()
    assert none is None and only.tobytes() == force.tobytes()  # sens = NULL: the same force bits
    worst_f, worst_s = 0.0, 0.0
    for e, case in enumerate(cases):
        N = case["n_shooting"]
        assert np.all(np.isnan(force[e, N + 1:])) and np.all(np.isnan(sens[e, N + 1:]))
        assert np.all(force[e, 0] == 0.0) and np.all(sens[e, 0] == 0.0)  # the rest state
        ef, es = R.scaled_errors(force[e, : N + 1], sens[e, : N + 1], Fs[e], Ss[e])
        worst_f, worst_s = max(worst_f, ef), max(worst_s, float(es.max()))
    print(f"idm parity {which} {name} {scheme} x {m} {'subset' if subset else 'full'}: force {worst_f:.2e} "
          f"sens {worst_s:.2e}")
    return worst_f, worst_s


@pytest.mark.parametrize("subset", [False, True], ids=["full", "subset"])
@pytest.mark.parametrize("name, scheme, m", GRID)
def test_forces_and_sensitivities_match_the_autodiff_reference(name, scheme, m, subset):
    """Largest measured on MI355X over the grid: see DESIGN section 7d."""
    ef, es = _parity(name, scheme, m, subset, "mixed")
    assert ef < TOL and es < TOL, (ef, es)


def _float64_sums(force, sens, cases, y, w):
    """cost, grad, gn (packed), their scales and cost per train from cfx_idm_forces outputs, summed in the order of
    ``cases`` with every train's own dt; entries past a train's N are never read."""
    n, nb = sens.shape[2], force.shape[2]
    cost, cpt = np.zeros(nb), []
    grad, sc_g, full = np.zeros((n, nb)), np.zeros((n, nb)), np.zeros((n, n, nb))
    for e, case in enumerate(cases):
        N, dt = case["n_shooting"], case["final_time"] / case["n_shooting"]
        F, S = force[e, : N + 1], sens[e, : N + 1]
        r = F - y[e][:, None]
        cpt.append(dt * np.sum(w[e][:, None] * r * r, axis=0))
        cost = cost + cpt[-1]
        grad = grad + 2 * dt * np.einsum("k,kb,kjb->jb", w[e], r, S)
        sc_g = sc_g + 2 * dt * np.einsum("k,kb,kjb->jb", w[e], np.abs(r), np.abs(S))
        full = full + 2 * dt * np.einsum("k,kib,kjb->ijb", w[e], S, S)
    gn = np.stack([full[i, j] for i in range(n) for j in range(i + 1)])
    sc_h = np.sqrt(np.stack([full[i, i] * full[j, j] for i in range(n) for j in range(i + 1)]))
    return cost, grad, gn, sc_g, sc_h, np.stack(cpt)


@pytest.mark.parametrize("name, scheme, m", [(n, s, m) for n in MODELS for s, m in (("RK1", 1), ("RK2", 5), ("RK4", 5))])
def test_normal_equations_equal_the_sums_over_the_trains(name, scheme, m):
    rng = np.random.default_rng(23)
    for keys in (R.FULL_KEYS[name], M.SUBSET[name]):
        theta = M.theta_of(name, keys, B, seed=29)
        idm, trains = _idm(name, scheme, m, M.MIXED)
        force, sens = idm.forces(trains, _ids(keys), theta, with_sens=True)
        idm.close()
        y, w = [], []
        for e, case in enumerate(M.MIXED):
            N = case["n_shooting"]
            y.append(force[e, : N + 1, 3] * (1 + 0.1 * rng.uniform(-1, 1, N + 1)))
            w.append(rng.uniform(0.5, 2.0, N + 1))
            w[-1][[0, 2, N]] = 0.0
        idm, trains = _idm(name, scheme, m, M.MIXED, targets=y, weights=w)  # NaN past every train's N
        cost, grad, gn, cpt = idm.normal(trains, _ids(keys), theta, per_train=True)
        cost2, grad2, gn2, none = idm.normal(trains, _ids(keys), theta)
        idm.close()
        ref_c, ref_g, ref_h, sc_g, sc_h, ref_cpt = _float64_sums(force, sens, M.MIXED, y, w)
        assert np.all(np.isfinite(cost)) and np.all(np.isfinite(grad)) and np.all(np.isfinite(gn))
        assert np.max(np.abs(cost - ref_c) / ref_c) < TOL
        assert np.max(np.abs(grad - ref_g) / sc_g) < TOL
        assert np.max(np.abs(gn - ref_h) / sc_h) < TOL
        assert np.max(np.abs(cpt - ref_cpt) / ref_cpt) < TOL
        acc = cpt[0].copy()
        for e in range(1, len(M.MIXED)):
            acc = acc + cpt[e]
        assert np.array_equal(acc, cost)  # the sum over the trains, in train order
        assert none is None and cost2.tobytes() == cost.tobytes() and grad2.tobytes() == grad.tobytes()
        assert gn2.tobytes() == gn.tobytes()


@pytest.mark.parametrize("name, scheme, m", [("ding2003", "RK2", 1), ("ding2007", "RK4", 5), ("hmed2018", "RK4", 5),
                                              ("hmed2018", "RK1", 5)])
def test_single_train_agrees_with_the_handle_path(name, scheme, m):
    """E = 1 against cfx_id_forces / cfx_id_normal on a cfx_create handle of the same train.  The bits differ (the
    handle's forcing comes from host tables, this one is factorised on the device)."""
    from tests import sweep_reference as SR

    case = M.MIXED[3]
    N = case["n_shooting"]
    rng = np.random.default_rng(5)
    for keys in (R.FULL_KEYS[name], M.SUBSET[name]):
        theta = M.theta_of(name, keys, B, seed=31)
        ivp = SR.make_ivp(name, case, scheme, m)
        h = ivp.handle(batch=B, layout="soa")
        u = ivp.controls.T.reshape(-1).copy()
        u = u if u.size else None
        F, S = h.id_forces(_ids(keys), theta, u=u, with_sens=True)
        y, w = F[:, 7] * (1 + 0.1 * rng.uniform(-1, 1, N + 1)), rng.uniform(0.5, 2.0, N + 1)
        c0, g0, h0 = h.id_normal(_ids(keys), theta, y, w, u=u)
        h.close()
        idm, trains = _idm(name, scheme, m, [case], targets=[y], weights=[w])
        force, sens = idm.forces(trains, _ids(keys), theta, with_sens=True)
        cost, grad, gn, _ = idm.normal(trains, _ids(keys), theta)
        idm.close()
        ef, es = R.scaled_errors(force[0], sens[0], F, S)
        _, _, _, sc_g, sc_h, _ = _float64_sums(force, sens, [case], [y], [w])
        ec = np.max(np.abs(cost - c0) / c0)
        eg, eh = np.max(np.abs(grad - g0) / sc_g), np.max(np.abs(gn - h0) / sc_h)
        print(f"idm E = 1 against the handle {name} {scheme} x {m}: force {ef:.2e} sens {es.max():.2e} "
              f"cost {ec:.2e} grad {eg:.2e} gn {eh:.2e}")
        assert max(ef, es.max(), ec, eg, eh) < TOL


@pytest.mark.parametrize("name", ["ding2007", "hmed2018"])
def test_position_independence(name):
    """A start alone, in the batch and in the reversed batch, and the trains in another order: identical bits."""
    keys = R.FULL_KEYS[name]
    theta = M.theta_of(name, keys, B, seed=37)
    idm, trains = _idm(name, "RK4", 5, M.MIXED)
    force, sens = idm.forces(trains, _ids(keys), theta, with_sens=True)
    rf, rs = idm.forces(trains, _ids(keys), np.ascontiguousarray(theta[:, ::-1]), with_sens=True)
    idm.close()
    assert np.array_equal(rf[:, :, ::-1], force, equal_nan=True) and np.array_equal(rs[..., ::-1], sens, equal_nan=True)
    one, trains1 = _idm(name, "RK4", 5, M.MIXED, batch=1)
    for b in (0, 63, 64, 69):
        f1, s1 = one.forces(trains1, _ids(keys), np.ascontiguousarray(theta[:, b: b + 1]), with_sens=True)
        assert np.array_equal(f1[:, :, 0], force[:, :, b], equal_nan=True)
        assert np.array_equal(s1[..., 0], sens[..., b], equal_nan=True)
    one.close()
    perm = [2, 0, 3, 1]
    idm, trains = _idm(name, "RK4", 5, [M.MIXED[i] for i in perm])
    pf, ps = idm.forces(trains, _ids(keys), theta, with_sens=True)
    idm.close()
    for j, i in enumerate(perm):
        N = M.MIXED[i]["n_shooting"]
        assert np.array_equal(pf[j, : N + 1], force[i, : N + 1]) and np.array_equal(ps[j, : N + 1], sens[i, : N + 1])


def test_device_buffers_give_the_host_bits():
    import torch

    name = "hmed2018"
    keys = R.FULL_KEYS[name]
    theta = M.theta_of(name, keys, B, seed=43)
    y = [np.linspace(0, 50, c["n_shooting"] + 1) for c in M.MIXED]
    w = [np.ones(c["n_shooting"] + 1) for c in M.MIXED]
    idm, trains = _idm(name, "RK4", 5, M.MIXED, targets=y, weights=w)
    force, sens = idm.forces(trains, _ids(keys), theta, with_sens=True)
    host = idm.normal(trains, _ids(keys), theta, per_train=True)
    dev = {k: (None if v is None else torch.as_tensor(v).cuda()) for k, v in trains.items()}
    dth = torch.as_tensor(theta).cuda()
    dforce, dsens = idm.forces(dev, _ids(keys), dth, with_sens=True)
    dnorm = idm.normal(dev, _ids(keys), dth, per_train=True)
    torch.cuda.synchronize()
    idm.close()
    assert np.array_equal(dforce.cpu().numpy(), force, equal_nan=True)
    assert np.array_equal(dsens.cpu().numpy(), sens, equal_nan=True)
    for a, b in zip(dnorm, host):
        assert np.array_equal(a.cpu().numpy(), b)


def test_invalid_arguments_launch_nothing():
    from cocofest_amd import CfxError, _cfx
    from oracle import fes_oracle as O

    name = "ding2007"
    keys = R.FULL_KEYS[name]
    theta = M.theta_of(name, keys, B, seed=47)
    y = [np.zeros(c["n_shooting"] + 1) for c in M.MIXED]
    w = [np.ones(c["n_shooting"] + 1) for c in M.MIXED]
    idm, trains = _idm(name, "RK2", 1, M.MIXED, targets=y, weights=w)
    good, _ = idm.forces(trains, _ids(keys), theta)
    ids = np.asarray(_ids(keys), dtype=np.int32)
    idp = ids.ctypes.data_as(C.POINTER(C.c_int32))
    for key, idx, value, message in (("times", (2, 0), -1.0, "train 0: pulse 2: time decreases"),
                                     ("act_node", (0, 2), 6, "train 2: pulse 0: activation node past n_shooting"),
                                     ("truncation", 1, 0, "train 1: truncation must be >= 1"),
                                     ("weight", (3, 1), -2.0, "train 1: node 3: weight must be finite")):
        bad = {k: (None if v is None else v.copy()) for k, v in trains.items()}
        bad[key][idx] = value
        st, keep = _cfx._idm_trains(bad, 4, idm.max_pulses, idm.max_shooting, True)
        out = np.full((4, idm.max_shooting + 1, B), -7.0)
        small = np.full((1 + 6 + 21, B), -7.0)
        if key != "weight":  # the forces call does not read the weights
            rc = idm.lib.cfx_idm_forces(idm.h, C.byref(st), 6, idp, theta.ctypes.data, out.ctypes.data, None, 0, None)
            assert rc == _cfx.EINVAL and message in idm.lib.cfx_idm_last_error(idm.h).decode()
        rc = idm.lib.cfx_idm_normal(idm.h, C.byref(st), 6, idp, theta.ctypes.data, small[0:1].ctypes.data,
                                    small[1:7].ctypes.data, small[7:].ctypes.data, None, 0, None)
        assert rc == _cfx.EINVAL and message in idm.lib.cfx_idm_last_error(idm.h).decode()
        assert np.all(out == -7.0) and np.all(small == -7.0)  # nothing was launched or copied back
        with pytest.raises(CfxError, match=message):
            idm.normal(bad, _ids(keys), theta)
    with pytest.raises(CfxError, match="duplicate parameter id"):
        idm.forces(trains, [1, 1], theta[:2])
    again, _ = idm.forces(trains, _ids(keys), theta)  # the handle still works
    idm.close()
    assert np.array_equal(again, good, equal_nan=True)
    c = dict(O.model_constants("ding2007_with_fatigue"), fl=1.0, fv=1.0, fp=0.0)
    with pytest.raises(CfxError, match="not available for the fatigue models") as exc:
        _cfx.Idm(model_id=_cfx.MODEL_IDS["ding2007_with_fatigue"], constants=c, scheme=4, n_steps=1, batch=B,
                 n_trains=4, max_pulses=12, max_shooting=20)
    assert exc.value.code == _cfx.EUNSUPPORTED


@pytest.mark.parametrize("name", MODELS)
def test_a_train_no_handle_could_carry(name):
    """40 pulses, truncation 40, N = 40 next to a short train: cfx_create stops at truncation 32."""
    from cocofest_amd import CfxError
    from tests import sweep_reference as SR

    with pytest.raises(CfxError, match=r"truncation must be in \[1, 32\]"):
        SR.make_ivp(name, M.LONG[0], "RK4", 2).handle(batch=1)
    for subset in (False, True):
        ef, es = _parity(name, "RK4", 2, subset, "long")
        assert ef < TOL and es < TOL, (ef, es)


# ---- fits -------------------------------------------------------------------------------------------------
def _fit(which, max_iter=100):
    """The product's fit of ``M.fit_problem``: curves generated by IvpFes at the model defaults (RK4 x 5), 64 seeded
    starts (spread 0.2) around the guess true x 1.15 / x 0.87 alternating."""
    from cocofest_amd import FesMultiTrainIdentification, IvpFes, ModelMaker, OdeSolver

    name, keys, values = M.fit_problem(which)
    kw = "pulse_width" if name == "ding2007" else "pulse_intensity"
    solver = OdeSolver.RK4(n_integration_steps=M.FIT_M)
    trains = []
    for v in values:
        model = ModelMaker.create_model(name, stim_time=list(M.TRAIN_THEN_REST), sum_stim_truncation=10)
        ivp = IvpFes({"model": model, kw: v}, {"final_time": 1.0, "ode_solver": solver})
        curve = [float(x) for x in ivp.integrate(return_time=False)["F"][0][:: M.FIT_M]]
        ivp.close()
        trains.append({"stim_time": list(M.TRAIN_THEN_REST), "final_time": 1.0, "force_tracking": curve,
                       kw: {"fixed": v}})
    model = ModelMaker.create_model(name, sum_stim_truncation=10)
    true = dict(model.identifiable_parameters)
    guess = {k: true[k] * (1.15 if j % 2 == 0 else 0.87) for j, k in enumerate(keys)}
    ident = FesMultiTrainIdentification(model, trains, key_parameter_to_identify=keys, ode_solver=solver,
                                        initial_guess=guess, n_starts=M.FIT_STARTS, seed=M.FIT_SEED,
                                        start_spread=M.FIT_SPREAD)
    assert ident.n_shooting == [20, 20, 20]
    th0 = ident.starts()
    tv = np.array([true[k] for k in keys])
    assert np.array_equal(th0, M.fit_starts(tv, ident.lower, ident.upper))  # the starts the CPU reference ran from
    assert np.all(np.abs(th0 / tv[:, None] - 1).max(axis=0) > 0.05)  # no start begins at the generating point
    res = ident.solve(max_iter=max_iter)
    ident.close()
    s = res["starts"]
    print(which, "status", np.bincount(s["status"], minlength=4), "iterations max", s["iterations"].max(),
          "cost max %.3e" % s["cost"].max(), "rel err max",
          " ".join(f"{k} {np.abs(s['theta'][:, j] / tv[j] - 1).max():.2e}" for j, k in enumerate(keys)))
    assert np.all(np.diff(s["cost_history"], axis=0) <= 0.0)  # the cost never rises
    assert np.all(s["cost_history"][-1] == s["cost"]) and res["cost"] == s["cost"].min()
    assert s["cost_per_train"].shape == (64, 3)
    np.testing.assert_allclose(s["cost_per_train"].sum(axis=1), s["cost"], rtol=1e-12, atol=1e-300)
    assert np.array_equal(res["cost_per_train"], s["cost_per_train"][res["best_start"]])
    return keys, tv, res


# The CPU reference LM (M.reference_fit("ding2007"): exact-AD joint normal equations, the same 64 starts) stops on the
# gradient test from every start within 9 iterations, cost <= 1.04e-11, no parameter at a bound, largest relative
# errors over the starts as below.  Every GPU start must recover each parameter to 100 x that.
DING2007_REFERENCE_ERRORS = {"a_scale": 2.14e-6, "km_rest": 5.03e-6, "tau1_rest": 2.87e-7, "tau2": 3.33e-5,
                             "pd0": 1.69e-9, "pdt": 4.62e-9}


def test_ding2007_three_pulse_widths_identify_all_six_parameters():
    """Three trains, each under ONE constant pulse width (2e-4, 3.5e-4, 6e-4 s): with a single width a_scale, pd0
    and pdt enter only through a_scale E(pw) and cannot be told apart; jointly they are identified."""
    from cocofest_amd.identification import CONVERGED_GRADIENT

    keys, true, res = _fit("ding2007")
    s = res["starts"]
    assert np.all(s["status"] == CONVERGED_GRADIENT), s["status"]
    assert np.all(s["iterations"] >= 1) and np.all(s["cost"] < 1e-3 * s["cost_history"][0])
    for j, k in enumerate(keys):
        err = np.abs(s["theta"][:, j] / true[j] - 1)
        assert np.all(err <= 100 * DING2007_REFERENCE_ERRORS[k]), (k, err.max())
        assert abs(res[k] / true[j] - 1) <= 100 * DING2007_REFERENCE_ERRORS[k]


# The CPU reference LM of the Hmed2018 fit (M.reference_fit("hmed2018", max_iter=25), the same 64 starts, run in chunks
# of starts) does NOT converge from every start.  Its figures, per start, are what the GPU test asserts:
#   * status: CONVERGED_GRADIENT from 58 starts (in <= 18 iterations), NOT_CONVERGED from the 6 starts of
#     HMED2018_REFERENCE_NOT_CONVERGED, no step-size stop and no stall;
#   * final cost < 1e-3 of the initial cost from every start (largest 8.7e-6) except the four of
#     HMED2018_REFERENCE_SLOW, whose value is the reference's final / initial cost after the 25 iterations (their
#     initial costs are 2.6e4 to 5.6e6, against 35.7 from the guess itself);
#   * the cost never rises and is finite from every start (largest final cost 3.6e4).
# The starts it converges from recover km_rest and ar to 1.4e-2 (they trade off) and the other six to 8.1e-5; the six
# others are up to 95 % off.
HMED2018_MAX_ITER = 25
HMED2018_REFERENCE_NOT_CONVERGED = (10, 23, 26, 30, 55, 58)
HMED2018_REFERENCE_SLOW = {10: 3.58e-3, 26: 8.98e-2, 55: 0.203, 58: 3.39e-3}  # start: final / initial cost


def test_hmed2018_eight_parameters_over_three_intensity_ramps():
    """All eight parameters from three trains under intensity ramps 30..66, 45..100 and 95..50 mA, 25 LM iterations.
    The reference's figures (above, and DESIGN section 7d): the parameters are not recovered from every start
    (a_rest, ar and km_rest trade off along a valley), so no parameter is asserted."""
    from cocofest_amd.identification import CONVERGED_GRADIENT, NOT_CONVERGED

    keys, true, res = _fit("hmed2018", max_iter=HMED2018_MAX_ITER)
    s = res["starts"]
    ratio = s["cost"] / s["cost_history"][0]
    slow = np.flatnonzero(~(ratio < 1e-3))
    print("hmed2018 NOT_CONVERGED", np.flatnonzero(s["status"] == NOT_CONVERGED).tolist(), "final / initial >= 1e-3",
          [(int(b), float("%.3g" % ratio[b])) for b in slow], "largest of the others %.2e" % np.delete(ratio, slow).max())
    assert np.all(np.isfinite(s["cost"])) and np.all(np.isfinite(s["theta"]))
    assert np.all(np.isin(s["status"], (CONVERGED_GRADIENT, NOT_CONVERGED))), s["status"]
    assert np.count_nonzero(s["status"] == NOT_CONVERGED) <= len(HMED2018_REFERENCE_NOT_CONVERGED)
    assert np.all(s["iterations"] >= 1) and np.all(s["cost"] < s["cost_history"][0])
    for b in range(M.FIT_STARTS):
        if b not in HMED2018_REFERENCE_SLOW:
            assert ratio[b] < 1e-3, (b, ratio[b])
