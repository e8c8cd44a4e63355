"""Multi-train fatigue-parameter identification, the parts that need no device: self-checks of the exact-autodiff
reference (tests/multitrain_fatigue_ident_reference.py), the argument checks of cfx_idfm_check and the class
validation of ``FesMultiTrainFatigueIdentification``.
"""

import numpy as np
import pytest

from tests import multitrain_fatigue_ident_reference as MF
from tests import sweep_reference as SR

# Two float64 rollouts of the same scheme that differ only in how the exponentials of the calcium forcing are
# grouped: the project's tolerance for these kernels.
TOL = 1e-9


@pytest.mark.parametrize("name", MF.MODELS)
def test_train_rollout_equals_fatigue_setup_when_the_truncation_covers_all_pulses(name):
    """The doublet train (truncation 20 > 8 pulses): rows and controls rebuilt from the activation nodes are the
    oracle's table, so forces and sensitivities are those of ``FatigueSetup``."""
    from tests.fatigue_ident_reference import FatigueSetup

    case = MF.MIXED[1]
    v = SR.case_values(name, case)
    theta = MF.theta_of(name, MF.FATIGUE_KEYS, 3, seed=5)
    for scheme, m in (("RK1", 1), ("RK4", 5)):
        ref = FatigueSetup(name, SR.expanded_times(case), case["final_time"], case["n_shooting"], case["truncation"],
                           scheme, m, pulse_width=v.get("pulse_width"), pulse_intensity=v.get("pulse_intensity"))
        new = MF.setup_of(name, case, scheme, m)
        N = case["n_shooting"]
        assert np.array_equal(new.rows[:N].numpy(), ref.rows[:N].numpy())
        assert (new.controls is None) == (ref.controls is None)
        if new.controls is not None:
            assert np.array_equal(new.controls.numpy(), ref.controls.numpy())
        F, S = new.forces_and_sens(MF.FATIGUE_KEYS, theta)
        F0, S0 = ref.forces_and_sens(MF.FATIGUE_KEYS, theta)
        assert np.array_equal(F, F0) and np.array_equal(S, S0)
        assert np.all(np.max(np.abs(S), axis=0) > 0.0)  # every sensitivity column is live


@pytest.mark.parametrize("name", MF.MODELS)
def test_train_rollout_at_the_model_constants_equals_the_sweep_rollout(name):
    from oracle import fes_oracle as O

    c = O.model_constants(name)
    true = np.array([[c[k]] for k in MF.FATIGUE_KEYS], dtype=float)
    worst = 0.0
    for scheme in MF.SCHEMES:
        for m in (1, 5):
            for case in MF.MIXED:
                F = MF.setup_of(name, case, scheme, m).forces(MF.FATIGUE_KEYS, true)[:, 0]
                ref = SR.sweep_rollout(name, c, MF.packed_train(name, case), scheme, m)[1]
                worst = max(worst, float(np.max(np.abs(F - ref)) / np.max(np.abs(ref))))
    print(f"train rollout against the sweep rollout {name}: {worst:.3e}")
    assert worst < TOL


def test_reference_noise_is_far_below_the_tolerance():
    """jacfwd against jacrev on the test shapes (printed; the GPU tests compare to 1e-9)."""
    for name in MF.MODELS:
        noise = MF.reference_noise(name, "RK4", 5, B=3)
        print(f"reference noise {name} RK4 x 5: {noise:.2e}")
        assert noise < 1e-2 * TOL


def _check(name, trains, P, Nmax, keys, *, scheme=4, m=2, B=8, E=None):
    from cocofest_amd import _cfx

    E = len(trains["n_shooting"]) if E is None else E
    _cfx.idfm_check(_cfx.MODEL_IDS[name], scheme, m, B, E, P, Nmax, [_cfx.FATIGUE_PARAM_IDS[k] for k in keys], trains)


@pytest.mark.parametrize("name", MF.MODELS)
def test_check_accepts_the_mixed_trains(name):
    rng = np.random.default_rng(0)
    y = [rng.uniform(0, 100, c["n_shooting"] + 1) for c in MF.MIXED]
    w = [rng.uniform(0, 2, c["n_shooting"] + 1) for c in MF.MIXED]
    trains, P, Nmax = MF.pack(name, MF.MIXED, y, w)
    assert (P, Nmax) == (8, 13)
    _check(name, trains, P, Nmax, MF.FATIGUE_KEYS)
    _check(name, trains, P, Nmax, MF.SUBSET)
    trains.pop("target"), trains.pop("weight")
    _check(name, trains, P, Nmax, MF.FATIGUE_KEYS)


def test_check_refusals():
    from cocofest_amd import CfxError, _cfx

    name = "ding2007_with_fatigue"
    mid = _cfx.MODEL_IDS[name]
    good, P, Nmax = MF.pack(name, MF.MIXED)

    def bad(**kw):
        t = {k: (None if v is None else v.copy()) for k, v in good.items()}
        for k, (idx, v) in kw.items():
            t[k][idx] = v
        return t

    with pytest.raises(CfxError, match="cfx_idfm_check: unknown parameter id 4"):
        _cfx.idfm_check(mid, 4, 2, 8, 3, P, Nmax, [1, 4], good)
    with pytest.raises(CfxError, match="cfx_idfm_check: duplicate parameter id 1"):
        _cfx.idfm_check(mid, 4, 2, 8, 3, P, Nmax, [1, 1], good)
    with pytest.raises(CfxError, match=r"n_id must be in \[1, 4\]"):
        _cfx.idfm_check(mid, 4, 2, 8, 3, P, Nmax, [], good)
    with pytest.raises(CfxError, match=r"n_id must be in \[1, 4\]"):
        _cfx.idfm_check(mid, 4, 2, 8, 3, P, Nmax, [0, 1, 2, 3, 0], good)
    for plain in ("ding2003", "ding2007", "hmed2018"):
        with pytest.raises(CfxError, match="only available for the fatigue models") as exc:
            _cfx.idfm_check(_cfx.MODEL_IDS[plain], 4, 2, 8, 3, P, Nmax, [1], None)
        assert exc.value.code == _cfx.EUNSUPPORTED
    with pytest.raises(CfxError, match="unknown model") as exc:
        _cfx.idfm_check(6, 4, 2, 8, 3, P, Nmax, [1], None)
    assert exc.value.code == _cfx.EINVAL
    with pytest.raises(CfxError, match="n_trains must be positive"):
        _cfx.idfm_check(mid, 4, 2, 8, 0, P, Nmax, [1], None)
    with pytest.raises(CfxError, match="n_trains must be <= 65535"):
        _cfx.idfm_check(mid, 4, 2, 8, 65536, P, Nmax, [1], None)
    with pytest.raises(CfxError, match="batch, max_pulses and max_shooting must be positive"):
        _cfx.idfm_check(mid, 4, 2, 0, 3, P, Nmax, [1], None)
    with pytest.raises(CfxError, match="max_shooting must be <= 65535"):
        _cfx.idfm_check(mid, 4, 2, 8, 3, P, 65536, [1], None)
    with pytest.raises(CfxError, match="unknown scheme"):
        _cfx.idfm_check(mid, 3, 2, 8, 3, P, Nmax, [1], None)
    for kw, message in (({"times": ((2, 0), -1.0)}, "train 0: pulse 2: time decreases"),
                        ({"times": ((1, 1), np.nan)}, "train 1: pulse 1: time is not finite"),
                        ({"act_node": ((0, 2), 9)}, "train 2: pulse 0: activation node past n_shooting"),
                        ({"act_node": ((3, 0), -1)}, "train 0: pulse 3: activation node is negative"),
                        ({"act_node": ((3, 1), 0)}, "train 1: pulse 3: activation node decreases"),
                        ({"truncation": (1, 0)}, "train 1: truncation must be >= 1"),
                        ({"n_shooting": (2, 14)}, r"train 2: n_shooting must be in \[1, max_shooting\]"),
                        ({"n_pulses": (0, 9)}, r"train 0: n_pulses must be in \[0, max_pulses\]"),
                        ({"final_time": (1, 0.0)}, "train 1: final_time must be positive"),
                        ({"value": ((1, 2), np.nan)}, "train 2: pulse 1: value is not finite")):
        with pytest.raises(CfxError, match="cfx_idfm_check: " + message) as exc:
            _check(name, bad(**kw), P, Nmax, MF.FATIGUE_KEYS)
        assert exc.value.code == _cfx.EINVAL
    y = [np.zeros(c["n_shooting"] + 1) for c in MF.MIXED]
    w = [np.ones(c["n_shooting"] + 1) for c in MF.MIXED]
    w[2][5] = -1.0
    with pytest.raises(CfxError, match="train 2: node 5: weight must be finite and >= 0"):
        _check(name, MF.pack(name, MF.MIXED, y, w)[0], P, Nmax, MF.FATIGUE_KEYS)
    y[0][10] = np.inf
    w[2][5] = 1.0
    with pytest.raises(CfxError, match="train 0: node 10: target is not finite"):
        _check(name, MF.pack(name, MF.MIXED, y, w)[0], P, Nmax, MF.FATIGUE_KEYS)


def test_class_checks_packing_and_the_neighbours_refusals():
    """FesMultiTrainFatigueIdentification without a device: the reference's wording for a model without fatigue,
    FesFatigueIdentification's keys, guesses and bounds, FesMultiTrainIdentification's train handling; the two
    neighbouring classes refuse what they refused."""
    from cocofest_amd import (FesFatigueIdentification, FesMultiTrainFatigueIdentification,
                              FesMultiTrainIdentification, ModelMaker, OdeSolver, _cfx)

    model = ModelMaker.create_model("ding2007_with_fatigue", sum_stim_truncation=10)
    short = {"stim_time": [0.0, 0.1, 0.2], "final_time": 0.5, "pulse_width": {"fixed": 3e-4},
             "force_tracking": [0.0] * 6, "weight": [1, 1, 0, 1, 1, 2], "sum_stim_truncation": 2}
    t = np.linspace(0, 1, 50)
    long_ = {"stim_time": [round(0.05 * i, 2) for i in range(10)], "final_time": 1.0,
             "pulse_width": {"fixed": [2e-4 + 2e-5 * i for i in range(10)]}, "time": list(t), "force": list(100 * t),
             "sum_stim_truncation": 40}
    kw = dict(key_parameter_to_identify=["tau_fat", "alpha_a"], ode_solver=OdeSolver.RK4(n_integration_steps=2),
              n_starts=3)
    ident = FesMultiTrainFatigueIdentification(model, [short, long_], **kw)
    assert ident.param_ids == [_cfx.FATIGUE_PARAM_IDS["tau_fat"], _cfx.FATIGUE_PARAM_IDS["alpha_a"]]
    assert ident.n_shooting == [5, 20] and list(ident.order) == [1, 0]
    tr = ident.trains
    assert list(tr["n_shooting"]) == [20, 5] and list(tr["truncation"]) == [40, 2] and list(tr["n_pulses"]) == [10, 3]
    assert np.array_equal(tr["target"][:, 0], np.interp(np.linspace(0, 1, 21), t, 100 * t))
    assert np.array_equal(tr["weight"][:6, 1], [1, 1, 0, 1, 1, 2]) and np.all(tr["weight"][6:, 1] == 0)
    own = model.identifiable_parameters
    assert np.array_equal(ident.initial_guess, [own["tau_fat"], own["alpha_a"]])
    assert np.allclose(ident.lower, [0.01 * own["tau_fat"], 100 * own["alpha_a"]], rtol=1e-15)  # alpha_a < 0
    assert np.allclose(ident.upper, [100 * own["tau_fat"], 0.01 * own["alpha_a"]], rtol=1e-15)
    assert ident.starts().shape == (2, 3) and not model.stim_time  # the caller's model is left as it is
    single = FesFatigueIdentification(model, stim_time=short["stim_time"], final_time=0.5, force_tracking=[0.0] * 6,
                                      pulse_width={"fixed": 3e-4}, **kw)
    assert np.array_equal(single.lower, ident.lower) and np.array_equal(single.upper, ident.upper)
    assert np.array_equal(single.initial_guess, ident.initial_guess)
    with pytest.raises(ValueError, match="The given model is not valid and should be including the fatigue equation "
                                         "in the model"):
        FesMultiTrainFatigueIdentification(ModelMaker.create_model("ding2007", sum_stim_truncation=10), [short], **kw)
    with pytest.raises(TypeError, match="model must be a FesModel type"):
        FesMultiTrainFatigueIdentification("ding2007_with_fatigue", [short], **kw)
    with pytest.raises(ValueError, match="the available values are .*alpha_a.*tau_fat"):
        FesMultiTrainFatigueIdentification(model, [short], **dict(kw, key_parameter_to_identify=["a_scale"]))
    with pytest.raises(ValueError, match=r"trains\[1\]: force_tracking has 5 values, expected one per node"):
        FesMultiTrainFatigueIdentification(model, [short, dict(short, force_tracking=[0.0] * 5)], **kw)
    with pytest.raises(TypeError, match="trains must be a non-empty list of dict"):
        FesMultiTrainFatigueIdentification(model, [], **kw)
    # the neighbours
    with pytest.raises(ValueError, match="should not be including the fatigue"):
        FesMultiTrainIdentification(model, [short], **dict(kw, key_parameter_to_identify=["a_scale"]))
    with pytest.raises(ValueError, match="should be including the fatigue"):
        FesFatigueIdentification(ModelMaker.create_model("ding2007", sum_stim_truncation=10),
                                 stim_time=short["stim_time"], final_time=0.5, force_tracking=[0.0] * 6,
                                 pulse_width={"fixed": 3e-4}, **kw)


def test_joint_normal_and_lm_reference_on_the_fatigue_rollout():
    """The infrastructure behind the hand-run reference fit (``MF.reference_fit_parallel``), at a size that runs in
    seconds: on two short trains the joint normal equations equal the sums formed from ``forces_and_sens``, and LM
    iterations on the three rates from starts 20 % off lower the cost monotonically."""
    from oracle import fes_autodiff as AD

    name = "ding2003_with_fatigue"
    cases = [MF.MIXED[0], MF.MIXED[2]]
    setups = [MF.setup_of(name, case, "RK4", 2) for case in cases]
    true, lower, upper = MF.fit_bounds(name)
    targets = [st.forces(MF.FATIGUE_KEYS, true[:, None])[:, 0] for st in setups]
    rng = np.random.default_rng(1)
    weights = [rng.uniform(0.5, 2.0, st.N + 1) for st in setups]
    theta = MF.theta_of(name, MF.FATIGUE_KEYS, 2, seed=9)
    normal = MF.joint_normal(setups, MF.FATIGUE_KEYS, targets, weights)
    c, g, H = (t.numpy() for t in normal(AD._t(theta)))
    rc, rg, rH = np.zeros(2), np.zeros((2, 4)), np.zeros((2, 4, 4))
    for st, y, w in zip(setups, targets, weights):
        F, S = st.forces_and_sens(MF.FATIGUE_KEYS, theta)
        r = F - y[:, None]
        rc += st.dt * np.einsum("k,kb,kb->b", w, r, r)
        rg += 2 * st.dt * np.einsum("k,kb,kjb->bj", w, r, S)
        rH += 2 * st.dt * np.einsum("k,kib,kjb->bij", w, S, S)
    assert np.all(rc > 0) and np.all(np.abs(rg).max(axis=1) > 0)
    np.testing.assert_allclose(c, rc, rtol=1e-12)
    np.testing.assert_allclose(g, rg, rtol=1e-10, atol=1e-12 * np.abs(rg).max())
    np.testing.assert_allclose(H, rH, rtol=1e-10, atol=1e-12 * np.abs(rH).max())
    # the three rates (tau_fat is not identifiable from two trains of a second): six LM iterations
    keys = MF.FATIGUE_KEYS[:3]
    rates = MF.joint_normal(setups, keys, targets, weights)
    rep = lambda a: np.repeat(a[:3, None], 2, 1)  # noqa: E731
    th, cost, iters, status, hist = MF.lm_reference(rates, theta[:3], rep(lower), rep(upper), max_iter=6)
    print("six LM iterations on the fatigue rollout: cost", hist[0], "->", cost, "status", status)
    assert np.all(np.diff(hist, axis=0) <= 0) and np.all(cost < hist[0]) and np.all(hist[-1] == cost)
    assert np.all(iters >= 1) and np.all(th >= rep(lower)) and np.all(th <= rep(upper))
