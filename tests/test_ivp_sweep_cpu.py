"""IvpSweep without a device: packing, per-interval controls, the kernel's formulation restated in numpy
(tests/sweep_reference.py) against the oracle, the cfx_sweep_check messages, the IvpSweep refusals and the sort.

Formulation bound: the restatement differs from ``oracle.fes_oracle.ivp_integrate`` only by the factorised
exponentials, exp(-(t - t_i) / tauc) = exp(-(t - t_k) / tauc) exp(-(t_k - t_i) / tauc).  Measured on the mixed batch,
scaled per state by its largest magnitude over the trajectory: 5.4e-12 at worst (ding2003_with_fatigue, RK4 x 5, a
train with N = 4 whose coarse steps carry a calcium stage value across -Km, where the force row is singular and
rounding differences are amplified about a thousand times; well-resolved trains stay below 1e-13).  Asserted at
100 x that, capped at 1e-11, the project's bar for a reassociation: 1e-11.
"""

import numpy as np
import pytest

from oracle import fes_oracle as O
from tests import sweep_reference as R

MEASURED = 5.4e-12
FORMULATION_TOL = min(100 * MEASURED, 1e-11)
COMBOS = [("RK1", 1), ("RK2", 5), ("RK4", 1), ("RK4", 5)]


@pytest.mark.parametrize("name", O.MODEL_NAMES)
def test_packing_and_controls(name):
    """The window rebuilt from the packed activation nodes and truncation is the model's stimulation table at every
    node, exactly; the per-interval controls implied by the per-pulse values are IvpFes._build_controls."""
    from cocofest_amd.ivp import pack_train

    for case in R.mixed_cases():
        ivp = R.make_ivp(name, case)
        train = pack_train(ivp)
        assert train["n_shooting"] == R.case_n_shooting(case)
        table, _ = ivp.model.get_numerical_data_time_series(ivp.n_shooting, ivp.final_time)
        assert np.array_equal(R.window_rows(train), table["stim_time"][:, 0, :].T), case
        assert np.array_equal(R.interval_controls(name, train), ivp.controls), case
        assert all(0 <= a <= train["n_shooting"] for a in train["act_node"])


def test_mixed_batch_covers_what_it_says():
    from cocofest_amd.ivp import pack_train

    cases = R.mixed_cases()
    trains = [pack_train(R.make_ivp("ding2003", c)) for c in cases]
    assert len(cases) == 70
    assert {t["n_shooting"] for t in trains} == {3, 4, 10, 20}
    assert {len(t["times"]) for t in trains} == set(range(1, 13))
    assert {t["truncation"] for t in trains} == set(range(1, 13))
    assert {c["final_time"] for c in cases} == {0.3, 0.5, 1.0}
    assert {c["pulse_mode"] for c in cases} == {"single", "doublet", "triplet"}
    assert any(t["truncation"] < len(t["times"]) for t in trains)
    assert any(t["truncation"] > len(t["times"]) for t in trains)
    assert any(len(set(t["times"])) < len(t["times"]) for t in trains)  # a duplicated pulse time
    assert any(t["times"] == [0.0] for t in trains)
    # a pulse strictly between two nodes: its activation node's time is later than the pulse
    assert any(a * t["final_time"] / t["n_shooting"] > s + 1e-9 for t in trains for a, s in zip(t["act_node"], t["times"]))


def test_pulse_past_the_last_node_is_left_out():
    from cocofest_amd.ivp import activation_nodes, pack_train

    assert activation_nodes([0.0, 0.1, 0.2, 0.25], 3, 0.3) == [0, 1, 2, 3]  # 0.3 s / 3: the float <= misses 0.1 and 0.2
    case = dict(R.mixed_cases()[0], stim_time=[0.0, 0.5, 1.5], truncation=3)
    train = pack_train(R.make_ivp("ding2003", case))
    assert train["times"] == [0.0, 0.5] and train["act_node"] == [0, 5]


@pytest.mark.parametrize("name", O.MODEL_NAMES)
def test_formulation_against_oracle(name):
    from cocofest_amd.ivp import pack_train

    c = O.model_constants(name)
    worst = 0.0
    for scheme, m in COMBOS:
        for case in R.mixed_cases():
            train = pack_train(R.make_ivp(name, case, scheme, m))
            worst = max(worst, R.scaled_error(R.sweep_rollout(name, c, train, scheme, m),
                                              R.oracle_nodes(name, case, scheme, m)))
    print(f"formulation {name}: {worst:.3e}")
    assert worst <= FORMULATION_TOL


def test_formulation_with_a_start_state():
    from cocofest_amd.ivp import pack_train

    name = "ding2003_with_fatigue"
    c = O.model_constants(name)
    x0 = np.array([0.2, 30.0, 2800.0, 0.055, 0.11])
    case = R.mixed_cases()[8]
    train = pack_train(R.make_ivp(name, case, "RK4", 5))
    got, ref = R.sweep_rollout(name, c, train, "RK4", 5, x0=x0), R.oracle_nodes(name, case, "RK4", 5, x0=x0)
    assert np.array_equal(got[:, 0], x0)
    assert R.scaled_error(got, ref) <= FORMULATION_TOL


# ---- cfx_sweep_check ------------------------------------------------------------------------------------------------
def _trains(B=3, P=4, N=10):
    return {"times": np.tile(np.array([[0.0], [0.1], [0.2], [0.3]]), (1, B)),
            "act_node": np.tile(np.array([[0], [1], [2], [3]], dtype=np.int32), (1, B)),
            "value": np.full((P, B), 0.0004),
            "n_pulses": np.full(B, P, dtype=np.int32), "truncation": np.full(B, 2, dtype=np.int32),
            "n_shooting": np.full(B, N, dtype=np.int32), "final_time": np.ones(B)}


def _check(trains, model=0, scheme=4, n_steps=2, B=3, P=4, Nmax=10):
    from cocofest_amd import _cfx

    _cfx.sweep_check(model, scheme, n_steps, B, P, Nmax, trains)


def _refused(match, trains=None, **kw):
    from cocofest_amd import CfxError, _cfx

    with pytest.raises(CfxError, match=match) as e:
        _check(trains, **kw)
    assert e.value.code == _cfx.EINVAL


def test_check_accepts_a_valid_batch():
    for model in range(6):
        _check(_trains(), model=model)
    _check(None)
    t = _trains()
    t["n_pulses"][1] = 0  # an empty train
    t["value"] = None  # Ding2003 reads no per-pulse value
    _check(t)


def test_check_messages():
    t = _trains()
    t["times"][2, 1] = 0.05
    _refused(r"instance 1: pulse 2: time decreases", t)
    t = _trains()
    t["act_node"][3, 2] = 11
    _refused(r"instance 2: pulse 3: activation node past n_shooting", t)
    t = _trains()
    t["act_node"][1, 0] = -1
    _refused(r"instance 0: pulse 1: activation node is negative", t)
    t = _trains()
    t["act_node"][2, 0] = 0
    _refused(r"instance 0: pulse 2: activation node decreases", t)
    t = _trains()
    t["truncation"][1] = 0
    _refused(r"instance 1: truncation must be >= 1", t)
    t = _trains()
    t["n_pulses"][2] = 5
    _refused(r"instance 2: n_pulses must be in \[0, max_pulses\]", t)
    t = _trains()
    t["n_shooting"][0] = 65536
    _refused(r"instance 0: n_shooting must be <= 65535", t)
    t = _trains()
    t["n_shooting"][0] = 11
    _refused(r"instance 0: n_shooting must be in \[1, max_shooting\]", t)
    t = _trains()
    t["final_time"][1] = 0.0
    _refused(r"instance 1: final_time must be positive", t)
    t = _trains()
    t["value"] = None
    _refused(r"sweep: trains\['value'\] is missing", t, model=2)
    _refused(r"cfx_sweep_check: max_shooting must be <= 65535", Nmax=65536)
    _refused(r"cfx_sweep_check: unknown model", model=6)
    _refused(r"cfx_sweep_check: unknown model", model=-1)
    _refused(r"cfx_sweep_check: unknown scheme", scheme=3)
    _refused(r"cfx_sweep_check: unknown scheme", scheme=16)  # collocation
    _refused(r"must be positive", n_steps=0)


# ---- IvpSweep -------------------------------------------------------------------------------------------------------
def _ivp(name="ding2003", scheme="RK4", m=2, previous_stim=None, **attrs):
    from cocofest_amd import IvpFes, ModelMaker, OdeSolver

    kw = {"previous_stim": previous_stim} if previous_stim else {}
    model = ModelMaker.create_model(name, stim_time=[0.0, 0.1, 0.2], sum_stim_truncation=3, **kw)
    for k, v in attrs.items():
        setattr(model, k, v)
    solver = OdeSolver.COLLOCATION() if scheme == "COLLOCATION" else getattr(OdeSolver, scheme)(n_integration_steps=m)
    return IvpFes({"model": model}, {"final_time": 1.0, "ode_solver": solver})


def test_refusals_name_the_first_offending_index():
    from cocofest_amd import IvpSweep

    with pytest.raises(ValueError, match=r"ivps\[2\]: model class DingModelFrequencyWithFatigue differs"):
        IvpSweep([_ivp(), _ivp(), _ivp("ding2003_with_fatigue"), _ivp("hmed2018")])
    with pytest.raises(ValueError, match=r"ivps\[1\]: model constants differ"):
        IvpSweep([_ivp(), _ivp(tauc=0.03)])
    with pytest.raises(ValueError, match=r"ivps\[1\]: ode_solver differs"):
        IvpSweep([_ivp(), _ivp(scheme="RK2")])
    with pytest.raises(ValueError, match=r"ivps\[2\]: ode_solver differs"):
        IvpSweep([_ivp(), _ivp(), _ivp(m=3)])
    with pytest.raises(ValueError, match=r"ivps\[0\]: OdeSolver.COLLOCATION is not supported"):
        IvpSweep([_ivp(scheme="COLLOCATION")])
    with pytest.raises(ValueError, match=r"ivps\[1\]: previous_stim is not supported"):
        IvpSweep([_ivp(), _ivp(previous_stim={"time": [-0.2, -0.1]})])
    with pytest.raises(ValueError, match="at least one"):
        IvpSweep([])
    # the placeholders the models pad previous_stim with themselves are no history
    sweep = IvpSweep([_ivp(), _ivp("ding2003")])
    assert sweep.batch == 2 and sweep.max_pulses == 3 and sweep.max_shooting == 10


def test_sort_and_unsort_round_trip():
    from cocofest_amd import IvpSweep
    from cocofest_amd.ivp import pack_train, sweep_order

    cases = list(R.mixed_cases())
    perm = np.random.default_rng(3).permutation(len(cases))
    ivps = [R.make_ivp("hmed2018", cases[i], "RK2", 5) for i in perm]
    sweep = IvpSweep(ivps)
    order = sweep.order
    assert sorted(order.tolist()) == list(range(len(cases)))
    work = [t["n_shooting"] * 5 * max(1, min(t["truncation"], len(t["times"]))) for t in map(pack_train, ivps)]
    assert np.array_equal(order, sweep_order(work))
    assert all(work[a] >= work[b] for a, b in zip(order, order[1:]))  # heaviest first
    # the packed column j is the caller's instance order[j] ...
    for j, i in enumerate(order):
        t = pack_train(ivps[i])
        n = len(t["times"])
        assert sweep.trains["n_pulses"][j] == n and sweep.trains["n_shooting"][j] == t["n_shooting"]
        assert np.array_equal(sweep.trains["times"][:n, j], t["times"])
        assert np.array_equal(sweep.trains["value"][:n, j], t["value"])
    # ... and the inverse permutation puts a packed result back in the caller's order
    inverse = np.empty(len(order), dtype=np.int64)
    inverse[order] = np.arange(len(order))
    assert np.array_equal(sweep.trains["n_shooting"][inverse], sweep.n_shooting)
