"""Train search without a device: the metrics of cfx_sweep_score restated in numpy against the oracle, the target
rule, cfx_sweep_target_check, IvpSweep.from_trains against IvpSweep([IvpFes...]) and TrainSearch's grid and ranking.

Restatement bound: the six formulas of include/cfx.h on the node forces of ``sweep_reference.sweep_rollout`` (the
kernel's factorised rollout in numpy) against the same formulas on ``sweep_reference.oracle_nodes``, both reduced with
``math.fsum`` (tests/train_search_reference.py).  Errors are scaled: track by dt sum (|F_k| + |y_k|)^2, impulse (and
mean_force) by dt sum |F_k|, peak and end_error by max(|F|, |y|); peak_node is exact.  Measured on the mixed batch, six
models x RK1 / RK2 / RK4 x m in {1, 5}: 3.0e-11 at worst (ding2003_with_fatigue; ding2003 1.7e-12, ding2007 3.4e-12,
ding2007_with_fatigue 4.7e-12, hmed2018 8.6e-12, hmed2018_with_fatigue 2.2e-12), the size of the node-state errors
the sweep tests trace to the coarse trains whose stage values cross the force row's singularity (DESIGN section 7c:
2.5e-11 on the same model).  Asserted at 100 x that, capped at the sweep tests' 1e-9: 1e-9.
"""

import ctypes as C
import math
import pathlib
import re

import numpy as np
import pytest

from oracle import fes_oracle as O
from tests import sweep_reference as R
from tests import train_search_reference as S

MEASURED = 3.0e-11
RESTATEMENT_TOL = min(100 * MEASURED, 1e-9)
COMBOS = [(s, m) for s in ("RK1", "RK2", "RK4") for m in (1, 5)]
PEAK_GAP = 1e-6


@pytest.mark.parametrize("name", O.MODEL_NAMES)
def test_metrics_restated_against_the_oracle(name):
    from cocofest_amd.ivp import pack_train

    c = O.model_constants(name)
    worst = 0.0
    for scheme, m in COMBOS:
        for case in R.mixed_cases():
            tf = case["final_time"]
            train = pack_train(R.make_ivp(name, case, scheme, m))
            ref_force = R.oracle_nodes(name, case, scheme, m)[1]
            # a peak_node can differ legitimately only between nodes whose forces agree to rounding: none here
            assert S.top_two_gap(ref_force) > PEAK_GAP, (name, scheme, m, case)
            ref, yk = S.metrics_of(ref_force, tf, S.TARGET_Y, S.TARGET_DT)
            got, _ = S.metrics_of(R.sweep_rollout(name, c, train, scheme, m)[1], tf, S.TARGET_Y, S.TARGET_DT)
            assert got["peak_node"] == ref["peak_node"], (name, scheme, m, case)
            worst = max(worst, S.scaled_metric_error(got, ref, S.metric_scales(ref_force, tf, yk)))
    print(f"score restatement {name}: {worst:.3e}")
    assert worst <= RESTATEMENT_TOL


def test_metric_formulas_on_a_hand_case():
    # F = 0, 2, 4, 2 at t = 0, 0.1, 0.2, 0.3 against the constant target 1
    got, yk = S.metrics_of([0.0, 2.0, 4.0, 2.0], 0.3, [1.0], 1.0)
    dt = 0.3 / 3
    assert np.array_equal(yk, np.ones(4))
    assert got["track"] == dt * 12.0 and got["impulse"] == dt * 7.0
    assert got["peak"] == 4.0 and got["peak_node"] == 2 and got["end_error"] == 1.0
    assert got["mean_force"] == got["impulse"] / 0.3
    # the first node that attains the peak
    assert S.metrics_of([3.0, 5.0, 5.0], 1.0, [0.0], 1.0)[0]["peak_node"] == 1
    assert S.metrics_of([5.0, 5.0], 1.0, [0.0], 1.0)[0]["peak_node"] == 0  # n_shooting = 1


# ---- the target rule ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_samples", [1, 2, 8])
def test_target_rule(n_samples):
    y = list(S.TARGET_Y[:n_samples]) if n_samples > 1 else [75.0]
    sdt = 0.1
    end = (n_samples - 1) * sdt
    # a table shorter than final_time (the last sample is held) and one longer
    for tf, N in ((end + 0.45, 13), (max(end, sdt) * 0.6, 7)):
        got = S.node_targets(y, sdt, N, tf)
        times = np.arange(N + 1) * (tf / N)
        ref = np.interp(times, np.arange(n_samples) * sdt, y)  # clamps beyond the table: hold-last
        assert np.max(np.abs(got - ref)) <= 4 * np.finfo(float).eps * max(np.abs(y))
        assert np.all(got[times >= end] == y[-1])
    if n_samples == 1:
        assert S.target_at(y, -1.0, 0.3) == 75.0  # sample_dt is ignored
        return
    # a node time exactly on a sample: tf = 0.5, N = 5, k = 1 -> t = 0.1 exactly, u = 1
    assert 1 * (0.5 / 5) == 0.1 and 0.1 * (1.0 / 0.1) == 1.0
    assert S.target_at(y, sdt, 0.1) == y[1]
    assert S.target_at(y, sdt, 0.0) == y[0]
    # halfway: one fma
    assert S.target_at(y, 0.5, 0.25) == y[0] + 0.5 * (y[1] - y[0])
    # at and past the last sample
    assert S.target_at(y, sdt, (n_samples - 1) * sdt * 1.0000001) == y[-1]
    assert S.target_at(y, sdt, 1e9) == y[-1]


def _target_check(y, n_samples, sample_dt):
    from cocofest_amd import _cfx

    lib = _cfx.load_library()
    arr = None if y is None else np.ascontiguousarray(y, dtype=np.float64)
    tg = _cfx.SweepTarget(None if arr is None else arr.ctypes.data, n_samples, sample_dt)
    rc = lib.cfx_sweep_target_check(C.byref(tg))
    return rc, lib.cfx_last_error(None).decode()


def test_target_check():
    from cocofest_amd import CfxError, _cfx

    assert _target_check([1.0, 2.0, 3.0], 3, 0.1)[0] == _cfx.OK
    assert _target_check([1.0], 1, 0.0)[0] == _cfx.OK  # one sample: sample_dt is ignored
    for y, n, sdt, field in (([1.0, 2.0], 0, 0.1, "n_samples"), ([1.0, 2.0], 2, 0.0, "sample_dt"),
                             ([1.0, 2.0], 2, -0.1, "sample_dt"), ([1.0, 2.0], 2, math.nan, "sample_dt"),
                             ([1.0, math.nan, 2.0], 3, 0.1, r"y\[1\]"), ([1.0, math.inf], 2, 0.1, r"y\[1\]"),
                             (None, 2, 0.1, "y is NULL")):
        rc, message = _target_check(y, n, sdt)
        assert rc == _cfx.EINVAL
        assert "cfx_sweep_target_check: target: " in message and re.search(field, message), message
    lib = _cfx.load_library()
    assert lib.cfx_sweep_target_check(None) == _cfx.EINVAL
    _cfx.sweep_target_check([1.0, 2.0], 0.5)
    with pytest.raises(CfxError, match="sample_dt must be positive"):
        _cfx.sweep_target_check([1.0, 2.0], 0.0)
    with pytest.raises(CfxError, match="n_samples must be >= 1"):
        _cfx.sweep_target_check([], 0.5)


def test_header_binding_and_abi():
    from cocofest_amd import _cfx

    text = (pathlib.Path(__file__).resolve().parents[1] / "include" / "cfx.h").read_text()
    assert int(re.search(r"#define CFX_SWEEP_N_METRICS (\d+)", text).group(1)) == len(_cfx.SWEEP_METRICS) == 6
    assert _cfx.SWEEP_METRICS == S.METRICS
    assert "cfx_sweep_score" in _cfx.SIGNATURES and "cfx_sweep_target_check" in _cfx.SIGNATURES
    assert [f[0] for f in _cfx.SweepTarget._fields_] == ["y", "n_samples", "sample_dt"]
    assert _cfx.load_library().cfx_abi_version() == _cfx.ABI_VERSION  # additions only: the number does not move


# ---- IvpSweep.from_trains -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["ding2003_with_fatigue", "ding2007", "hmed2018"])
def test_from_trains_packs_what_ivpfes_packs(name, monkeypatch):
    from cocofest_amd import IvpFes, IvpSweep, ModelMaker, OdeSolver

    cases = R.mixed_cases()
    assert {c["pulse_mode"] for c in cases} == {"single", "doublet", "triplet"}
    assert any(c["n_shooting"] is None for c in cases)
    by_ivp = IvpSweep([R.make_ivp(name, case, "RK2", 5) for case in cases])
    model = ModelMaker.create_model(name, stim_time=[0.0], sum_stim_truncation=7)

    def no_ivp(*a, **k):
        raise AssertionError("from_trains constructed an IvpFes")

    monkeypatch.setattr(IvpFes, "__init__", no_ivp)
    direct = IvpSweep.from_trains(model, [S.train_dict(name, case) for case in cases],
                                  ode_solver=OdeSolver.RK2(n_integration_steps=5))
    assert model.stim_time == [0.0] and model._sum_stim_truncation == 7  # the model is left as it was
    assert set(direct.trains) == set(by_ivp.trains)
    for key, a in by_ivp.trains.items():
        b = direct.trains[key]
        assert (a is None and b is None) or (a.dtype == b.dtype and np.array_equal(a, b)), key
    assert np.array_equal(direct.order, by_ivp.order)
    assert np.array_equal(direct.n_shooting, by_ivp.n_shooting)
    assert (direct.batch, direct.max_pulses, direct.max_shooting) == (by_ivp.batch, by_ivp.max_pulses,
                                                                      by_ivp.max_shooting)
    assert type(direct.ode_solver) is OdeSolver.RK2 and direct.ode_solver.n_integration_steps == 5


def test_from_trains_defaults_and_errors():
    from cocofest_amd import IvpSweep, ModelMaker, OdeSolver

    model = ModelMaker.create_model("ding2007", stim_time=[0.0], sum_stim_truncation=4)
    good = {"stim_time": [0.0, 0.1, 0.2], "final_time": 0.3}
    sweep = IvpSweep.from_trains(model, [good, dict(good, pulse_mode="doublet")])
    assert isinstance(sweep.ode_solver, OdeSolver.RK4) and sweep.ode_solver.n_integration_steps == 10
    # the defaults of IvpFes: the LCM rule after the pulse mode, the model's truncation, pulse_width 0.0003
    assert sweep.n_shooting.tolist() == [3, 60]
    assert np.all(sweep.trains["truncation"] == 4)
    assert np.all(sweep.trains["value"][:3, :] == 0.0003)
    for bad, exc, match in (
            (dict(good, final_time="1"), ValueError, r"trains\[1\]: final_time must be an int or float type"),
            (dict(good, final_time=0), ValueError, r"trains\[1\]: final_time must be positive"),
            (dict(good, n_shooting=0), ValueError, r"trains\[1\]: n_shooting must be a positive int"),
            (dict(good, pulse_mode="quadruplet"), ValueError, r"trains\[1\]: Pulse mode not yet implemented"),
            (dict(good, pulse_mode=2), ValueError, r"trains\[1\]: pulse_mode must be a string type"),
            (dict(good, sum_stim_truncation=0), ValueError, r"trains\[1\]: sum_stim_truncation must be a positive"),
            (dict(good, pulse_width=1e-5), ValueError, r"trains\[1\]: pulse width must be greater than minimum"),
            (dict(good, pulse_width="wide"), TypeError, r"trains\[1\]: pulse_width must be int, float or list"),
            (dict(good, stim_time=[0.2, 0.1]), ValueError, r"trains\[1\]: stim_time must be sorted"),
            (dict(good, stim_time=None), TypeError, r"trains\[1\]: stim_time must be a list"),
            (dict(good, frequency=10), ValueError, r"trains\[1\]: unknown keys \['frequency'\]"),
            ("train", TypeError, r"trains\[1\]: a train must be a dictionary")):
        with pytest.raises(exc, match=match):
            IvpSweep.from_trains(model, [good, bad])
    with pytest.raises(ValueError, match="at least one"):
        IvpSweep.from_trains(model, [])
    with pytest.raises(ValueError, match="COLLOCATION is not supported"):
        IvpSweep.from_trains(model, [good], ode_solver=OdeSolver.COLLOCATION())
    with pytest.raises(TypeError, match="model must be a FesModel"):
        IvpSweep.from_trains("ding2007", [good])
    history = ModelMaker.create_model("ding2003", stim_time=[0.0], sum_stim_truncation=3,
                                      previous_stim={"time": [-0.2, -0.1]})
    with pytest.raises(ValueError, match="previous_stim is not supported"):
        IvpSweep.from_trains(history, [good])
    hmed = ModelMaker.create_model("hmed2018", stim_time=[0.0], sum_stim_truncation=3)
    with pytest.raises(ValueError, match=r"trains\[0\]: Pulse intensity must be greater than minimum"):
        IvpSweep.from_trains(hmed, [dict(good, pulse_intensity=1)])


# ---- TrainSearch ----------------------------------------------------------------------------------------------------
def _search(**kw):
    from cocofest_amd import ModelMaker, OdeSolver, TrainSearch

    model = ModelMaker.create_model("ding2003_with_fatigue", stim_time=[0.0], sum_stim_truncation=5)
    args = dict(final_time=0.5, frequencies=[10, 20, 40], pulse_modes=("single", "doublet"), truncations=[2, 5],
                ode_solver=OdeSolver.RK4(n_integration_steps=2))
    args.update(kw)
    return TrainSearch(model, **args)


def test_train_search_grid():
    from cocofest_amd import IvpSweep, ModelMaker, TrainSearch

    search = _search()
    assert isinstance(search.sweep, IvpSweep) and search.sweep.batch == 12
    # frequencies x pulse_modes x values x truncations, the last fastest
    assert [(c["frequency"], c["pulse_mode"], c["sum_stim_truncation"]) for c in search.candidates] == [
        (f, mode, T) for f in (10, 20, 40) for mode in ("single", "doublet") for T in (2, 5)]
    # the packed instance of candidate i is column j with order[j] == i: 40 Hz doublets are 20 + 20 pulses
    inverse = np.argsort(search.sweep.order)
    assert search.sweep.trains["n_pulses"][inverse].tolist() == [5, 5, 10, 10, 10, 10, 20, 20, 20, 20, 40, 40]
    j = int(inverse[4])  # 20 Hz, single: round(i / 20, 3)
    assert np.array_equal(search.sweep.trains["times"][:10, j], [round(i / 20, 3) for i in range(10)])
    # the LCM rule per candidate: a doublet's second pulse, 5 ms = final_time / 100 later, needs 100 intervals
    assert search.sweep.n_shooting.tolist() == [5, 5, 100, 100, 10, 10, 100, 100, 20, 20, 100, 100]
    # values: one constant width per candidate; refused for a model without one
    ding2007 = ModelMaker.create_model("ding2007", stim_time=[0.0], sum_stim_truncation=3)
    widths = TrainSearch(ding2007, 0.3, [10, 20], values=[0.0003, 0.0005], n_shooting=6)
    assert [(c["frequency"], c["pulse_width"]) for c in widths.candidates] == [(10, 0.0003), (10, 0.0005),
                                                                              (20, 0.0003), (20, 0.0005)]
    assert np.all(widths.sweep.n_shooting == 6)
    k = int(np.argsort(widths.sweep.order)[3])
    assert np.all(widths.sweep.trains["value"][:6, k] == 0.0005)
    with pytest.raises(ValueError, match="has no pulse width or intensity"):
        _search(values=[0.0003])
    with pytest.raises(ValueError, match="frequencies must be positive"):
        _search(frequencies=[10, 0])
    with pytest.raises(ValueError, match=r"candidates\[1\]: pulse width must be greater"):
        TrainSearch(ding2007, 0.3, [10], values=[0.0003, 1e-6])


def _fake_scores(n):
    track = np.array([5.0, 3.0, 9.0, 1.0, 4.0, 2.0, 8.0, 7.0, 6.0, 10.0, 11.0, 12.0][:n])
    return {"Cn": np.zeros(n), "F": np.linspace(10, 120, n), "A": np.linspace(3000, 2900, n),
            "Tau1": np.full(n, 0.05), "Km": np.linspace(0.103, 0.125, n), "track": track,
            "impulse": np.linspace(1, 12, n), "peak": np.linspace(50, 160, n),
            "peak_node": np.arange(n, dtype=np.int64), "end_error": -track, "mean_force": np.linspace(2, 24, n)}


def test_train_search_best_on_an_injected_score(monkeypatch):
    search = _search()
    calls = []

    def fake(target, sample_dt=None, x0=None):
        calls.append((target, sample_dt))
        return _fake_scores(12)

    monkeypatch.setattr(search.sweep, "score", fake)
    with pytest.raises(ValueError, match="run"):
        search.best()
    result = search.run(100.0)
    assert calls == [(100.0, None)]  # one score call per run
    assert result.candidates is search.candidates and np.array_equal(result["track"], _fake_scores(12)["track"])
    best = search.best()
    assert best["index"] == 3 and best["track"] == 1.0 and best["frequency"] == 10 and best["pulse_mode"] == "doublet"
    assert best["sum_stim_truncation"] == 5 and best["peak_node"] == 3 and isinstance(best["peak_node"], int)
    assert result.ranking()[:4].tolist() == [3, 5, 1, 4]
    # candidates 3 and 5 break the Km bound, candidate 1 the peak bound
    km, peak = _fake_scores(12)["Km"], _fake_scores(12)["peak"]
    bounded = search.best(subject_to={"Km": (None, km[2]), "A": (2900.0, None), "peak": (peak[2], None)})
    assert bounded["index"] == 2 and bounded["track"] == 9.0
    assert search.best(metric="impulse")["index"] == 0
    assert search.best(metric="track", subject_to={"Km": (km[4], None)})["index"] == 5
    with pytest.raises(ValueError, match="no candidate satisfies"):
        search.best(subject_to={"Km": (None, 0.05)})
    with pytest.raises(ValueError, match="no candidate satisfies"):
        search.best(subject_to={"peak": (1e3, None), "A": (None, 1e9)})
    with pytest.raises(ValueError, match="unknown key 'Kmm'"):
        search.best(subject_to={"Kmm": (None, 1.0)})
    with pytest.raises(ValueError, match="unknown metric"):
        search.best(metric="cost")
    # a candidate whose metric is not finite is never the best
    scores = _fake_scores(12)
    scores["track"][3] = np.nan
    monkeypatch.setattr(search.sweep, "score", lambda *a, **k: scores)
    assert search.run(100.0).best()["index"] == 5
