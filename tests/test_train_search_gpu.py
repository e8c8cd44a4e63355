"""cfx_sweep_score / IvpSweep.score / TrainSearch on the GPU: every train of a sweep scored on the device.

The batch (tests/train_search_reference.py::score_cases): the mixed batch of the sweep tests (B = 70, N in {3, 4, 10,
20}, 1..12 pulses) plus an instance with zero pulses, one with n_shooting = 1 and one whose start force exceeds every
later node (peak at node 0): B = 73, two blocks.  Target: 8 samples every 0.1 s, shorter than final_time = 1 and
longer than 0.3 and 0.5.  Reference: the six formulas of include/cfx.h on ``oracle.fes_oracle.ivp_integrate``'s node
forces, reduced with ``math.fsum``.  Errors are scaled as in tests/test_train_search_cpu.py: track by
dt sum (|F_k| + |y_k|)^2, impulse and mean_force by dt sum |F_k|, peak and end_error by max(|F|, |y|); peak_node is
exact.  Tolerance 1e-9, the sweep tests' figure.
"""

import ctypes as C
import functools
import math

import numpy as np
import pytest

from tests import sweep_reference as R
from tests import train_search_reference as S

pytestmark = pytest.mark.gpu

TOL = 1e-9
MODELS = ("ding2003", "ding2003_with_fatigue", "ding2007", "ding2007_with_fatigue", "hmed2018",
          "hmed2018_with_fatigue")
GRID = [(n, s, m) for n in MODELS for s in ("RK1", "RK2", "RK4") for m in (1, 5)]
PEAK_GAP = 1e-6


@functools.lru_cache(maxsize=None)
def _oracle(name, scheme, m):
    """Per case: (node forces, metrics, node targets) by the oracle, computed once."""
    x0 = S.score_x0(name)
    out = []
    for b, case in enumerate(S.score_cases()):
        force = R.oracle_nodes(name, case, scheme, m, x0=x0[b])[1].copy()
        force.setflags(write=False)
        ref, yk = S.metrics_of(force, case["final_time"], S.TARGET_Y, S.TARGET_DT)
        out.append((force, ref, yk))
    return tuple(out)


def _sweep(name, scheme, m, cases=None):
    from cocofest_amd import IvpSweep, ModelMaker, OdeSolver

    model = ModelMaker.create_model(name, stim_time=[0.0], sum_stim_truncation=3)
    cases = S.score_cases() if cases is None else cases
    return IvpSweep.from_trains(model, [S.train_dict(name, c) for c in cases],
                                ode_solver=getattr(OdeSolver, scheme)(n_integration_steps=m))


def test_the_batch_covers_what_it_says():
    sweep = _sweep("ding2003", "RK4", 1)
    assert sweep.batch == 73 and sweep.max_shooting == 20
    inverse = np.argsort(sweep.order)
    n_pulses = sweep.trains["n_pulses"][inverse]
    assert set(sweep.n_shooting[:70].tolist()) == {3, 4, 10, 20} and set(n_pulses[:70].tolist()) == set(range(1, 13))
    assert n_pulses[70] == 0 and sweep.n_shooting[70] == 4
    assert sweep.n_shooting[71] == 1


@pytest.mark.parametrize("name,scheme,m", GRID)
def test_parity_with_the_oracle(name, scheme, m):
    sweep = _sweep(name, scheme, m)
    x0 = S.score_x0(name)
    got = sweep.score(S.TARGET_Y, S.TARGET_DT, x0=x0)
    final = sweep.integrate(x0=x0)
    for key in list(sweep.model.name_dof) + list(S.METRICS):
        assert got[key].shape == (73,)
    assert got["peak_node"].dtype == np.int64
    for nm in sweep.model.name_dof:  # cfx_sweep_integrate's final state, to the bit
        assert np.array_equal(got[nm], final[nm])
    worst = 0.0
    for b, (force, ref, yk) in enumerate(_oracle(name, scheme, m)):
        # a peak_node can differ legitimately only between nodes whose forces agree to rounding: none here (the
        # zero-pulse instance's forces are all exactly zero, where the first node is the answer on both sides)
        assert S.top_two_gap(force) > PEAK_GAP or not np.any(force), (b, force)
        assert got["peak_node"][b] == ref["peak_node"], (b, force)
        scales = S.metric_scales(force, S.score_cases()[b]["final_time"], yk)
        worst = max(worst, S.scaled_metric_error({k: got[k][b] for k in scales}, ref, scales))
    print(f"score parity {name} {scheme} x {m}: {worst:.3e}")
    assert got["peak_node"][72] == 0 and got["peak"][72] == S.START_FORCE  # the start force is the peak
    assert worst <= TOL


@pytest.mark.parametrize("target,sample_dt", [(75.0, None), ((20.0, 60.0), 0.4), (S.TARGET_Y, S.TARGET_DT),
                                              (S.TARGET_Y, 0.25)])
def test_zero_pulse_instance_and_the_target_rule(target, sample_dt):
    """No pulse: F = 0 at every node, so the metrics are the target's own.  n_samples 1, 2 and 8; tables shorter
    (0.4 s, 0.7 s) and longer (1.75 s) than final_time = 1; with N = 4 node 2 (t = 0.5) falls on a sample of the
    0.25 s table."""
    sweep = _sweep("ding2003_with_fatigue", "RK4", 5)
    got = sweep.score(target, sample_dt)
    case = S.score_cases()[70]
    N, tf = case["n_shooting"], case["final_time"]
    y = np.atleast_1d(np.asarray(target, dtype=np.float64))
    yk = S.node_targets(y, 1.0 if sample_dt is None else sample_dt, N, tf)
    exact = (tf / N) * math.fsum(float(v) ** 2 for v in yk)
    print(f"zero-pulse track: {got['track'][70]!r} against {exact!r}")
    assert abs(got["track"][70] - exact) <= 1e-15 * exact
    assert got["peak"][70] == 0.0 and got["peak_node"][70] == 0 and got["impulse"][70] == 0.0
    assert got["mean_force"][70] == 0.0 and got["F"][70] == 0.0
    assert got["end_error"][70] == -yk[N]  # the target rule, to the bit
    # ... and at other node times: the one-interval instance (t = 0.01) and the N = 20, final_time = 0.5 one
    for b in (71, 72):
        c = S.score_cases()[b]
        y_end = S.target_at(y, 1.0 if sample_dt is None else sample_dt, c["n_shooting"] * (c["final_time"] /
                                                                                           c["n_shooting"]))
        assert got["end_error"][b] == got["F"][b] - y_end


@pytest.mark.parametrize("name", ["ding2003", "ding2007_with_fatigue", "hmed2018_with_fatigue"])
def test_metrics_do_not_depend_on_the_position(name):
    """An instance alone, inside the batch and inside the reversed batch: identical bits."""
    cases = list(S.score_cases())
    x0 = S.score_x0(name)
    fwd, rev = _sweep(name, "RK4", 5), _sweep(name, "RK4", 5, cases[::-1])
    assert not np.array_equal(np.argsort(fwd.order), np.argsort(rev.order)[::-1])
    a = fwd.score(S.TARGET_Y, S.TARGET_DT, x0=x0)
    b = rev.score(S.TARGET_Y, S.TARGET_DT, x0=x0[::-1])
    for key in a:
        assert np.array_equal(a[key], b[key][::-1]), key
    for j in (0, 1, 13, 40, 69, 70, 71, 72):
        alone = _sweep(name, "RK4", 5, [cases[j]]).score(S.TARGET_Y, S.TARGET_DT, x0=x0[j])
        for key in a:
            assert alone[key][0] == a[key][j], (key, j)


def test_device_buffers_give_the_host_call_its_bits():
    import torch

    name = "hmed2018_with_fatigue"
    sweep = _sweep(name, "RK4", 5)
    lib = sweep.sweep()
    x0 = np.ascontiguousarray(S.score_x0(name)[sweep.order].T)
    y = np.array(S.TARGET_Y)
    final, metrics = lib.score(sweep.trains, y, S.TARGET_DT, x0=x0)
    assert final.shape == (5, 73) and metrics.shape == (6, 73)
    dev = {k: torch.as_tensor(v).cuda() for k, v in sweep.trains.items()}
    dfinal, dmetrics = lib.score(dev, torch.as_tensor(y).cuda(), S.TARGET_DT, x0=torch.as_tensor(x0).cuda())
    torch.cuda.synchronize()
    assert np.array_equal(dfinal.cpu().numpy(), final)
    assert np.array_equal(dmetrics.cpu().numpy(), metrics)
    plain, _ = lib.integrate(sweep.trains, x0=x0)
    assert np.array_equal(final, plain)
    # the rest state by default
    rest, _ = lib.score(sweep.trains, y, S.TARGET_DT)
    plain_rest, _ = lib.integrate(sweep.trains)
    assert np.array_equal(rest, plain_rest) and not np.array_equal(rest, final)


def test_invalid_inputs_launch_nothing():
    from cocofest_amd import CfxError, _cfx

    sweep = _sweep("ding2007", "RK2", 1)
    lib = sweep.sweep()
    good = np.array(S.TARGET_Y)
    ok_final, ok_metrics = lib.score(sweep.trains, good, S.TARGET_DT)

    def call(trains, y, n_samples, sample_dt, null=None):
        st, keep = _cfx._sweep_trains(trains, sweep.batch, sweep.max_pulses, True)
        tg = _cfx.SweepTarget(None if y is None else y.ctypes.data, n_samples, sample_dt)
        final, metrics = np.full((2, sweep.batch), -7.0), np.full((6, sweep.batch), -7.0)
        rc = lib.lib.cfx_sweep_score(lib.h, C.byref(st), None if null == "target" else C.byref(tg), None,
                                     None if null == "final_state" else final.ctypes.data,
                                     None if null == "metrics" else metrics.ctypes.data, 0, None)
        assert np.all(final == -7.0) and np.all(metrics == -7.0)  # nothing was launched or copied back
        return rc, lib.lib.cfx_sweep_last_error(lib.h).decode()

    nan = good.copy()
    nan[5] = np.nan
    bad_trains = {k: (None if v is None else v.copy()) for k, v in sweep.trains.items()}
    bad_trains["truncation"][3] = 0
    for args, message in (((sweep.trains, nan, 8, 0.1), r"target: y[5] is not finite"),
                          ((sweep.trains, good, 0, 0.1), "n_samples must be >= 1"),
                          ((sweep.trains, good, 8, 0.0), "sample_dt must be positive"),
                          ((sweep.trains, good, 8, -0.1), "sample_dt must be positive"),
                          ((sweep.trains, None, 8, 0.1), "target: y is NULL"),
                          ((bad_trains, good, 8, 0.1), "instance 3: truncation must be >= 1")):
        rc, text = call(*args)
        assert rc == _cfx.EINVAL and message in text and text.startswith("cfx_sweep_score: "), text
    for null in ("target", "final_state", "metrics"):
        rc, text = call(sweep.trains, good, 8, 0.1, null=null)
        assert rc == _cfx.EINVAL and "is NULL" in text
    with pytest.raises(CfxError, match="not finite"):
        lib.score(sweep.trains, nan, 0.1)
    with pytest.raises(CfxError, match="truncation must be >= 1"):
        lib.score(bad_trains, good, 0.1)
    with pytest.raises(ValueError, match="sample_dt must be given"):
        sweep.score(S.TARGET_Y)
    # the handle still works
    final, metrics = lib.score(sweep.trains, good, S.TARGET_DT)
    assert np.array_equal(final, ok_final) and np.array_equal(metrics, ok_metrics)


def test_train_search_end_to_end():
    """Ding2003 + fatigue, {10, 20, 40} Hz x {single, doublet}, final_time 0.5, RK4 x 2, a constant target: the
    ranking is that of the node trajectories of IvpSweep.integrate(nodes=True) reduced in numpy."""
    from cocofest_amd import ModelMaker, OdeSolver, TrainSearch

    model = ModelMaker.create_model("ding2003_with_fatigue", stim_time=[0.0], sum_stim_truncation=10)
    search = TrainSearch(model, final_time=0.5, frequencies=[10, 20, 40], pulse_modes=("single", "doublet"),
                         ode_solver=OdeSolver.RK4(n_integration_steps=2))
    target = 100.0
    result = search.run(target)
    nodes = search.sweep.integrate(nodes=True)
    ref = []
    for b, N in enumerate(nodes["n_shooting"]):
        ref.append(S.metrics_of(nodes["F"][b, : N + 1], 0.5, [target], 1.0)[0])
    cost = np.array([r["track"] for r in ref])
    order = np.argsort(cost, kind="stable")
    gaps = np.diff(cost[order]) / cost[order][1:]
    assert np.all(gaps > 1e-6), cost[order]  # the reference ranking is not a matter of rounding
    assert result.ranking("track").tolist() == order.tolist()
    best = search.best()
    assert best["index"] == order[0] and best["frequency"] == search.candidates[order[0]]["frequency"]
    # the same node forces on both sides; the device sums up to 101 terms of one sign sequentially, at most
    # 101 x 2^-53 = 1.1e-14 relative away from fsum: held to 1e-12
    for key in ("track", "impulse", "peak", "end_error", "mean_force"):
        want = np.array([r[key] for r in ref])
        assert np.allclose(result[key], want, rtol=1e-12, atol=1e-12 * np.abs(want).max()), key
    assert np.array_equal(result["peak_node"], [r["peak_node"] for r in ref])
    # a bound on the final fatigue state removes the best candidates of the unconstrained ranking
    km = np.sort(result["Km"])
    bounded = search.best(subject_to={"Km": (None, km[2])})
    assert result["Km"][bounded["index"]] <= km[2]
    with pytest.raises(ValueError, match="no candidate satisfies"):
        search.best(subject_to={"Km": (None, 0.0)})
