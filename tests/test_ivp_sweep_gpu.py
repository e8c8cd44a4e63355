"""IvpSweep on the GPU: every instance of a batch carries its own stimulation train (cfx_sweep_integrate).

The mixed batch (tests/sweep_reference.py::mixed_cases): B = 70, one full wave plus a partial one, N in {3, 4, 10,
20}, 1..12 pulses, truncation 1..12, final_time in {0.3, 0.5, 1}, single / doublet / triplet trains, per-pulse widths
and intensities.  Reference: ``oracle.fes_oracle.ivp_integrate`` per case, computed once per (model, scheme, m).
Tolerance 1e-9 on errors scaled per instance and state by the largest magnitude over the nodes, the figure of
tests/test_identification_gpu.py.  Largest measured error on MI355X: 2.5e-11 (ding2003_with_fatigue, RK2 x 1).  The
CPU restatement (tests/test_ivp_sweep_cpu.py) shows errors of that size on the trains with N = 3 or 4, whose coarse
steps carry a calcium stage value across -Km: the force row is singular there and rounding differences are amplified;
the table per model and scheme is in DESIGN section 7c.
"""

import ctypes as C
import functools

import numpy as np
import pytest

from tests import sweep_reference as R

pytestmark = pytest.mark.gpu

TOL = 1e-9
MODELS = ("ding2003", "ding2003_with_fatigue", "ding2007", "ding2007_with_fatigue", "hmed2018",
          "hmed2018_with_fatigue")
GRID = [(n, s, m) for n in MODELS for s in ("RK1", "RK2", "RK4") for m in (1, 5)]


@functools.lru_cache(maxsize=None)
def _oracle(name, scheme, m):
    """Node states (nx, N_b + 1) of every case of the mixed batch, computed once."""
    out = tuple(R.oracle_nodes(name, case, scheme, m) for case in R.mixed_cases())
    for a in out:
        a.setflags(write=False)
    return out


def _sweep(name, scheme, m, cases=None):
    from cocofest_amd import IvpSweep

    return IvpSweep([R.make_ivp(name, case, scheme, m) for case in (R.mixed_cases() if cases is None else cases)])


def _nodes_of(result, names, b):
    """(nx, N_b + 1) node states of instance b and the (nx, rest) entries past its own n_shooting."""
    n = int(result["n_shooting"][b])
    full = np.stack([result[name][b] for name in names])
    return full[:, : n + 1], full[:, n + 1:]


@pytest.mark.parametrize("name,scheme,m", GRID)
def test_parity_with_the_oracle(name, scheme, m):
    sweep = _sweep(name, scheme, m)
    names = sweep.model.name_dof
    nodes, final = sweep.integrate(nodes=True), sweep.integrate()
    ref = _oracle(name, scheme, m)
    assert nodes[names[0]].shape == (70, 21)
    worst = 0.0
    for b, r in enumerate(ref):
        got, past = _nodes_of(nodes, names, b)
        assert got.shape == r.shape and np.all(np.isnan(past))
        worst = max(worst, R.scaled_error(got, r))
        # the final state of the plain call is the last node's, to the bit
        assert np.array_equal(np.array([final[nm][b] for nm in names]), got[:, -1])
    print(f"sweep parity {name} {scheme} x {m}: {worst:.3e}")
    assert worst <= TOL


def test_beyond_the_old_truncation_limit():
    """40 pulses, truncation 40, N = 40: cfx_create stops at truncation 32."""
    from cocofest_amd import CfxError, IvpSweep

    name = "ding2003_with_fatigue"
    case = {"stim_time": [round(i * 0.025, 3) for i in range(40)], "pulse_mode": "single", "truncation": 40,
            "n_shooting": 40, "final_time": 1.0, "varying": True, "seed": 1}
    ivp = R.make_ivp(name, case, "RK4", 2)
    with pytest.raises(CfxError, match=r"truncation must be in \[1, 32\]"):
        ivp.handle(batch=1)
    res = IvpSweep([ivp]).integrate(nodes=True)
    got, _ = _nodes_of(res, ivp.model.name_dof, 0)
    err = R.scaled_error(got, R.oracle_nodes(name, case, "RK4", 2))
    print(f"sweep truncation 40: {err:.3e}")
    assert err <= TOL


@pytest.mark.parametrize("name", ["ding2003_with_fatigue", "ding2007", "hmed2018"])
def test_agreement_with_ivpfes_integrate(name):
    m = 5
    picks = list(range(6)) + [9, 17, 28, 36, 51, 69]
    cases = [R.mixed_cases()[i] for i in picks]
    assert all(c["truncation"] <= 32 for c in cases)
    sweep = _sweep(name, "RK4", m, cases)
    names = sweep.model.name_dof
    res = sweep.integrate(nodes=True)
    worst = 0.0
    for b, case in enumerate(cases):
        ivp = R.make_ivp(name, case, "RK4", m)
        single = ivp.integrate(return_time=False)
        ivp.close()
        ref = np.stack([single[nm][0, ::m] for nm in names])
        got, _ = _nodes_of(res, names, b)
        worst = max(worst, R.scaled_error(got, ref))
    print(f"sweep against IvpFes.integrate {name}: {worst:.3e}")
    assert worst <= TOL


@pytest.mark.parametrize("name", ["ding2003", "ding2007_with_fatigue", "hmed2018_with_fatigue"])
def test_position_independence(name):
    """An instance alone, inside the batch and inside the reversed batch: identical bits."""
    cases = list(R.mixed_cases())
    fwd = _sweep(name, "RK4", 5)
    rev = _sweep(name, "RK4", 5, cases[::-1])
    # the packed position of case j really differs between the two batches
    assert not np.array_equal(np.argsort(fwd.order), np.argsort(rev.order)[::-1])
    a, b = fwd.integrate(nodes=True), rev.integrate(nodes=True)
    names = fwd.model.name_dof
    for nm in names:
        assert np.array_equal(a[nm], b[nm][::-1], equal_nan=True)
    for j in (0, 1, 13, 40, 69):
        alone = _sweep(name, "RK4", 5, [cases[j]]).integrate(nodes=True)
        n = int(alone["n_shooting"][0])
        assert n == a["n_shooting"][j]
        for nm in names:
            assert np.array_equal(alone[nm][0], a[nm][j, : n + 1])


def test_device_buffers_and_start_state():
    import torch

    name = "hmed2018_with_fatigue"
    sweep = _sweep(name, "RK4", 5)
    lib = sweep.sweep()
    final, nodes = lib.integrate(sweep.trains, nodes=True)
    dev = {k: torch.as_tensor(v).cuda() for k, v in sweep.trains.items()}
    dfinal, dnodes = lib.integrate(dev, nodes=True)
    torch.cuda.synchronize()
    assert np.array_equal(dfinal.cpu().numpy(), final)
    assert np.array_equal(dnodes.cpu().numpy(), nodes, equal_nan=True)
    # start state: the rest state given explicitly is the default; another one changes the result
    rest = sweep.model.standard_rest_values()[:, 0].astype(float)
    base = sweep.integrate()
    same = sweep.integrate(x0=rest)
    other_x0 = np.tile(rest, (70, 1))
    other_x0[:, 1] = 25.0
    other_x0[5, 2] *= 0.9
    other = sweep.integrate(x0=other_x0, nodes=True)
    for nm in sweep.model.name_dof:
        assert np.array_equal(base[nm], same[nm])
    assert np.all(other["F"][:, 0] == 25.0) and other["A"][5, 0] == other_x0[5, 2]
    assert np.all(other["F"][np.arange(70), other["n_shooting"]] != base["F"])
    dx0 = torch.as_tensor(np.ascontiguousarray(other_x0[sweep.order].T)).cuda()
    dfinal2, _ = lib.integrate(dev, x0=dx0)
    torch.cuda.synchronize()
    inverse = np.argsort(sweep.order)
    assert np.array_equal(dfinal2.cpu().numpy()[1][inverse], other["F"][np.arange(70), other["n_shooting"]])


def test_the_study_in_miniature():
    """n_stim in {1, 2, 4, 5} x truncation 1..n_stim x three modes in one launch; the doublet and triplet trains of
    n_stim 4 and 5 reach N = 200 by the LCM rule."""
    from cocofest_amd import IvpSweep

    name = "ding2003_with_fatigue"
    cases = [{"stim_time": [round(i / n, 3) for i in range(n)], "pulse_mode": mode, "truncation": T,
              "n_shooting": None, "final_time": 1, "varying": True, "seed": 1}
             for mode in ("single", "doublet", "triplet") for n in (1, 2, 4, 5) for T in range(1, n + 1)]
    assert len(cases) == 36
    sweep = IvpSweep([R.make_ivp(name, c, "RK4", 2) for c in cases])
    assert sweep.max_shooting == 200 and sweep.max_pulses == 15
    res = sweep.integrate()
    worst = 0.0
    for b, case in enumerate(cases):
        ref = R.oracle_nodes(name, case, "RK4", 2)
        scale = np.max(np.abs(ref), axis=1)
        got = np.array([res[nm][b] for nm in ("Cn", "F", "A", "Tau1", "Km")])
        worst = max(worst, float(np.max(np.abs(got - ref[:, -1]) / scale)))
    print(f"sweep study in miniature: {worst:.3e}")
    assert worst <= TOL


def test_invalid_host_arrays_launch_nothing():
    from cocofest_amd import CfxError, _cfx

    sweep = _sweep("ding2007", "RK2", 1)
    lib = sweep.sweep()
    good, _ = lib.integrate(sweep.trains)
    for key, row, value, message in (("times", 1, -1.0, "time decreases"), ("act_node", 0, 21, "past n_shooting"),
                                     ("truncation", None, 0, "truncation must be >= 1"),
                                     ("n_pulses", None, 13, "n_pulses must be in"),
                                     ("n_shooting", None, 21, "n_shooting must be in")):
        bad = {k: (None if v is None else v.copy()) for k, v in sweep.trains.items()}
        if row is None:
            bad[key][3] = value
        else:
            bad[key][row, 0] = value  # instance 0 is the heaviest: it has more than one pulse
        st, keep = _cfx._sweep_trains(bad, sweep.batch, sweep.max_pulses, True)
        final = np.full((2, sweep.batch), -7.0)
        rc = lib.lib.cfx_sweep_integrate(lib.h, C.byref(st), None, final.ctypes.data, None, 0, None)
        assert rc == _cfx.EINVAL
        assert message in lib.lib.cfx_sweep_last_error(lib.h).decode()
        assert np.all(final == -7.0)  # nothing was launched or copied back
        with pytest.raises(CfxError, match=message):
            lib.integrate(bad)
    # the handle still works, and so does a new one after it is destroyed
    again, _ = lib.integrate(sweep.trains)
    assert np.array_equal(again, good)
    sweep.close()
    assert sweep._sweep is None
    res = sweep.integrate()
    assert np.array_equal(res["F"][sweep.order], good[1])
