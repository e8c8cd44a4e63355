"""Fatigue-parameter identification, host side (no GPU): the C ABI's declarations and argument checks, the
``FesFatigueIdentification`` input checks, its seeded starts, and the exact-AD reference helper's own noise (forward
against reverse mode) on the shapes of the GPU tests."""

import ctypes as C
import re

import numpy as np
import pytest

from tests import cases
from tests.conftest import ROOT

I32P = C.POINTER(C.c_int32)
FATIGUE_MODELS = ["ding2003_with_fatigue", "ding2007_with_fatigue", "hmed2018_with_fatigue"]
KEYS = ["alpha_a", "alpha_tau1", "alpha_km", "tau_fat"]


def _ids(*names):
    from cocofest_amd import _cfx

    a = np.array([_cfx.FATIGUE_PARAM_IDS[n] if isinstance(n, str) else n for n in names], dtype=np.int32)
    return a, a.ctypes.data_as(I32P)


def _model(name, **kw):
    from cocofest_amd import ModelMaker

    return ModelMaker.create_model(name, stim_time=list(cases.TEN_PULSES), sum_stim_truncation=10, **kw)


def test_header_declares_and_library_exports_the_fatigue_identification_calls():
    from cocofest_amd import _cfx

    text = (ROOT / "include" / "cfx.h").read_text()
    lib = _cfx.load_library()
    for fn in ("cfx_idf_forces", "cfx_idf_normal", "cfx_idf_check"):
        assert re.search(r"^int %s\(" % fn, text, re.M), fn
        assert hasattr(lib, fn) and fn in _cfx.SIGNATURES
    assert _cfx.ABI_VERSION == lib.cfx_abi_version() == 12
    assert list(_cfx.FATIGUE_PARAM_IDS) == KEYS
    for key, val in _cfx.FATIGUE_PARAM_IDS.items():
        assert re.search(r"CFX_FP_%s = %d\b" % (key.upper(), val), text), key
    assert int(re.search(r"#define CFX_IDF_MAX_PARAMS (\d+)", text).group(1)) == _cfx.IDF_MAX_PARAMS == 4


@pytest.mark.parametrize("model, n_id, ids, code, msg", [
    ("ding2003_with_fatigue", 0, ["alpha_a"], "EINVAL", "n_id must be in [1, 4]"),
    ("ding2003_with_fatigue", 5, ["alpha_a"] * 5, "EINVAL", "n_id must be in [1, 4]"),
    ("ding2003_with_fatigue", 2, None, "EINVAL", "param_ids is NULL"),
    ("ding2007_with_fatigue", 2, ["alpha_km", "alpha_km"], "EINVAL", "duplicate parameter id 2"),
    ("hmed2018_with_fatigue", 2, ["alpha_a", 4], "EINVAL", "unknown parameter id 4"),
    ("ding2003_with_fatigue", 2, ["alpha_a", -1], "EINVAL", "unknown parameter id -1"),
    ("ding2003", 1, ["alpha_a"], "EUNSUPPORTED", "only available for the fatigue models"),
    ("ding2007", 1, ["tau_fat"], "EUNSUPPORTED", "only available for the fatigue models"),
    ("hmed2018", 1, ["alpha_a"], "EUNSUPPORTED", "only available for the fatigue models"),
    (6, 1, ["alpha_a"], "EINVAL", "unknown model"),
    (-1, 1, ["alpha_a"], "EINVAL", "unknown model"),
])
def test_parameter_list_checks_need_no_device(model, n_id, ids, code, msg):
    """cfx_idf_check runs the parameter-list checks of cfx_idf_forces / cfx_idf_normal for a model id, without a
    handle; the message comes through cfx_last_error(NULL)."""
    from cocofest_amd import _cfx

    lib = _cfx.load_library()
    keep, ptr = (None, None) if ids is None else _ids(*ids)
    mid = _cfx.MODEL_IDS[model] if isinstance(model, str) else model
    assert lib.cfx_idf_check(mid, n_id, ptr) == getattr(_cfx, code)
    assert msg in lib.cfx_last_error(None).decode()
    assert lib.cfx_last_error(None).decode().startswith("cfx_idf: ")


def test_valid_parameter_lists_pass_and_null_handles_are_refused():
    from cocofest_amd import _cfx

    lib = _cfx.load_library()
    for name in FATIGUE_MODELS:
        for keys in (KEYS, KEYS[::-1], ["tau_fat"], ["alpha_km", "alpha_a"]):
            keep, ptr = _ids(*keys)
            assert lib.cfx_idf_check(_cfx.MODEL_IDS[name], len(keys), ptr) == _cfx.OK, (name, keys)
        assert set(KEYS) <= set(_model(name).identifiable_parameters), name
    keep, ptr = _ids("alpha_a")
    buf = np.zeros(8)
    assert lib.cfx_idf_forces(None, 1, ptr, buf.ctypes.data, None, 1, buf.ctypes.data, None, 0) == _cfx.EINVAL
    assert "cfx_idf_forces: NULL handle" in lib.cfx_last_error(None).decode()
    assert lib.cfx_idf_normal(None, 1, ptr, buf.ctypes.data, None, buf.ctypes.data, buf.ctypes.data, 1,
                              buf.ctypes.data, buf.ctypes.data, buf.ctypes.data, 0) == _cfx.EINVAL
    assert "cfx_idf_normal: NULL handle" in lib.cfx_last_error(None).decode()


def test_fes_fatigue_identification_rejects_bad_input():
    from cocofest_amd import FesFatigueIdentification, OdeSolver

    force = [0.0] * 11
    ok = dict(final_time=1.0, force_tracking=force, key_parameter_to_identify=["alpha_a", "tau_fat"])
    d03 = _model("ding2003_with_fatigue")
    with pytest.raises(ValueError, match="should be including the fatigue equation"):
        FesFatigueIdentification(_model("ding2003"), **ok)
    with pytest.raises(TypeError, match="model must be a FesModel type"):
        FesFatigueIdentification(3, **ok)
    with pytest.raises(ValueError, match=re.escape("The given key_parameter_to_identify is not valid, the given value "
                                                   "is a_rest, the available values are ['alpha_a', 'alpha_tau1', "
                                                   "'alpha_km', 'tau_fat']")):
        FesFatigueIdentification(d03, **{**ok, "key_parameter_to_identify": ["alpha_a", "a_rest"]})
    with pytest.raises(TypeError, match="The given key_parameter_to_identify must be list type"):
        FesFatigueIdentification(d03, **{**ok, "key_parameter_to_identify": "alpha_a"})
    with pytest.raises(ValueError, match="every parameter once"):
        FesFatigueIdentification(d03, **{**ok, "key_parameter_to_identify": ["alpha_a", "alpha_a"]})
    with pytest.raises(ValueError, match="every parameter once"):
        FesFatigueIdentification(d03, **{**ok, "key_parameter_to_identify": []})
    with pytest.raises(ValueError, match="expected one per node: n_shooting . 1 = 11"):
        FesFatigueIdentification(d03, **{**ok, "force_tracking": [0.0] * 10})
    with pytest.raises(TypeError, match="force_tracking must be list type, currently force_tracking is"):
        FesFatigueIdentification(d03, **{**ok, "force_tracking": np.zeros(11)})
    with pytest.raises(TypeError, match="force_tracking must be list of int or float type."):
        FesFatigueIdentification(d03, **{**ok, "force_tracking": ["a"] * 11})
    with pytest.raises(TypeError, match="final_time must be int or float type."):
        FesFatigueIdentification(d03, **{**ok, "final_time": "1"})
    with pytest.raises(TypeError, match="ode_solver must be a OdeSolver.RK1, RK2 or RK4 type"):
        FesFatigueIdentification(d03, **ok, ode_solver=OdeSolver.COLLOCATION())
    with pytest.raises(ValueError, match="bounds / initial_guess given for alpha_km, which is not identified"):
        FesFatigueIdentification(d03, **ok, bounds={"alpha_km": (1e-7, 1e-3)})
    with pytest.raises(TypeError, match="pulse_width must be dict type, currently pulse_width is"):
        FesFatigueIdentification(_model("ding2007_with_fatigue"), **ok)
    with pytest.raises(ValueError, match="pulse_width must hold the key 'fixed'"):
        FesFatigueIdentification(_model("ding2007_with_fatigue"), **ok, pulse_width={"fix": 0.0003})
    with pytest.raises(TypeError, match="pulse_intensity must be dict type, currently pulse_intensity is"):
        FesFatigueIdentification(_model("hmed2018_with_fatigue"), **ok, pulse_intensity=50)
    with pytest.raises(ValueError, match="pulse_intensity must hold the key 'fixed'"):
        FesFatigueIdentification(_model("hmed2018_with_fatigue"), **ok, pulse_intensity={})


@pytest.mark.parametrize("name, ctl", [("ding2003_with_fatigue", {}),
                                       ("ding2007_with_fatigue", {"pulse_width": {"fixed": 0.0003}}),
                                       ("hmed2018_with_fatigue", {"pulse_intensity": {"fixed": 50}})])
def test_defaults_starts_and_the_callers_model(name, ctl):
    """Defaults: the model's own value as the guess, 0.01 x .. 100 x around it in increasing order (alpha_a is
    negative).  Starts: seeded, reproducible, inside the bounds, the sign of alpha_a kept.  The caller's model is
    deep-copied and left alone."""
    from cocofest_amd import FesFatigueIdentification

    model = _model(name)
    model.alpha_km = 3.0e-5  # not the literature value: the defaults must follow the model
    own = dict(model.identifiable_parameters)
    before = (list(model.stim_time), dict(model.previous_stim), dict(model.identifiable_parameters))
    ident = FesFatigueIdentification(model, stim_time=[0.0, 0.25, 0.5], final_time=1.0, force_tracking=[0.0] * 5,
                                     key_parameter_to_identify=KEYS, n_starts=9, seed=4, **ctl)
    assert ident.n_shooting == 4 and ident.param_ids == [0, 1, 2, 3] and ident.model is not model
    assert (list(model.stim_time), dict(model.previous_stim), dict(model.identifiable_parameters)) == before
    guess = np.array([own[k] for k in KEYS])
    np.testing.assert_array_equal(ident.initial_guess, guess)
    np.testing.assert_array_equal(ident.lower, np.minimum(0.01 * guess, 100.0 * guess))
    np.testing.assert_array_equal(ident.upper, np.maximum(0.01 * guess, 100.0 * guess))
    assert np.all(ident.lower < ident.upper) and guess[0] < 0 and ident.upper[0] < 0 and guess[2] == 3.0e-5
    th = ident.starts()
    assert th.shape == (4, 9)
    np.testing.assert_array_equal(th[:, 0], guess)
    np.testing.assert_array_equal(th, ident.starts())
    assert np.all(th >= ident.lower[:, None]) and np.all(th <= ident.upper[:, None])
    assert np.all(th[0] < 0) and np.all(th[1:] > 0)
    assert np.all(np.abs(np.log(th / guess[:, None])) <= 0.5 + 1e-12) and len(np.unique(th[0])) == 9
    ident.close()
    # overrides, and a subset of the keys in the caller's order
    sub = FesFatigueIdentification(model, final_time=1.0, force_tracking=[0.0] * 11, n_starts=3, seed=1,
                                   key_parameter_to_identify=["tau_fat", "alpha_a"], bounds={"tau_fat": (50, 300)},
                                   initial_guess={"alpha_a": -0.5}, **ctl)
    assert sub.param_ids == [3, 0] and sub.n_shooting == 10
    np.testing.assert_array_equal(sub.lower, [50, 100.0 * own["alpha_a"]])
    np.testing.assert_array_equal(sub.upper, [300, 0.01 * own["alpha_a"]])
    np.testing.assert_array_equal(sub.starts()[:, 0], [own["tau_fat"], -0.5])
    sub.close()


REF_CASES = [("ding2003_with_fatigue", 10, {}), ("ding2007_with_fatigue", 10, {"pulse_width": 0.0003}),
             ("hmed2018_with_fatigue", 4, {"pulse_intensity": 50})]


@pytest.mark.parametrize("scheme, m", [("RK4", 5), ("RK1", 1)])
@pytest.mark.parametrize("name, T, kw", REF_CASES)
def test_reference_forward_mode_agrees_with_reverse_mode(name, T, kw, scheme, m):
    """The gap between jacfwd and jacrev of the same rollout is the reference's own rounding noise, scaled per column
    by the column's max |S| over the nodes.  Measured on these shapes (N = 10, 6 instances within +-20 % of the
    defaults): <= 6.7e-14, the worst Hmed's tau_fat column; asserted 1e-12.  Every column is nonzero."""
    from tests import fatigue_ident_reference as R

    st = R.FatigueSetup(name, cases.TEN_PULSES, 1.0, 10, T, scheme, m, **kw)
    th = st.defaults(KEYS)[:, None] * (1 + 0.2 * np.random.default_rng(5).uniform(-1, 1, (4, 6)))
    F, S = st.forces_and_sens(KEYS, th)
    F2, S2 = st.forces_and_sens(KEYS, th, mode="rev")
    ef, es = R.scaled_errors(F2, S2, F, S)
    print(f"{name} {scheme} x {m}: reference noise force {ef:.2e} sens {es}")
    assert S.shape == (11, 4, 6) and np.all(np.abs(S).max(axis=(0, 2)) > 0)
    assert np.all(F[0] == 0.0) and np.all(S[0] == 0.0) and np.all(F[-1] > 0)
    assert ef == 0.0 and es.max() < 1e-12


def test_reference_agrees_with_a_central_difference_of_its_trajectory():
    """Central difference with relative step 1e-4 on a subset of the keys in another order: the columns follow the
    caller's keys.  Truncation ~(1e-4)^2 = 1e-8 relative.  Rounding: the tau_fat column is small, |S| ~ 1e-5 against
    |F| ~ 1e2 (127 s of recovery seen through 1 s of data), so 1e-16 |F| / (1e-4 tau_fat |S|) ~ 1e-8 as well;
    asserted 1e-6."""
    from tests import fatigue_ident_reference as R

    st = R.FatigueSetup("ding2007_with_fatigue", cases.TEN_PULSES, 1.0, 10, 10, "RK2", 2, pulse_width=0.0003)
    keys = ["tau_fat", "alpha_a", "alpha_km"]
    th = st.defaults(keys)[:, None] * np.array([[0.9, 1.15]])
    F, S = st.forces_and_sens(keys, th)
    np.testing.assert_array_equal(F, st.forces(keys, th))
    for j in range(len(keys)):
        d = np.zeros_like(th)
        d[j] = 1e-4 * th[j]
        fd = (st.forces(keys, th + d) - st.forces(keys, th - d)) / (2 * d[j])
        err = np.max(np.abs(fd - S[:, j, :])) / np.max(np.abs(S[:, j, :]))
        assert err < 1e-6, (keys[j], err)
