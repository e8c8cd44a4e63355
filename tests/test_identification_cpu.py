"""Force-parameter identification, host side (no GPU): the C ABI's declarations and argument checks, the
``FesIdentification`` input checks with the reference's messages, and the exact-AD reference helper's own accuracy
(forward against reverse mode: the reference noise; against a central difference of its own trajectory)."""

import ctypes as C
import re

import numpy as np
import pytest

from tests import cases
from tests.conftest import ROOT

I32P = C.POINTER(C.c_int32)


def _ids(*names):
    from cocofest_amd import _cfx

    a = np.array([_cfx.PARAM_IDS[n] if isinstance(n, str) else n for n in names], dtype=np.int32)
    return a, a.ctypes.data_as(I32P)


def test_header_declares_and_library_exports_the_identification_calls():
    from cocofest_amd import _cfx

    text = (ROOT / "include" / "cfx.h").read_text()
    lib = _cfx.load_library()
    for fn in ("cfx_id_forces", "cfx_id_normal", "cfx_id_check"):
        assert re.search(r"^int %s\(" % fn, text, re.M), fn
        assert hasattr(lib, fn) and fn in _cfx.SIGNATURES
    assert _cfx.ABI_VERSION == lib.cfx_abi_version() == 12
    assert int(re.search(r"#define CFX_ABI_VERSION (\d+)", text).group(1)) == 12
    # the parameter ids of the header and of the binding agree
    for key, val in _cfx.PARAM_IDS.items():
        assert re.search(r"CFX_P_%s = %d\b" % (key.upper(), val), text), key


@pytest.mark.parametrize("model, n_id, ids, code, msg", [
    ("ding2003", 0, ["a_rest"], "EINVAL", "n_id must be in [1, 8]"),
    ("ding2003", 9, ["a_rest"] * 9, "EINVAL", "n_id must be in [1, 8]"),
    ("ding2003", 2, None, "EINVAL", "param_ids is NULL"),
    ("ding2003", 2, ["a_rest", "a_rest"], "EINVAL", "duplicate parameter id 0"),
    ("ding2003", 2, ["a_rest", 11], "EINVAL", "unknown parameter id 11"),
    ("ding2003", 2, ["a_rest", -1], "EINVAL", "unknown parameter id -1"),
    ("ding2003", 2, ["a_rest", "pd0"], "EINVAL", "parameter id 5 is not a parameter of model 0"),
    ("ding2003", 1, ["a_scale"], "EINVAL", "parameter id 4 is not a parameter of model 0"),
    ("ding2007", 1, ["a_rest"], "EINVAL", "parameter id 0 is not a parameter of model 2"),
    ("ding2007", 1, ["cr"], "EINVAL", "parameter id 10 is not a parameter of model 2"),
    ("hmed2018", 1, ["pdt"], "EINVAL", "parameter id 6 is not a parameter of model 4"),
    ("ding2003_with_fatigue", 1, ["a_rest"], "EUNSUPPORTED", "not available for the fatigue models"),
    ("hmed2018_with_fatigue", 1, ["a_rest"], "EUNSUPPORTED", "not available for the fatigue models"),
    (7, 1, ["a_rest"], "EINVAL", "unknown model"),
])
def test_parameter_list_checks_need_no_device(model, n_id, ids, code, msg):
    """cfx_id_check runs the parameter-list checks of cfx_id_forces / cfx_id_normal for a model id, without a handle
    (a handle needs a device); the message comes through cfx_last_error(NULL)."""
    from cocofest_amd import _cfx

    lib = _cfx.load_library()
    keep, ptr = (None, None) if ids is None else _ids(*ids)
    mid = _cfx.MODEL_IDS[model] if isinstance(model, str) else model
    assert lib.cfx_id_check(mid, n_id, ptr) == getattr(_cfx, code)
    assert msg in lib.cfx_last_error(None).decode()


def test_valid_parameter_lists_pass_and_null_handles_are_refused():
    from cocofest_amd import _cfx
    from tests.ident_reference import FULL_KEYS

    lib = _cfx.load_library()
    for name, keys in FULL_KEYS.items():
        keep, ptr = _ids(*keys)
        assert lib.cfx_id_check(_cfx.MODEL_IDS[name], len(keys), ptr) == _cfx.OK, name
        assert set(keys) == set(cases_model(name).identifiable_parameters), name
    keep, ptr = _ids("a_rest")
    buf = np.zeros(8)
    assert lib.cfx_id_forces(None, 1, ptr, buf.ctypes.data, None, 1, buf.ctypes.data, None, 0) == _cfx.EINVAL
    assert "cfx_id_forces: NULL handle" in lib.cfx_last_error(None).decode()
    assert lib.cfx_id_normal(None, 1, ptr, buf.ctypes.data, None, buf.ctypes.data, buf.ctypes.data, 1,
                             buf.ctypes.data, buf.ctypes.data, buf.ctypes.data, 0) == _cfx.EINVAL
    assert "cfx_id_normal: NULL handle" in lib.cfx_last_error(None).decode()


def cases_model(name, **kw):
    from cocofest_amd import ModelMaker

    return ModelMaker.create_model(name, stim_time=list(cases.TEN_PULSES), sum_stim_truncation=10, **kw)


def test_fes_identification_rejects_bad_input_with_the_reference_messages():
    from cocofest_amd import CfxError, FesIdentification, OdeSolver

    force = [0.0] * 11
    ok = dict(final_time=1.0, force_tracking=force, key_parameter_to_identify=["a_rest", "km_rest"])
    d03 = cases_model("ding2003")
    with pytest.raises(ValueError, match=re.escape("The given key_parameter_to_identify is not valid, the given value "
                                                   "is pd0, the available values are ['a_rest', 'km_rest', "
                                                   "'tau1_rest', 'tau2']")):
        FesIdentification(d03, **{**ok, "key_parameter_to_identify": ["a_rest", "pd0"]})
    with pytest.raises(TypeError, match="The given key_parameter_to_identify must be list type"):
        FesIdentification(d03, **{**ok, "key_parameter_to_identify": "a_rest"})
    with pytest.raises(ValueError, match="every parameter once"):
        FesIdentification(d03, **{**ok, "key_parameter_to_identify": ["a_rest", "a_rest"]})
    with pytest.raises(ValueError, match="should not be including the fatigue equation"):
        FesIdentification(cases_model("ding2003_with_fatigue"), **ok)
    with pytest.raises(TypeError, match="force_tracking must be list type, currently force_tracking is"):
        FesIdentification(d03, **{**ok, "force_tracking": np.zeros(11)})
    with pytest.raises(TypeError, match="force_tracking must be list of int or float type."):
        FesIdentification(d03, **{**ok, "force_tracking": ["a"] * 11})
    with pytest.raises(TypeError, match="final_time must be int or float type."):
        FesIdentification(d03, **{**ok, "final_time": "1"})
    with pytest.raises(ValueError, match="expected one per node: n_shooting . 1 = 11"):
        FesIdentification(d03, **{**ok, "force_tracking": [0.0] * 10})
    with pytest.raises(TypeError, match="pulse_width must be dict type, currently pulse_width is"):
        FesIdentification(cases_model("ding2007"), final_time=1.0, force_tracking=force,
                          key_parameter_to_identify=["a_scale"])
    with pytest.raises(TypeError, match="pulse_intensity must be dict type, currently pulse_intensity is"):
        FesIdentification(cases_model("hmed2018"), final_time=1.0, force_tracking=force,
                          key_parameter_to_identify=["ar"], pulse_intensity=50)
    with pytest.raises(ValueError, match="fixed pulse_intensity must be a int, float or list type."):
        FesIdentification(cases_model("hmed2018"), final_time=1.0, force_tracking=force,
                          key_parameter_to_identify=["ar"], pulse_intensity={"fixed": "50"})
    with pytest.raises(TypeError, match="model must be a FesModel type"):
        FesIdentification(3, **ok)
    with pytest.raises(TypeError, match="ode_solver must be a OdeSolver.RK1, RK2 or RK4 type"):
        FesIdentification(d03, **ok, ode_solver=OdeSolver.COLLOCATION())
    # a well-formed problem is set up on the host alone: grid, defaults, seeded starts inside the bounds
    ident = FesIdentification(cases_model("ding2007"), final_time=1.0, force_tracking=force, n_starts=5, seed=3,
                              key_parameter_to_identify=["a_scale", "pd0"], pulse_width={"fixed": 0.0003},
                              bounds={"pd0": (5e-5, 3e-4)})
    assert ident.n_shooting == 10 and ident.param_ids == [4, 5]
    th = ident.starts()
    assert th.shape == (2, 5) and th[0, 0] == 5000 and th[1, 0] == 1e-4
    assert np.all(th >= ident.lower[:, None]) and np.all(th <= ident.upper[:, None])
    np.testing.assert_array_equal(th, ident.starts())
    np.testing.assert_array_equal(ident.lower, [1, 5e-5])
    assert isinstance(CfxError(0, ""), RuntimeError)


REF_CASES = [("ding2003", 10, {}), ("ding2007", 10, {"pulse_width": 0.0003}), ("hmed2018", 4, {"pulse_intensity": 50})]


@pytest.mark.parametrize("name, T, kw", REF_CASES)
def test_reference_forward_mode_agrees_with_reverse_mode(name, T, kw):
    """The gap between jacfwd and jacrev of the same rollout is the reference's own rounding noise.  Measured
    (RK4 x 5, N = 10, 6 instances within +-20 % of the defaults): <= 4e-15 scaled, every model; asserted 1e-12."""
    from tests import ident_reference as R

    st = R.Setup(name, cases.TEN_PULSES, 1.0, 10, T, "RK4", 5, **kw)
    keys = R.FULL_KEYS[name]
    th = st.defaults(keys)[:, None] * (1 + 0.2 * np.random.default_rng(5).uniform(-1, 1, (len(keys), 6)))
    F, S = st.forces_and_sens(keys, th)
    F2, S2 = st.forces_and_sens(keys, th, mode="rev")
    ef, es = R.scaled_errors(F2, S2, F, S)
    print(f"{name}: reference noise force {ef:.2e} sens {es.max():.2e}")
    assert S.shape == (11, len(keys), 6) and np.all(np.abs(S).max(axis=(0, 2)) > 0)
    assert ef == 0.0 and es.max() < 1e-12


@pytest.mark.parametrize("name, T, kw", REF_CASES)
def test_reference_agrees_with_a_central_difference_of_its_trajectory(name, T, kw):
    """Central difference with relative step 1e-6: truncation ~1e-12 relative, rounding ~1e-16 / 1e-6 = 1e-10."""
    from tests import ident_reference as R

    st = R.Setup(name, cases.TEN_PULSES, 1.0, 10, T, "RK2", 2, **kw)
    keys = R.FULL_KEYS[name]
    th = st.defaults(keys)[:, None] * np.array([[0.9, 1.15]])
    F, S = st.forces_and_sens(keys, th)
    np.testing.assert_array_equal(F, st.forces(keys, th))
    for j in range(len(keys)):
        d = np.zeros_like(th)
        d[j] = 1e-6 * th[j]
        fd = (st.forces(keys, th + d) - st.forces(keys, th - d)) / (2 * d[j])
        err = np.max(np.abs(fd - S[:, j, :])) / np.max(np.abs(S[:, j, :]))
        assert err < 1e-8, (keys[j], err)


def _exp_fit_normal(sign=1.0):
    """Normal equations of fitting y = a exp(-b t) at 12 nodes, in cfx_id_normal's layout (cost (B,), grad (2, B),
    packed lower triangle (3, B)); ``sign`` flips the gradient (a broken kernel)."""
    import torch

    t = torch.linspace(0, 1, 12, dtype=torch.float64)[:, None]
    y = 3.0 * torch.exp(-2.0 * t)

    def normal(theta):
        a, b = theta[0][None, :], theta[1][None, :]
        e = torch.exp(-b * t)
        r = a * e - y
        S = torch.stack([e, -a * t * e])  # (2, K, B)
        cost = (r * r).sum(dim=0)
        grad = sign * 2 * (S * r[None]).sum(dim=1)
        H = 2 * torch.einsum("ikb,jkb->ijb", S, S)
        return cost, grad, torch.stack([H[0, 0], H[1, 0], H[1, 1]])

    return normal


def test_lm_solve_converges_on_the_gradient_test_and_reports_a_stall():
    """The product's Levenberg-Marquardt on an analytic two-parameter fit (CPU tensors): from starts away from the
    solution every instance stops on the projected-gradient test at the generating values; with the gradient's sign
    flipped no trial can be accepted, and every instance must end STALLED at its start, not as converged."""
    import torch

    from cocofest_amd.identification import CONVERGED_GRADIENT, STALLED, lm_solve

    rng = np.random.default_rng(2)
    th0 = torch.as_tensor(np.array([[3.0], [2.0]]) * np.exp(0.5 * rng.uniform(-1, 1, (2, 16))))
    lo, hi = torch.full_like(th0, 0.01), torch.full_like(th0, 100.0)
    theta, c, iters, status, hist = lm_solve(_exp_fit_normal(), th0, lo, hi)
    assert torch.all(status == CONVERGED_GRADIENT) and torch.all(iters >= 1)
    np.testing.assert_allclose(theta.numpy(), np.repeat([[3.0], [2.0]], 16, 1), rtol=1e-6)
    assert torch.all(hist[1:] <= hist[:-1]) and torch.all(c < 1e-12 * hist[0])
    theta, c, iters, status, hist = lm_solve(_exp_fit_normal(sign=-1.0), th0, lo, hi)
    assert torch.all(status == STALLED), status
    assert torch.equal(theta, th0) and torch.all(c == hist[0])
    # a start at a bound with the gradient pointing outwards stays there and converges on the free parameter
    lo2 = lo.clone()
    lo2[1] = 2.5
    th1 = th0.clone()
    th1[1] = 2.5
    theta, c, iters, status, hist = lm_solve(_exp_fit_normal(), th1, lo2, hi)
    assert torch.all(status > 0) and torch.all(status != STALLED) and torch.all(theta[1] == 2.5)


def test_fes_identification_leaves_the_model_alone_and_names_a_missing_key():
    from cocofest_amd import FesIdentification

    model = cases_model("ding2007")
    before = (list(model.stim_time), dict(model.previous_stim), model.pulse_width)
    with pytest.raises(ValueError, match="pulse_width must hold the key 'fixed'"):
        FesIdentification(model, final_time=1.0, force_tracking=[0.0] * 11, key_parameter_to_identify=["a_scale"],
                          pulse_width={"fix": 0.0003})
    with pytest.raises(ValueError, match="pulse_intensity must hold the key 'fixed'"):
        FesIdentification(cases_model("hmed2018"), final_time=1.0, force_tracking=[0.0] * 11,
                          key_parameter_to_identify=["ar"], pulse_intensity={})
    ident = FesIdentification(model, stim_time=[0.0, 0.5], final_time=1.0, force_tracking=[0.0] * 3,
                              key_parameter_to_identify=["a_scale"], pulse_width={"fixed": 0.0003})
    assert ident.n_shooting == 2 and ident.model is not model
    assert (list(model.stim_time), dict(model.previous_stim), model.pulse_width) == before
