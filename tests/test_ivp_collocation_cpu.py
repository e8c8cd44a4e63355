"""Host-side checks of the implicit collocation integrator: the CPU reference helper the GPU tests compare with
(tests/colloc_ivp_reference.py) against an independent solver, its own noise, and the additive C ABI."""

import ctypes as C
import re

import numpy as np
import pytest
from scipy.optimize import fsolve

from oracle import fes_collocation as CO
from oracle import fes_oracle as O
from tests import colloc_ivp_reference as R
from tests.conftest import ROOT


@pytest.mark.parametrize("method", ["legendre", "radau"])
def test_helper_reproduces_the_fsolve_trajectory(method):
    """The problem of test_collocation_oracle's convergence test (Ding2003 from rest, 5 pulses, N = 20), degree 3:
    MINPACK's hybrid solver with a finite-difference Jacobian, interval by interval, against the helper's Newton."""
    d = 3
    pb = R.col_problem("ding2003", [0.0, 0.1, 0.2, 0.3, 0.4], 0.5, 4, 20, d, method)
    tau, Cm, D = CO.coefficients(d, method)
    x = np.zeros(2)
    samples = []
    for k in range(pb.n_shooting):
        def residual(z, k=k, x=x):
            XC = np.concatenate([x, z]).reshape(d + 1, 2)
            out = []
            for j in range(1, d + 1):
                t = k * pb.dt + tau[j] * pb.dt
                f = O.rhs("ding2003", pb.c, t, XC[j][:, None], None, pb.rows[k][:, None])[:, 0]
                out.append(Cm[:, j] @ XC - pb.dt * f)
            return np.concatenate(out)

        z = fsolve(residual, np.tile(x, d), xtol=1e-14)
        XC = np.concatenate([x, z]).reshape(d + 1, 2)
        samples.append(XC)
        x = D @ XC
    want = np.concatenate(samples + [x[None, :]])[None]
    got, conv = R.integrate(pb, np.zeros((1, 2)), np.zeros((1, pb.n_shooting, 0)), "copy")
    assert conv.all()
    assert got.shape == (1, pb.n_shooting * (d + 1) + 1, 2)
    err = R.scaled_error(got, want)
    print(f"helper vs fsolve ({method}): {err:.3e}")
    assert err <= 1e-11  # fsolve stops at a relative step of 1e-14; both sides solve the same rows


@pytest.mark.parametrize("name, method, degree, n", [("ding2003", "legendre", 4, 10),
                                                    ("ding2007_with_fatigue", "radau", 5, 10),
                                                    ("hmed2018_with_fatigue", "legendre", 9, 20)])
def test_helper_noise_between_two_newton_starts(name, method, degree, n):
    """eps_ref: the node-copy start and the explicit-Euler predictor reach the same trajectory to rounding on the
    GPU tests' own inputs, and every instance converges."""
    pb, X0, U, traj, conv, eps = R.reference(name, method, degree, n)
    print(f"eps_ref {name} {method} d={degree} N={n}: {eps:.3e}")
    assert conv.all()
    assert traj.shape == (R.B_MAX, n * (degree + 1) + 1, pb.nx)
    assert eps <= 1e-12


def test_integrate_status_is_declared_exported_and_bound():
    from cocofest_amd import _cfx

    text = (ROOT / "include" / "cfx.h").read_text()
    assert re.search(r"^int cfx_integrate_status\(cfx_handle \*h, int32_t \*status, uint32_t flags\);", text, re.M)
    assert "cfx_integrate is not available" not in text
    lib = _cfx.load_library()
    assert hasattr(lib, "cfx_integrate_status")
    assert "cfx_integrate_status" in _cfx.SIGNATURES
    assert lib.cfx_abi_version() == 12 == _cfx.ABI_VERSION


def test_integrate_status_null_arguments_are_einval_with_a_message():
    from cocofest_amd import _cfx

    lib = _cfx.load_library()
    status = np.zeros(1, dtype=np.int32)
    assert lib.cfx_integrate_status(None, status.ctypes.data, 0) == _cfx.EINVAL
    assert b"cfx_integrate_status" in lib.cfx_last_error(None)
    assert lib.cfx_collocation_points(None, status.ctypes.data_as(C.POINTER(C.c_double))) == _cfx.EINVAL


def test_msk_create_still_refuses_collocation_schemes():
    """The musculoskeletal transcription stays explicit: cfx_msk_create refuses schemes 16 / 17 before any HIP call,
    and OcpFesMsk refuses OdeSolver.COLLOCATION."""
    import cocofest_amd as CA
    from cocofest_amd import _cfx
    from tests import msk_cases as MC

    lib = _cfx.load_library()
    for scheme in (_cfx.COLLOCATION_LEGENDRE, _cfx.COLLOCATION_RADAU):
        mp = _cfx.MskProblem()
        mp.abi_version, mp.scheme, mp.n_steps, mp.n_shooting = _cfx.ABI_VERSION, scheme, 4, 10
        mp.truncation, mp.layout, mp.batch, mp.final_time = 10, _cfx.LAYOUT_SOA, 1, 1.0
        out = C.c_void_p()
        assert lib.cfx_msk_create(C.byref(mp), C.byref(out)) == _cfx.EUNSUPPORTED and not out.value
        assert "scheme must be" in lib.cfx_last_error(None).decode()
    model = MC.product_ocp(**MC.cfg5()).model
    with pytest.raises(NotImplementedError):
        CA.OcpFesMsk.prepare_ocp(model=model, final_time=1, objective={}, ode_solver=CA.OdeSolver.COLLOCATION(4),
                                 msk_info={"bound_type": "start_end", "bound_data": [[0, 5], [0, 90]],
                                           "with_residual_torque": False})
