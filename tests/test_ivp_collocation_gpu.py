"""The implicit collocation integrator on the GPU (cfx_integrate on a collocation handle, IvpFes with
OdeSolver.COLLOCATION, FesOcp.integrated_guess) against the CPU reference helper (tests/colloc_ivp_reference.py: a
full Newton on all d nx unknowns of every interval) and through the existing, oracle-pinned g kernels.

Tolerance of the trajectory parity: max(1e-11, 10 eps_ref), eps_ref the helper's own noise between two Newton starts
on the same inputs — both sides solve the same equations to rounding, 10x covers the different elimination order.
"""

import numpy as np
import pytest

from oracle import fes_collocation as CO
from oracle import fes_oracle as O
from tests import cases
from tests import colloc_ivp_reference as R

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps


@pytest.fixture(scope="module", autouse=True)
def _require_gpu():
    from cocofest_amd import _cfx

    lib = _cfx.load_library()  # raises if libcfx.so is missing: no silent fallback
    if lib.cfx_device_count() < 1:
        pytest.fail("no HIP device visible to libcfx")


def _handle(name, method, degree, n, batch, layout="soa"):
    ocp = cases.product_collocation_ocp(name, cases.TEN_PULSES, 1.0, 10, degree=degree, method=method, n_shooting=n,
                                        intensity_params=False)
    return ocp.nlp(batch=batch, layout=layout)


def _soa(X0, U):
    """(B, nx), (B, N, nu) -> the SoA host buffers of Handle.integrate: (nx, B), (N nu, B) or None."""
    B = X0.shape[0]
    return np.ascontiguousarray(X0.T), (np.ascontiguousarray(U.reshape(B, -1).T) if U.shape[2] else None)


def _run(name, method, degree, n, X0, U):
    """(traj (B, samples, nx), status (B,)) of the product on a SoA handle of X0's batch."""
    B, nx = X0.shape
    h = _handle(name, method, degree, n, B)
    try:
        x0, u = _soa(X0, U)
        traj = h.integrate(x0=x0, u=u)
        status = h.integrate_status()
    finally:
        h.close()
    return np.ascontiguousarray(traj.reshape(-1, nx, B).transpose(2, 0, 1)), status


# ---- 1. parity with the reference helper ------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [10, 20])
@pytest.mark.parametrize("degree", [1, 4, 5, 9])
@pytest.mark.parametrize("method", ["legendre", "radau"])
@pytest.mark.parametrize("name", O.MODEL_NAMES)
def test_trajectory_matches_the_full_newton_reference(name, method, degree, n):
    pb, X0, U, ref, conv, eps_ref = R.reference(name, method, degree, n)
    assert conv.all(), "the reference helper must converge on every instance of these inputs"
    assert eps_ref <= 1e-12, f"eps_ref {eps_ref:.3e}: the reference's own noise must stay at rounding level"
    tol = max(1e-11, 10 * eps_ref)
    fatigue = name.endswith("with_fatigue")
    for B in (R.B_MAX, 1):
        got, status = _run(name, method, degree, n, X0[:B], U[:B])
        assert got.shape == (B, n * (degree + 1) + 1, pb.nx)
        err = R.scaled_error(got, ref[:B])
        print(f"colloc ivp {name} {method} d={degree} N={n} B={B}: err {err:.3e} eps_ref {eps_ref:.3e} "
              f"max status {status.max()}")
        assert np.isfinite(got).all()
        assert err <= tol, f"scaled error {err:.3e} > {tol:.1e} (eps_ref {eps_ref:.3e})"
        assert (status >= 0).all()
        if fatigue:
            assert (status >= 1).all() and (status < 20).all()
        else:
            assert (status == 0).all()


# ---- 2. residual through the existing callbacks -----------------------------------------------------------------------
def _set_controls(ocp, name):
    if name.startswith("ding2007"):
        ocp.u_init[:] = 4e-4
    elif name.startswith("hmed2018"):
        ocp.u_init[:] = 60.0


def _row_terms_collocation(pb, v):
    """Largest term of every row of the collocation g at v, (B, ng): |C[i][j] x^i_r| and |dt f_r| for a defect row,
    |D[i] x^i_r| and |x_{k+1}| for a continuity row, |u| and the window for a sliding-window row."""
    _, Cm, D = CO.coefficients(pb.degree, pb.method)
    XC = pb.unpack_points(v)
    X, U, P = pb.unpack(v)
    blocks = []
    for j in range(1, pb.degree + 1):
        poly = np.abs(Cm[:, j][None, None, :, None] * XC).max(axis=2)
        blocks.append(np.maximum(poly, np.abs(pb.dt * CO._point_rhs(pb, XC, U, j))))
    blocks.append(np.maximum(np.abs(D[None, None, :, None] * XC).max(axis=2), np.abs(X[:, 1:, :])))
    if pb.n_slide:
        blocks.append(np.stack([np.maximum(np.abs(U[:, k, :]), np.abs(O.sliding_window(pb, P, k)))
                                for k in range(pb.n_shooting)], axis=1))
    return np.concatenate(blocks, axis=2).reshape(v.shape[0], -1)


COL_GUESS = [("ding2003_with_fatigue", "legendre", 4), ("ding2007", "radau", 3), ("hmed2018", "legendre", 9)]


@pytest.mark.parametrize("name, method, degree", COL_GUESS)
def test_integrated_guess_zeroes_the_collocation_rows(name, method, degree):
    """eval_g through k_colloc (pinned to the oracle by test_collocation_gpu.py) at FesOcp.integrated_guess: every
    defect, continuity and sliding-window row is zero to rounding.  Each row is measured against the same row at the
    reference helper's solution evaluated by oracle.fes_collocation.eval_g: 10x that, or 8 ulps of the row's largest
    term (a row is a sum of up to d + 2 rounded terms of that size)."""
    n = 10
    ocp = cases.product_collocation_ocp(name, cases.TEN_PULSES, 1.0, 10, degree=degree, method=method, n_shooting=n)
    _set_controls(ocp, name)
    v = ocp.integrated_guess(batch=2)
    assert v.shape == (2, ocp.nv) and np.array_equal(v[0], v[1])
    h = ocp.nlp(batch=2)
    try:
        g = h.eval_g(v)
    finally:
        h.close()
    pb = R.col_problem(name, cases.TEN_PULSES, 1.0, 10, n, degree, method, intensity_params=True)
    _, U, P = pb.unpack(v[:1])
    if pb.n_slide:  # the controls are the sliding windows of p_init
        assert np.array_equal(P[0], ocp.p_init)
        for k in range(n):
            assert np.array_equal(U[:, k, :], O.sliding_window(pb, P, k))
    elif pb.nu:
        assert np.array_equal(U[0], ocp.u_init.T)
    x0 = np.asarray(ocp.x_init, dtype=float)[:, 0][None, :]
    ref, conv = R.integrate(pb, x0, U, "copy")
    assert conv.all()
    body = ref[:, :-1, :].reshape(1, n, degree + 1, pb.nx)
    v_ref = pb.pack(body, ref[:, -1, :], U if pb.nu else None, P if pb.n_params else None)
    g_ref = CO.eval_g(pb, v_ref)
    terms = _row_terms_collocation(pb, v[:1])
    bound = np.maximum(10 * np.abs(g_ref), 8 * EPS * terms)
    worst = float((np.abs(g[:1]) / np.maximum(terms, 1e-300)).max())
    print(f"integrated_guess {name} {method} d={degree}: max |g| / largest term {worst:.3e}, "
          f"max |g| {np.abs(g).max():.3e}, reference rows max {np.abs(g_ref).max():.3e}")
    assert np.array_equal(g[0], g[1])
    assert (np.abs(g[:1]) <= bound).all(), f"worst row / term {worst:.3e}"
    # the node states are the reference's
    assert R.scaled_error(pb.unpack_points(v[:1]).reshape(1, -1, pb.nx), ref[:, :-1, :]) <= 1e-11


@pytest.mark.parametrize("name, scheme, m", [("ding2007_with_fatigue", "RK4", 5), ("hmed2018", "RK1", 1)])
def test_integrated_guess_zeroes_the_shooting_rows(name, scheme, m):
    """RK problems: every m-th sub-step of the k_ivp trajectory.  Rows measured against fes_oracle.eval_g at the
    oracle's own sequential integration: 10x that, or 8 ulps of the row's largest term (|x_{k+1}|, resp. |u|)."""
    n = 10
    ocp = cases.product_ocp(name, cases.TEN_PULSES, 1.0, 10, scheme=scheme, m=m, n_shooting=n)
    _set_controls(ocp, name)
    v = ocp.integrated_guess(batch=1)
    h = ocp.nlp(batch=1)
    try:
        g = h.eval_g(v)
    finally:
        h.close()
    pb = cases.oracle_problem(name, cases.TEN_PULSES, 1.0, 10, scheme=scheme, m=m, n_shooting=n)
    X, U, P = pb.unpack(v)
    x0 = np.asarray(ocp.x_init, dtype=float)[:, 0]
    tr = O.ivp_integrate(name, pb.c, pb.rows, U[0], 1.0, scheme, m, x0=x0)[:, ::m].T  # (N+1, nx)
    v_ref = np.concatenate([np.concatenate([tr[:-1], U[0]], axis=1).reshape(-1), tr[-1], P[0]])[None, :]
    g_ref = O.eval_g(pb, v_ref)
    parts = []
    for k in range(n):
        parts.append(np.maximum(np.abs(X[:, k + 1, :]), np.abs(X[:, k, :])))
        if pb.n_slide:
            parts.append(np.abs(U[:, k, :]))
    terms = np.concatenate(parts, axis=1)
    worst = float((np.abs(g) / np.maximum(terms, 1e-300)).max())
    print(f"integrated_guess {name} {scheme}x{m}: max |g| / largest term {worst:.3e}, reference rows max "
          f"{np.abs(g_ref).max():.3e}")
    assert (np.abs(g) <= np.maximum(10 * np.abs(g_ref), 8 * EPS * terms)).all(), f"worst row / term {worst:.3e}"
    assert R.scaled_error(X, tr[None]) <= 1e-11


# ---- 3. order ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method", ["legendre", "radau"])
def test_node_error_falls_with_the_degree(method):
    """Ding2003 from rest, N = 20 (the problem of test_collocation_oracle's convergence test): the node-state error
    against a fine RK4 integration falls monotonically over degrees 1..5, by at least 20x overall."""
    from cocofest_amd import IvpFes, ModelMaker, OdeSolver

    stims = [0.0, 0.1, 0.2, 0.3, 0.4]
    pb0 = R.col_problem("ding2003", stims, 0.5, 4, 20, 1, method)
    fine = O.ivp_integrate("ding2003", pb0.c, pb0.rows, np.zeros((20, 0)), 0.5, "RK4", 200)[:, ::200]
    errs = []
    for d in (1, 2, 3, 4, 5):
        model = ModelMaker.create_model("ding2003", stim_time=list(stims), sum_stim_truncation=4)
        ivp = IvpFes({"model": model}, {"final_time": 0.5, "n_shooting": 20,
                                        "ode_solver": OdeSolver.COLLOCATION(d, method)})
        res = ivp.integrate(return_time=False)
        ivp.close()
        nodes = np.stack([res["Cn"][0][:: d + 1], res["F"][0][:: d + 1]])
        errs.append(np.abs(nodes - fine).max())
    print(f"order {method}: {errs}")
    assert all(b < a for a, b in zip(errs, errs[1:])) and errs[-1] < errs[0] / 20, errs


# ---- 4. interfaces ----------------------------------------------------------------------------------------------------
def test_host_and_device_buffers_give_the_same_bits_and_batch_one_is_instance_zero():
    import torch

    name, method, degree, n = "hmed2018_with_fatigue", "radau", 4, 10
    pb, X0, U, _, _, _ = R.reference(name, method, degree, n)
    host, st_host = _run(name, method, degree, n, X0, U)
    one, st_one = _run(name, method, degree, n, X0[:1], U[:1])
    assert np.array_equal(one[0], host[0]) and st_one[0] == st_host[0]
    h = _handle(name, method, degree, n, R.B_MAX)
    try:
        x0, u = _soa(X0, U)
        dev = h.integrate(x0=torch.from_numpy(x0).cuda(), u=torch.from_numpy(u).cuda(),
                          traj=torch.empty((h.n_samples * h.nx, R.B_MAX), dtype=torch.float64, device="cuda"))
        st_dev = h.integrate_status(torch.empty(R.B_MAX, dtype=torch.int32, device="cuda"))
        torch.cuda.synchronize()
        got = dev.cpu().numpy().reshape(-1, pb.nx, R.B_MAX).transpose(2, 0, 1)
        assert np.array_equal(got, host)
        assert np.array_equal(st_dev.cpu().numpy(), st_host)
    finally:
        h.close()
    # AoS host buffers: the same values through the transposes
    h = _handle(name, method, degree, n, R.B_MAX, layout="aos")
    try:
        aos = h.integrate(x0=X0, u=U.reshape(R.B_MAX, -1))
        assert np.array_equal(aos.reshape(R.B_MAX, -1, pb.nx), host)
    finally:
        h.close()


@pytest.mark.parametrize("name", ["ding2003", "ding2007_with_fatigue"])
def test_default_start_is_the_rest_state(name):
    pb = R.col_problem(name, cases.TEN_PULSES, 1.0, 10, 10, 4, "legendre")
    _, U = R.random_inputs(pb, 3, seed=5)
    rest = np.tile(O.rest_values(name, pb.c)[None, :], (3, 1))
    h = _handle(name, "legendre", 4, 10, 3)
    try:
        _, u = _soa(rest, U)
        a = h.integrate(x0=None, u=u).copy()
        b = h.integrate(x0=np.ascontiguousarray(rest.T), u=u)
    finally:
        h.close()
    assert np.isfinite(a).all() and np.array_equal(a, b)


def test_status_before_any_integrate_is_einval():
    from cocofest_amd import CfxError, _cfx

    h = _handle("ding2003", "legendre", 2, 10, 1)
    try:
        with pytest.raises(CfxError) as exc:
            h.integrate_status()
        assert exc.value.code == _cfx.EINVAL and "cfx_integrate_status" in str(exc.value)
    finally:
        h.close()


@pytest.mark.parametrize("method, degree", [("legendre", 4), ("radau", 3), ("legendre", 7)])
def test_ivpfes_collocation_shapes_and_times(method, degree):
    from cocofest_amd import IvpFes, ModelMaker, OdeSolver

    n = 10
    model = ModelMaker.create_model("ding2007_with_fatigue", stim_time=list(cases.TEN_PULSES), sum_stim_truncation=10)
    ivp = IvpFes({"model": model, "pulse_width": 4e-4},
                 {"final_time": 1.0, "ode_solver": OdeSolver.COLLOCATION(degree, method)})
    assert ivp.n_shooting == n
    res, time = ivp.integrate()
    ivp.close()
    tau = np.concatenate([[0.0], CO.collocation_points(degree, method)])
    want_t = np.concatenate([(np.arange(n)[:, None] * 0.1 + tau[None, :] * 0.1).reshape(-1), [1.0]])
    assert time.shape == (n * (degree + 1) + 1,)
    np.testing.assert_allclose(time, want_t, rtol=0, atol=1e-14)
    assert set(res) == set(model.name_dof)
    pb = R.col_problem("ding2007_with_fatigue", cases.TEN_PULSES, 1.0, 10, n, degree, method)
    ref, conv = R.integrate(pb, O.rest_values(pb.name, pb.c)[None, :], np.full((1, n, 1), 4e-4), "copy")
    assert conv.all()
    got = np.stack([res[k][0] for k in model.name_dof], axis=1)[None]
    assert got.shape == (1, n * (degree + 1) + 1, 5)
    assert R.scaled_error(got, ref) <= 1e-11


def test_rk_handle_integrates_as_before_and_reports_zero_status():
    """The explicit path is untouched: every sub-step against the oracle (as test_gpu_parity.py), status all zero."""
    name = "ding2003_with_fatigue"
    ocp = cases.product_ocp(name, cases.TEN_PULSES, 1.0, 10, scheme="RK4", m=5, n_shooting=20)
    pb = cases.oracle_problem(name, cases.TEN_PULSES, 1.0, 10, scheme="RK4", m=5, n_shooting=20)
    h = ocp.nlp(batch=3, layout="soa")
    try:
        traj = h.integrate()
        status = h.integrate_status()
    finally:
        h.close()
    assert traj.shape == ((20 * 5 + 1) * 5, 3) and status.dtype == np.int32 and (status == 0).all()
    ref = O.ivp_integrate(name, pb.c, pb.rows, np.zeros((20, 0)), 1.0, "RK4", 5)  # (nx, samples)
    got = traj.reshape(-1, 5, 3)
    for b in range(3):
        scale = np.maximum(np.abs(ref), 1e-6 * np.abs(ref).max(axis=1, keepdims=True) + 1e-300)
        assert (np.abs(got[:, :, b].T - ref) / scale).max() <= 1e-11


def test_tiled_collocation_handles_still_refuse():
    from cocofest_amd import CfxError, _cfx

    ocp = cases.product_collocation_ocp("ding2003", cases.TEN_PULSES, 1.0, 10, degree=4, n_shooting=10)
    h = ocp.nlp(batch=64, layout="tiled64")
    try:
        with pytest.raises(CfxError) as exc:
            h.integrate()
        assert exc.value.code == _cfx.EUNSUPPORTED
    finally:
        h.close()


def test_msk_handles_keep_their_integration_and_refuse_collocation():
    """A musculoskeletal handle: `OcpFesMsk` and `cfx_msk_create` still refuse collocation, the RK trajectory keeps
    its size and values (every sub-step against the oracle, as test_msk_gpu.py), and the status is all zeros."""
    import ctypes as C

    import cocofest_amd as CA
    from cocofest_amd import _cfx
    from oracle import fes_msk as M
    from tests import msk_cases as MC

    cfg = MC.cfg5(m=4)
    ocp = MC.product_ocp(**cfg)
    pb = MC.oracle_problem(**cfg)
    with pytest.raises(NotImplementedError):
        CA.OcpFesMsk.prepare_ocp(model=ocp.model, final_time=1, objective={}, ode_solver=CA.OdeSolver.COLLOCATION(4),
                                 msk_info={"bound_type": "start_end", "bound_data": [[0, 5], [0, 90]],
                                           "with_residual_torque": False})
    lib = _cfx.load_library()
    for scheme in (_cfx.COLLOCATION_LEGENDRE, _cfx.COLLOCATION_RADAU):
        mp = _cfx.MskProblem()
        mp.abi_version, mp.scheme, mp.n_steps, mp.n_shooting = _cfx.ABI_VERSION, scheme, 4, 10
        mp.truncation, mp.layout, mp.batch, mp.final_time = 10, _cfx.LAYOUT_SOA, 1, 1.0
        out = C.c_void_p()
        assert lib.cfx_msk_create(C.byref(mp), C.byref(out)) == _cfx.EUNSUPPORTED and not out.value
        assert "scheme must be" in lib.cfx_last_error(None).decode()
    B = 2
    r = np.random.default_rng(9)
    U = r.uniform(2e-4, 5e-4, size=(B, pb.n_shooting, pb.nu))
    x0 = np.tile(ocp.initial_guess_vector()[: pb.nx], (B, 1))
    x0[:, pb.nxm + pb.nq - 1] = 0.3
    h = ocp.nlp(batch=B, layout="aos")
    try:
        assert not h.collocation and h.scheme == _cfx.RK4
        assert h.n_samples == pb.n_shooting * 4 + 1
        with pytest.raises(CA.CfxError):
            h.integrate_status()  # nothing integrated yet
        tr = h.integrate(x0=x0, u=U.reshape(B, -1))
        status = h.integrate_status()
    finally:
        h.close()
    assert tr.shape == (B, (pb.n_shooting * 4 + 1) * pb.nx)
    assert status.shape == (B,) and (status == 0).all()
    for b in range(B):
        ref = M.ivp(pb, x0[b], U[b])
        scale = np.abs(ref) + 1e-8 * np.abs(ref).max(axis=0)
        assert (np.abs(tr[b].reshape(-1, pb.nx) - ref) / scale).max() < 1e-9
