"""The native interior point (cfx_ipm_*, csrc/cfx_ipm.hip) certified by tests/kkt_certificate.py: the returned v, y
(k_ipm_out) and bound multipliers (k_ipm_final) satisfy the first-order conditions of the unscaled NLP, recomputed in
numpy from the float64 oracle with no line of the solver.  Every instance of every case is certified.

Beside the assertions of test_kkt_certificate_cpu.py (kkt_certificate.assert_certified) each case checks the reported
``kkt_error``: at most tol, and equal to the recomputed scaled error to within the certificate's rounding allowance
plus the gap between GPU and oracle evaluations — the project's parity tolerance (1e-9 relative on g, J_g and grad f)
carried through the residual sums (certificate()'s ``scaled_gap``), not a constant.
"""

import json
import pathlib

import numpy as np
import pytest

from tests import cases
from tests.kkt_certificate import active_jacobian, assert_certified, certificate, describe
from tests.oracle_handle import oracle_problem_from_ocp
from tests.test_kkt_certificate_cpu import SCALINGS, T11, problem, specification, starts

pytestmark = pytest.mark.gpu

TOL = 1e-8
FT = json.loads((pathlib.Path(__file__).parent / "golden" / "ref_formulas.json").read_text())["misc"]["force_tracking"]
TRACK = {"force_tracking": [np.array(FT["time"]), np.array(FT["force"])]}
_CFG3 = []


def cfg3():
    """cfg 3 with Fourier force tracking (Ding2007 pulse widths, 30 pulses, N = 100): many active width bounds."""
    if not _CFG3:
        cfg = dict(cases.cfg3(), objective=TRACK)
        _CFG3.append((cases.product_ocp(**cfg), cases.oracle_problem(**cfg)))
    return _CFG3[0]


def native(ocp, v0, options, fixed_values=None, warm_start=None):
    """One NativeIpm solve: (result, z_l, z_u)."""
    from cocofest_amd.solver import NativeIpm

    nat = NativeIpm(ocp, batch=v0.shape[0], options=options)
    try:
        r = nat.solve(v0, fixed_values=fixed_values, warm_start=warm_start)
        z_l, z_u = nat.last_bound_multipliers
    finally:
        nat.close()
    return r, np.asarray(z_l), np.asarray(z_u)


def certify(ocp, pb, v0, r, z_l, z_u, options, what=""):
    """Every assertion on one solve; returns the certificate."""
    lb, ub = ocp.bounds_vector()
    c = certificate(pb, lb, ub, r.v, r.y, z_l, z_u, v0, options)
    print(what, "iterations", r.iterations, "kkt_error", r.kkt_error, describe(c))
    assert (r.status == 0).all() and r.converged.all(), (what, r.status, r.kkt_error)
    assert z_l.shape == z_u.shape == r.v.shape
    assert_certified(c, options.tol, what=what)
    assert np.all(r.kkt_error <= options.tol), (what, r.kkt_error)
    assert np.all(np.abs(r.kkt_error - c["scaled_error"]) <= c["scaled_allow"] + c["scaled_gap"]), \
        (what, r.kkt_error, c["scaled_error"], c["scaled_gap"])
    return c


def compare_multipliers(kind, v0, r, z_l, z_u, options, full_rank=True, **opts):
    """y and z_l - z_u of the native solve against the CPU specification's.  Both satisfy, at the specification's
    point v_c with A = [J_g; unit rows of the active bounds] over the free variables,
    A^T lambda = -grad f + rho,  lambda = [y; z_u - z_l on the active set],  rho the stationarity residual of that
    multiplier set at v_c with the inactive bound multipliers counted as residual.  So
    A^T (lambda_gpu - lambda_cpu) = rho_gpu - rho_cpu, and where A has full row rank (asserted with matrix_rank)
    |lambda_gpu - lambda_cpu|_2 <= (|rho_gpu|_2 + |rho_cpu|_2) / sigma_min(A): the bound asserted on y and on the
    active z_l - z_u.  Where the active constraints are linearly dependent (``full_rank=False``, asserted too) the
    multipliers are not unique and only their image is determined: |A^T (lambda_gpu - lambda_cpu)|_2 <= |rho_gpu|_2 +
    |rho_cpu|_2 is asserted instead.  An inactive multiplier is bounded on each side by its own complementarity,
    z <= (tol s_c / sf + rounding) / slack."""
    ocp, pb = problem(kind)
    lb, ub = ocp.bounds_vector()
    free = lb != ub
    s, s_zl, s_zu, _ = specification(kind, v0, **opts)
    assert (s.status == 0).all()
    for b in range(v0.shape[0]):
        A, actL, actU = active_jacobian(pb, lb, ub, s.v[b], options)
        act = actL | actU
        rank = np.linalg.matrix_rank(A)
        assert (rank == A.shape[0]) == full_rank, (kind, b, A.shape, rank)
        rho = []
        for y_, zl_, zu_ in ((r.y, z_l, z_u), (s.y, s_zl, s_zu)):
            c = certificate(pb, lb, ub, s.v[b:b + 1], y_[b:b + 1], np.where(act, zl_[b], 0.0)[None],
                            np.where(act, zu_[b], 0.0)[None], v0[b:b + 1], options)
            rho.append(np.linalg.norm(c["r"][0][free]))
        zg, zc = (z_l - z_u)[b], (s_zl - s_zu)[b]
        dlam = np.concatenate([r.y[b] - s.y[b], -(zg - zc)[act]])
        dy = np.abs(r.y[b] - s.y[b]).max()
        dz = np.abs(zg - zc)[act].max(initial=0.0)
        ymax, zmax = np.abs(s.y[b]).max(), np.abs(zc).max()
        if full_rank:
            smin = np.linalg.svd(A, compute_uv=False)[-1]
            bound = (rho[0] + rho[1]) / smin
            print(kind, b, "rank %d sigma_min %.3e rho %.3e %.3e bound %.3e; dy / max|y| %.3e dz / max|z| %.3e bound / "
                  "max|y| %.3e bound / max|z| %.3e" % (rank, smin, rho[0], rho[1], bound, dy / ymax, dz / zmax,
                                                      bound / ymax, bound / zmax))
            assert dy / ymax <= bound / ymax and dz / zmax <= bound / zmax, (kind, b, dy, dz, bound)
        else:
            img = np.linalg.norm(A.T @ dlam)
            print(kind, b, "rank %d of %d rows; |A^T dlambda| %.3e rho %.3e %.3e; dy / max|y| %.3e dz / max|z| %.3e"
                  % (rank, A.shape[0], img, rho[0], rho[1], dy / ymax, dz / zmax))
            assert img <= rho[0] + rho[1], (kind, b, img, rho)
        # inactive multipliers: each side's own complementarity bounds them
        cg = certificate(pb, lb, ub, r.v[b:b + 1], r.y[b:b + 1], z_l[b:b + 1], z_u[b:b + 1], v0[b:b + 1], options)
        cc = certificate(pb, lb, ub, s.v[b:b + 1], s.y[b:b + 1], s_zl[b:b + 1], s_zu[b:b + 1], v0[b:b + 1], options)
        inL, inU = free & ~act & np.isfinite(lb), free & ~act & np.isfinite(ub)
        for (vv, zl_, zu_, c) in ((r.v[b], z_l[b], z_u[b], cg), (s.v[b], s_zl[b], s_zu[b], cc)):
            cap = options.tol * c["s_c"][0] / c["sf"][0] + c["complementarity_allow"][0]
            assert np.all(zl_[inL] * (vv - c["lb_relaxed"])[inL] <= cap), (kind, b)
            assert np.all(zu_[inU] * (c["ub_relaxed"] - vv)[inU] <= cap), (kind, b)


@pytest.mark.parametrize("range_scaling,method", SCALINGS)
@pytest.mark.parametrize("kind", ["ding2007", "hmed2018"])
def test_four_pulse_tracking_scalings_and_multipliers(kind, range_scaling, method):
    """4-pulse force tracking, B = 3 from perturbed starts (per-instance sf and sg), the four scaling combinations:
    k_ipm_init's scaling and k_ipm_final / k_ipm_out's unscaling with d != 1 and sf, sg != 1; multipliers against the
    CPU specification.

    Measured on an MI355X: ding2007 (rank 11 = 8 + 3 active bounds, sigma_min 1.9e-6): |dy| / max|y| 5e-16 .. 3e-15,
    |dz| / max|z| 5e-15 .. 4e-13, against bounds of 3e-4 .. 4.5 (y) and 5e-7 .. 8e-3 (z).  hmed2018: 35 active rows on
    28 free variables, rank 26 (states resting on their zero bound before the first effective pulse), so its
    multipliers are not unique and only A^T lambda is compared: |A^T dlambda| 9e-11 .. 1.5e-10 against 3e-7 .. 7e-6;
    the multipliers themselves still agree to 3e-12 .. 1e-10 relative."""
    from cocofest_amd.solver import IpmOptions

    ocp, pb = problem(kind)
    v0 = starts(ocp, 3, 11)
    o = dict(tol=TOL, max_iter=300, range_scaling=range_scaling, nlp_scaling_method=method)
    options = IpmOptions(**o)
    r, z_l, z_u = native(ocp, v0, options)
    certify(ocp, pb, v0, r, z_l, z_u, options, what=kind)
    compare_multipliers(kind, v0, r, z_l, z_u, options, full_rank=kind != "hmed2018", **o)


def test_fatigue_rk4_five_state_nodes():
    """ding2007_with_fatigue, RK4 x 3, 4 pulses, B = 2: five-state nodes; multipliers against the specification.

    Measured on an MI355X (rank 23, sigma_min 1.4e-6): |dy| / max|y| 2e-15 .. 3e-15, |dz| / max|z| 2e-12 .. 4e-12,
    against bounds of 7e-3 (y) and 4e-5 (z)."""
    from cocofest_amd.solver import IpmOptions

    ocp, pb = problem("fatigue")
    v0 = starts(ocp, 2, 1)
    o = dict(tol=TOL, max_iter=300)
    options = IpmOptions(**o)
    r, z_l, z_u = native(ocp, v0, options)
    certify(ocp, pb, v0, r, z_l, z_u, options, what="fatigue")
    compare_multipliers("fatigue", v0, r, z_l, z_u, options, **o)


@pytest.mark.parametrize("B", [1, 8])
def test_cfg3_dissected_blocks_and_one_band(B):
    """cfg 3: dissected blocks plus border at B = 1, one band at B = 8."""
    from cocofest_amd.solver import IpmOptions

    ocp, pb = cfg3()
    v0 = starts(ocp, B, 0)
    options = IpmOptions(tol=TOL, max_iter=300)
    r, z_l, z_u = native(ocp, v0, options)
    c = certify(ocp, pb, v0, r, z_l, z_u, options, what=f"cfg3 B={B}")
    # many active width bounds: their multipliers are what the unscaling divides by sf d
    assert ((np.maximum(z_l, z_u) * c["sf"][:, None] * c["d"]) > 1e3 * TOL).sum(1).min() >= 5


@pytest.mark.parametrize("kkt", ["chain", "band"])
def test_cfg3_chain_and_band_layouts(kkt, monkeypatch):
    from cocofest_amd.solver import IpmOptions

    monkeypatch.setenv("CFX_IPM_KKT", kkt)
    ocp, pb = cfg3()
    v0 = starts(ocp, 2, 0)
    options = IpmOptions(tol=TOL, max_iter=300)
    r, z_l, z_u = native(ocp, v0, options)
    certify(ocp, pb, v0, r, z_l, z_u, options, what=f"cfg3 {kkt}")


@pytest.mark.parametrize("mu", ["monotone", "adaptive"])
def test_cfg3_wide_split_kernels(mu, monkeypatch):
    """CFX_IPM_WIDE=1: the k_w* split kernels."""
    from cocofest_amd.solver import IpmOptions

    monkeypatch.setenv("CFX_IPM_WIDE", "1")
    ocp, pb = cfg3()
    v0 = starts(ocp, 2, 3)
    options = IpmOptions(tol=TOL, max_iter=300, mu_strategy=mu)
    r, z_l, z_u = native(ocp, v0, options)
    certify(ocp, pb, v0, r, z_l, z_u, options, what=f"cfg3 wide {mu}")


def test_hmed_sliding_window_parameters_in_the_border():
    """Hmed2018 intensities as parameters with sliding windows (k_ipm_schur's dense border); force tracking, so the
    optimum is not the flat valley of the end-node objective."""
    from cocofest_amd.solver import IpmOptions

    cfg = dict(name="hmed2018", stims=[0.0, 0.1, 0.2, 0.3, 0.4], final_time=0.5, truncation=5, scheme="RK1", m=5,
               objective={"force_tracking": [T11, 40 * T11]}, n_shooting=None)
    ocp, pb = cases.product_ocp(**cfg), cases.oracle_problem(**cfg)
    v0 = starts(ocp, 2, 5)
    options = IpmOptions(tol=TOL, max_iter=300)
    r, z_l, z_u = native(ocp, v0, options)
    certify(ocp, pb, v0, r, z_l, z_u, options, what="hmed sliding window")


def test_collocation_kkt_shape():
    """Direct collocation of the cfg 3 shape (test_ipm_native.py::test_native_ipm_collocation's problem): ding2007,
    30 pulses, truncation 10, Legendre degree 4, tol 1e-6.  The intervals are the problem's own (N = 100): with 10
    intervals of three pulses each the transcription is locally infeasible (the specification ends with
    Infeasible_Problem_Detected from the initial guess), and an infeasible exit has no KKT certificate."""
    from cocofest_amd.solver import IpmOptions

    stims = [float(t) for t in np.round(np.linspace(0, 1, 31)[:-1], 2)]
    ocp = cases.product_collocation_ocp("ding2007", stims, 1.0, 10, degree=4, objective=TRACK)
    pb = oracle_problem_from_ocp(ocp)
    v0 = starts(ocp, 2, 0)
    options = IpmOptions(tol=1e-6, max_iter=300)
    r, z_l, z_u = native(ocp, v0, options)
    certify(ocp, pb, v0, r, z_l, z_u, options, what="collocation")


def test_cfg3_fixed_values_per_instance():
    """Per-instance fixed values: v carries the caller's values, z is exactly 0 there (zero_where_no_bound)."""
    from cocofest_amd.solver import IpmOptions

    ocp, pb = cfg3()
    lb, ub = ocp.bounds_vector()
    nfix = int((lb == ub).sum())
    fixed = np.stack([np.linspace(0.0, 0.3, nfix), np.linspace(0.0, 20.0, nfix)])
    v0 = starts(ocp, 2, 3)
    options = IpmOptions(tol=TOL, max_iter=300)
    r, z_l, z_u = native(ocp, v0, options, fixed_values=fixed)
    np.testing.assert_array_equal(r.v[:, lb == ub], fixed)
    assert np.all(z_l[:, lb == ub] == 0) and np.all(z_u[:, lb == ub] == 0)
    certify(ocp, pb, v0, r, z_l, z_u, options, what="cfg3 fixed values")


def test_cfg3_relaxed_bounds_and_the_projection():
    """bound_relax_factor = 1e-8.  honor_original_bounds=False returns the iterate: a KKT point of the relaxed problem,
    inside the relaxed bounds, and (active width bounds) outside the original ones somewhere.  True projects that
    iterate onto the original bounds in k_ipm_final: the two solves take the same path (the option acts after the
    loop), so the projected v is the clipped iterate — up to the rounding of (lb / d) d — with the same y and z; it is
    inside the original bounds.  The projected point itself is 1e-8 away from the relaxed problem's KKT point at every
    active bound, so the residual bounds derived from err <= tol hold for the iterate, not for it."""
    from cocofest_amd.solver import IpmOptions

    ocp, pb = cfg3()
    lb, ub = ocp.bounds_vector()
    v0 = starts(ocp, 2, 0)
    res = {}
    for honor in (False, True):
        options = IpmOptions(tol=TOL, max_iter=300, bound_relax_factor=1e-8, honor_original_bounds=honor)
        res[honor] = native(ocp, v0, options) + (options,)
    r, z_l, z_u, options = res[False]
    c = certify(ocp, pb, v0, r, z_l, z_u, options, what="cfg3 relaxed")
    outside = (r.v < lb) | (r.v > ub)
    assert outside.any(1).all()  # the projection has something to do
    assert np.all(r.v >= c["lb_relaxed"]) and np.all(r.v <= c["ub_relaxed"])
    rh, zh_l, zh_u, oh = res[True]
    ch = certificate(pb, lb, ub, rh.v, rh.y, zh_l, zh_u, v0, oh)
    print("honor_original_bounds", describe(ch))
    assert (rh.status == 0).all()
    assert ch["finite"].all() and ch["nonnegative"].all() and ch["zero_where_no_bound"].all()
    assert np.all(ch["bound_violation"] == 0.0), ch["bound_violation_raw"]  # against the original bounds
    eps = np.finfo(np.float64).eps
    np.testing.assert_allclose(rh.v, np.clip(r.v, lb, ub), rtol=4 * eps, atol=0)
    np.testing.assert_array_equal(rh.v[~outside], r.v[~outside])
    np.testing.assert_array_equal(rh.y, r.y)
    np.testing.assert_array_equal(zh_l, z_l)
    np.testing.assert_array_equal(zh_u, z_u)
    np.testing.assert_array_equal(rh.kkt_error, r.kkt_error)


def test_cfg3_ipopt_profile():
    """IpmOptions.ipopt: adaptive mu, constant z init, no range scaling, bound relaxation, inertia test."""
    from cocofest_amd.solver import IpmOptions

    ocp, pb = cfg3()
    v0 = starts(ocp, 1, 0)
    options = IpmOptions.ipopt(tol=TOL)
    r, z_l, z_u = native(ocp, v0, options)
    certify(ocp, pb, v0, r, z_l, z_u, options, what="cfg3 ipopt profile")


def test_cfg3_limited_memory_hessian():
    """L-BFGS path: the certificate does not depend on the Hessian."""
    from cocofest_amd.solver import IpmOptions

    ocp, pb = cfg3()
    v0 = starts(ocp, 1, 3, spread=1.0)
    options = IpmOptions(tol=TOL, max_iter=1000, hessian_approximation="limited-memory")
    r, z_l, z_u = native(ocp, v0, options)
    certify(ocp, pb, v0, r, z_l, z_u, options, what="cfg3 limited-memory")


def test_warm_start_round_trip():
    """k_ipm_init's warm branch (y_s = sf y / sg, z_s = sf d z) is the inverse of k_ipm_out / k_ipm_final's unscaling.

    With warm_start_init_point, mu_init = tol / 10, the warm-start pushes at 1e-14 and max_iter = 1 the host loop
    (ipm_solve) evaluates the callbacks at the start, k_ipm_init scales and maps the multipliers (no least-squares
    step: S.reinit = 0), k_ipm_begin computes S.err0 of that start before any step, and nothing writes S.err0 after it
    (k_ipm_out copies it) — a converged start breaks out of the loop at the same value.  So the reported kkt_error is
    the scaled error of the given (v, y, z_l, z_u) with the scalings evaluated there, which the certificate recomputes:

    * at the converged point both are rounding-sized;
    * at non-optimal inputs (v at the middle of every finite range, y and z random in [0.5, 2]; and rescaled y, z at
      the feasible point, so that each of the three parts of the error leads once) the number is O(100) and the two
      must agree to the evaluation gap: this pins sf, sg, d, J^T y, the signs of z_l and z_u, s_d and s_c in the
      kernels against numpy.  Measured on an MI355X: reported and recomputed agree to all 9 printed digits
      (480.98991748 for the first input) against a propagated gap of 2.9e-6.
    Then a full warm-started solve from the converged point: status 0, the same point to 1e-6 of each range, strictly
    fewer iterations than the cold solve."""
    from cocofest_amd.solver import IpmOptions

    ocp, pb = cfg3()
    lb, ub = ocp.bounds_vector()
    free = lb != ub
    v0 = starts(ocp, 2, 0)
    cold_opt = IpmOptions(tol=TOL, max_iter=300)
    r, z_l, z_u = native(ocp, v0, cold_opt)
    certify(ocp, pb, v0, r, z_l, z_u, cold_opt, what="cold")
    warm = dict(tol=TOL, warm_start_init_point=True, mu_init=TOL / 10, warm_start_bound_push=1e-14,
                warm_start_bound_frac=1e-14, warm_start_mult_bound_push=1e-14)
    one = IpmOptions(max_iter=1, **warm)

    r1, _, _ = native(ocp, r.v, one, warm_start=(r.y, z_l, z_u))
    c1 = certificate(pb, lb, ub, r.v, r.y, z_l, z_u, r.v, one)
    print("round trip at the optimum: reported", r1.kkt_error, "recomputed", c1["scaled_error"], "gap", c1["scaled_gap"])
    assert np.all(np.abs(r1.kkt_error - c1["scaled_error"]) <= c1["scaled_allow"] + c1["scaled_gap"])

    rng = np.random.default_rng(7)
    both = free & np.isfinite(lb) & np.isfinite(ub)
    vm = r.v.copy()
    vm[:, both] = 0.5 * (lb[both] + ub[both])
    ym = rng.uniform(0.5, 2.0, r.y.shape)
    zlm = np.where(free & np.isfinite(lb), rng.uniform(0.5, 2.0, r.v.shape), 0.0)
    zum = np.where(free & np.isfinite(ub), rng.uniform(0.5, 2.0, r.v.shape), 0.0)
    # the reported number is a maximum of three parts, so one input pins one part.  The input above makes the
    # constraint violation the largest; at the feasible r.v, small z leaves the dual residual (s_d = 1), large y the
    # dual residual with s_d > 1, large z the complementarity with s_c > 1.  Which part leads is asserted from the
    # certificate, not from the solver
    inputs = {"e_p": (vm, ym, zlm, zum), "e_d": (r.v, ym, 1e-3 * zlm, 1e-3 * zum),
              "e_d, s_d > 1": (r.v, 1e3 * ym, 1e-3 * zlm, 1e-3 * zum), "e_c, s_c > 1": (r.v, 1e-3 * ym, 1e3 * zlm, 1e3 * zum)}
    for lead, (vv, yy, zl_, zu_) in inputs.items():
        r2, _, _ = native(ocp, vv, one, warm_start=(yy, zl_, zu_))
        c2 = certificate(pb, lb, ub, vv, yy, zl_, zu_, vv, one)
        print("round trip off the optimum,", lead, ": reported", r2.kkt_error, "recomputed", c2["scaled_error"], "parts",
              c2["e_d"], c2["e_p"], c2["e_c"], "s_d", c2["s_d"], "s_c", c2["s_c"], "gap", c2["scaled_gap"], "allow",
              c2["scaled_allow"])
        assert np.all(c2[lead[:3]] == c2["scaled_error"]) and np.all(c2["scaled_error"] > 1e2)  # O(100), not noise
        others = [k for k in ("e_d", "e_p", "e_c") if k != lead[:3]]
        assert all(np.all(c2[k] < 0.75 * c2["scaled_error"]) for k in others)
        if "s_d" in lead:
            assert np.all(c2["s_d"] > 1.5)
        if "s_c" in lead:
            assert np.all(c2["s_c"] > 1.5)
        assert np.all(np.abs(r2.kkt_error - c2["scaled_error"]) <= c2["scaled_allow"] + c2["scaled_gap"]), lead

    r3, _, _ = native(ocp, r.v, IpmOptions(max_iter=300, **warm), warm_start=(r.y, z_l, z_u))
    print("warm-started solve: iterations", r3.iterations, "cold", r.iterations)
    assert (r3.status == 0).all()
    span = np.where(np.isfinite(ub - lb), ub - lb, np.maximum(np.abs(r.v).max(0), 1.0))
    assert np.max(np.abs(r3.v - r.v)[:, free] / span[free]) <= 1e-6
    assert np.all(r3.iterations < r.iterations), (r3.iterations, r.iterations)
