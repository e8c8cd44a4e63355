"""The automatic-differentiation oracle (oracle/fes_autodiff.py, torch float64 on the CPU) pinned to the numpy
oracle, and its own rounding noise measured.  No GPU.

What is asserted, for every model x RK1/RK2/RK4 at the shape of test_lagrangian_hessian_vs_oracle and every model x
{Legendre 1, Legendre 4, Radau 3, Radau 5}:

  * g equals the numpy oracle's within 1e-13 (|Phi| scale) and J_g within 1e-12: both are float64 evaluations of the
    same formulas.  Measured: g bit-identical but for one Hmed RK2 row (1e-16), J_g <= 2.3e-15, f and grad f
    bit-identical.
  * the numpy oracles' finite-difference Hessian agrees with the AD Hessian within the tolerance the GPU tests grant
    it (1e-7 shooting, 1e-6 collocation, entries floored at 1e-4 of the instance's largest).  Measured gap, i.e. the
    accuracy the finite-difference reference really has: shooting <= 1.0e-10 (Ding2003 RK2; Ding2007 <= 9e-13,
    Hmed <= 4.5e-11), collocation <= 5.0e-12.
  * the reference noise eps_ref (forward-over-forward against reverse-over-reverse under hessian_error) stays below
    the figure recorded in tests/hessian_cases.py, whose docstring tabulates the measured values per family and
    scheme, Hmed at T = 32 under RK4 and Legendre degree 9 included.  The GPU tolerance is max(RTOL, 10 eps_ref).
  * one deliberate mutation of the reference each (a dropped second derivative of the Hmed intensity chain, a
    swapped pair in the packed order) is far outside the tolerance the GPU tests use: the comparison has teeth.

Every test prints its measured figures (pytest -s shows them)."""

import numpy as np
import pytest

from oracle import fes_autodiff as AD
from oracle import fes_collocation as CO
from oracle import fes_oracle as O
from tests import cases, hessian_cases as HC

COL_CONFIGS = [("legendre", 1), ("legendre", 4), ("radau", 3), ("radau", 5)]


def _scaled(actual, desired, scale=None):
    """The _close measure of tests/test_gpu_parity.py: |actual - desired| / max(scale, 1e-6 of the row's largest)."""
    desired = np.asarray(desired)
    floor = np.max(np.abs(desired), axis=-1, keepdims=True) * 1e-6 + 1e-300
    scale = np.maximum(np.abs(desired) if scale is None else scale, floor)
    return float(np.max(np.abs(actual - desired) / scale))


def _g_scale(pb, v, desired):
    """The _close_g scale: |g| + |x_{k+1}| (sliding rows: |u_k|); defect rows of a collocation problem: the
    O(|x| (d + 1)^2) size of their summands, as test_collocation_callbacks_vs_oracle."""
    if isinstance(pb, CO.ColProblem):
        return np.abs(v).max(axis=1, keepdims=True) * (pb.degree + 1) ** 2 * np.ones_like(desired)
    X, U, _ = pb.unpack(v)
    parts = []
    for k in range(pb.n_shooting):
        parts.append(np.abs(X[:, k + 1, :]))
        if pb.n_slide:
            parts.append(np.abs(U[:, k, :]))
    return np.abs(desired) + np.concatenate(parts, axis=1)


def _fd_gap(fd, ad):
    scale = np.maximum(np.abs(ad), 1e-4 * np.max(np.abs(ad), axis=1, keepdims=True))
    return float(np.max(np.abs(fd - ad) / scale))


def _eps_ref(pb, v, of, lam):
    scale = AD.hessian_scale(pb, v, of, lam)
    ff, rr = AD.hessian_values(pb, v, of, lam, "ff"), AD.hessian_values(pb, v, of, lam, "rr")
    return AD.hessian_error(pb, ff, rr, scale)


def _check_against_numpy(pb, what, fd_tol):
    M = CO if isinstance(pb, CO.ColProblem) else O
    B = 3
    v = HC.decision(pb, B)
    lam, of = HC.multipliers(pb, B)
    g_ref = M.eval_g(pb, v)
    eg = _scaled(AD.eval_g(pb, v), g_ref, scale=_g_scale(pb, v, g_ref))
    ej = _scaled(AD.eval_jac_g(pb, v), M.eval_jac_g(pb, v))
    ef = _scaled(AD.eval_f(pb, v)[:, None], M.eval_f(pb, v)[:, None])
    egr = _scaled(AD.eval_grad_f(pb, v), M.eval_grad_f(pb, v))
    ad = AD.hessian_values(pb, v, of, lam)
    gap = _fd_gap(M.hessian_values(pb, v, of, lam), ad)
    eps = _eps_ref(pb, v, of, lam)
    scheme = pb.method if isinstance(pb, CO.ColProblem) else pb.scheme
    print(f"\n{what}: g {eg:.2e}  J_g {ej:.2e}  f {ef:.2e}  grad f {egr:.2e}  finite-difference gap {gap:.2e}  "
          f"eps_ref {eps:.2e}")
    assert eg <= 1e-13, f"g {eg:.3e}"
    assert ej <= 1e-12, f"J_g {ej:.3e}"
    assert ef <= 1e-13 and egr <= 1e-13, f"objective {ef:.3e} {egr:.3e}"
    assert gap <= fd_tol, f"finite-difference Hessian vs AD {gap:.3e}"
    assert eps <= HC.EPS_REF[HC.family(pb.name), scheme], f"eps_ref {eps:.3e}"
    # the scale dominates the value entry by entry (triangle inequality), and the structure holds every non-zero
    assert np.all(np.abs(ad) <= AD.hessian_scale(pb, v, of, lam) * (1 + 1e-12) + 1e-300)
    return v, of, lam, ad


@pytest.mark.parametrize("scheme", ["RK1", "RK2", "RK4"])
@pytest.mark.parametrize("name", O.MODEL_NAMES)
def test_shooting_matches_numpy_oracle(name, scheme):
    pb = cases.oracle_problem(**HC.shooting_cfg(name, scheme))
    _check_against_numpy(pb, f"{name} {scheme}", fd_tol=1e-7)


@pytest.mark.parametrize("method,degree", COL_CONFIGS)
@pytest.mark.parametrize("name", O.MODEL_NAMES)
def test_collocation_matches_numpy_oracle(name, method, degree):
    pb = HC.collocation_problem(name, degree, method)
    v, of, lam, ad = _check_against_numpy(pb, f"{name} {method} {degree}", fd_tol=1e-6)
    # nothing of the interval's dense Hessian lies outside hess_structure
    r, c = CO.hess_structure(pb)
    H = AD.hessian_blocks(pb, v, lam)
    mask = np.zeros((pb.n_shooting, pb.nzc, pb.nzc), dtype=bool)
    inner = r < pb.n_shooting * pb.nzc
    k = r[inner] // pb.nzc
    mask[k, r[inner] - k * pb.nzc, c[inner] - k * pb.nzc] = True
    mask |= mask.transpose(0, 2, 1)
    assert np.all(H[:, ~mask] == 0.0)


@pytest.mark.parametrize("case", ["hmed T=32 RK2", "hmed_fatigue T=17 RK2", "hmed T=32 RK4",
                                  "hmed_fatigue T=32 RK4", "legendre 9 ding",
                                  "legendre 9 hmed", "radau 2 hmed T=32"])
def test_reference_noise_at_the_large_shapes(case):
    """eps_ref where the recursion is longest: 32 intensity directions under RK4, and Legendre degree 9."""
    if case.startswith("hmed"):
        name = "hmed2018_with_fatigue" if "fatigue" in case else "hmed2018"
        pb = cases.oracle_problem(**HC.bucket_cfg(name, int(case.split()[1][2:]), scheme=case.split()[-1]))
        scheme = pb.scheme
    elif case.startswith("legendre"):
        pb = HC.collocation_problem("hmed2018_with_fatigue" if "hmed" in case else "ding2007_with_fatigue", 9,
                                    "legendre")
        scheme = "legendre"
    else:
        pb = HC.collocation_problem("hmed2018", 2, "radau", T=32)
        scheme = "radau"
    v = HC.decision(pb, 3)
    lam, of = HC.multipliers(pb, 3)
    eps = _eps_ref(pb, v, of, lam)
    print(f"\n{case}: eps_ref {eps:.2e}")
    assert eps <= HC.EPS_REF[HC.family(pb.name), scheme]


def test_tolerance_is_the_first_order_bound():
    """10 eps_ref stays below RTOL for every family, so the GPU comparison runs at the first-order bound."""
    assert all(10 * e <= HC.RTOL for e in HC.EPS_REF.values())
    pb = cases.oracle_problem(**HC.shooting_cfg("hmed2018", "RK4"))
    assert HC.tolerance(pb) == 1e-11
    pb.n_steps = 10  # 40 stages per interval
    assert HC.tolerance(pb) == 1e-10


def test_sliding_rows_contribute_nothing_and_zero_multipliers_leave_the_objective():
    pb = cases.oracle_problem(**HC.shooting_cfg("hmed2018", "RK2"))
    assert pb.n_slide
    v = HC.decision(pb, 2)
    lam, of = HC.multipliers(pb, 2)
    lam2 = lam.copy().reshape(2, pb.n_shooting, -1)
    lam2[:, :, pb.nx:] = 7.0
    np.testing.assert_array_equal(AD.hessian_values(pb, v, of, lam),
                                  AD.hessian_values(pb, v, of, lam2.reshape(2, -1)))
    H0 = AD.hessian_values(pb, v, of, np.zeros_like(lam))
    r, c = O.hess_structure(pb)
    assert np.all(H0[:, r != c] == 0.0)
    np.testing.assert_allclose(H0, O.hessian_values(pb, v, of, np.zeros_like(lam)), rtol=1e-15, atol=0)


def test_mutations_of_the_reference_are_caught(monkeypatch):
    """The comparison of test_hessian_exact.py has teeth: two deliberate one-line errors, each far outside the
    tolerance when the unmutated reference stands in for the kernel."""
    pb = cases.oracle_problem(**HC.shooting_cfg("hmed2018", "RK2"))
    v = HC.decision(pb, 3)
    lam, of = HC.multipliers(pb, 3)
    good, scale = AD.hessian_values(pb, v, of, lam), AD.hessian_scale(pb, v, of, lam)
    tol = HC.tolerance(pb)
    assert AD.hessian_error(pb, good, good, scale) == 0.0
    # (a) swapped pair in the packed order: the (Cn, F) entries of the last interval's last intensity row
    r, c = O.hess_structure(pb)
    last_u = pb.u_off(pb.n_shooting - 1) + pb.nu - 1
    i = int(np.flatnonzero((r == last_u) & (c == pb.x_off(pb.n_shooting - 1)))[0])
    swapped = good.copy()
    swapped[:, [i, i + 1]] = swapped[:, [i + 1, i]]
    e_swap = AD.hessian_error(pb, swapped, good, scale)

    # (b) the intensity chain's second derivative dropped: lambda_i linearised at the point, so its value and
    # first derivative (g, J_g) are unchanged and only lambda'' is missing from the Hessian
    def linearised(c, intensity):
        import torch

        at = intensity.detach()
        th = torch.tanh(c["bs"] * (at - c["Is"]))
        return c["ar"] * (th + c["cr"]) + c["ar"] * c["bs"] * (1 - th * th) * (intensity - at)

    g_before = AD.eval_jac_g(pb, v)
    monkeypatch.setattr(AD, "lambda_i", linearised)
    np.testing.assert_allclose(AD.eval_jac_g(pb, v), g_before, rtol=1e-13, atol=1e-300)
    e_drop = AD.hessian_error(pb, AD.hessian_values(pb, v, of, lam, "rr"), good, scale)
    print(f"\nmutations: swapped pair {e_swap:.2e}, dropped lambda'' {e_drop:.2e} (tolerance {tol:.0e})")
    assert e_swap > 1e3 * tol and e_drop > 1e3 * tol
