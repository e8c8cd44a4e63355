"""The Lagrangian Hessian kernels (cfx_eval_h, and the g + J_g + Hessian instantiations behind cfx_eval_all_h)
against an exact second-order reference: oracle/fes_autodiff.py, torch float64 automatic differentiation of the same
recursion on the CPU, with no step size.

Every case compares entry by entry under ``fes_autodiff.hessian_error``: |kernel - reference| over
sum_r |lam_r| |d2 Phi_r| + |obj_factor| |d2 f|, floored at 1e-6 of the largest reference entry of the entry's
interval block (per block, not per instance).  The tolerance is max(RTOL, 10 eps_ref) (tests/hessian_cases.py): RTOL
= 1e-11 is the project's first-order bound and eps_ref, the reference's own forward-over-forward against
reverse-over-reverse noise measured on the CPU alone (tests/test_autodiff_oracle.py), is at most 1.4e-14 on the Hmed
family and 3.0e-15 on the Ding families, recorded as 1e-13 / 1e-14.  So every case here is held to 1e-11, four to five
orders tighter than the finite-difference comparisons (1e-7 shooting, 1e-6 collocation, floor 1e-4 of the instance).

Largest scaled error measured on an MI355X per group, both entry points (tolerance 1e-11 each): shooting Ding
4.8e-15, shooting Hmed 1.3e-14, Hmed TMAX buckets 2.2e-14, Hmed T = 32 RK4 7.6e-15, edges 2.2e-14, block boundary
1.8e-14, collocation 4.1e-15, obj_factor = 0 1.3e-14.  The new comparison exposed no kernel error.
"""

import numpy as np
import pytest

from oracle import fes_autodiff as AD
from oracle import fes_collocation as CO
from oracle import fes_oracle as O
from tests import cases, hessian_cases as HC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _require_gpu():
    from cocofest_amd import _cfx

    lib = _cfx.load_library()  # raises if libcfx.so is missing: no silent fallback
    if lib.cfx_device_count() < 1:
        pytest.fail("no HIP device visible to libcfx")


def _check(pb, h, v, of, lam, what):
    """Both Hessian entry points of a host AoS handle against the reference."""
    ref, scale = HC.reference(what, pb, v, of, lam)
    tol = HC.tolerance(pb)
    r, c = h.hess_structure()
    rr, cc = (CO if isinstance(pb, CO.ColProblem) else O).hess_structure(pb)
    np.testing.assert_array_equal(r, rr)
    np.testing.assert_array_equal(c, cc)
    e_h = AD.hessian_error(pb, h.eval_h(v, of, lam), ref, scale)
    e_all = AD.hessian_error(pb, h.eval_all_h(v, of, lam)[2], ref, scale)
    print(f"\n{what}: eval_h {e_h:.2e}  eval_all_h {e_all:.2e}  (tolerance {tol:.0e})")
    assert e_h <= tol, f"{what} cfx_eval_h: {e_h:.3e} > {tol:.1e}"
    assert e_all <= tol, f"{what} cfx_eval_all_h: {e_all:.3e} > {tol:.1e}"


def _shooting(cfg, what, B=3):
    ocp = cases.product_ocp(**cfg)
    pb = cases.oracle_problem(**cfg)
    assert (ocp.nv, ocp.n_shooting) == (pb.nv, pb.n_shooting)
    v = HC.decision(pb, B)
    lam, of = HC.multipliers(pb, B)
    h = ocp.nlp(batch=B)
    assert (h.nv, h.ng) == (pb.nv, pb.ng)
    try:
        _check(pb, h, v, of, lam, what)
    finally:
        h.close()


@pytest.mark.parametrize("scheme", ["RK1", "RK2", "RK4"])
@pytest.mark.parametrize("name", O.MODEL_NAMES)
def test_shooting_hessian_exact(name, scheme):
    """All six models x RK1/RK2/RK4 at the shape of test_lagrangian_hessian_vs_oracle."""
    _shooting(HC.shooting_cfg(name, scheme), f"{name} {scheme}")


@pytest.mark.parametrize("T", [1, 4, 5, 8, 9, 16, 17, 32])
@pytest.mark.parametrize("name", ["hmed2018", "hmed2018_with_fatigue"])
def test_hmed_truncation_buckets_hessian_exact(name, T):
    """Both sides of every edge of the TMAX buckets 4 / 8 / 16 / 32 that k_hessian is compiled for."""
    _shooting(HC.bucket_cfg(name, T), f"{name} T={T} RK2")


@pytest.mark.parametrize("name", ["hmed2018", "hmed2018_with_fatigue"])
def test_hmed_largest_footprint_hessian_exact(name):
    """T = 32 under RK4: 32 intensity directions, the largest register footprint."""
    _shooting(HC.bucket_cfg(name, 32, scheme="RK4"), f"{name} T=32 RK4")


@pytest.mark.parametrize("name", ["ding2003_with_fatigue", "ding2007", "hmed2018"])
def test_edge_sizes_hessian_exact(name):
    """N = 1, batch 1, T = 1, RK4 x 1 (the shapes of test_edge_sizes)."""
    cfg = HC.edge_cfg(name)
    assert cases.oracle_problem(**cfg).n_shooting == 1
    _shooting(cfg, f"edge {name}", B=1)


@pytest.mark.parametrize("name,T", [("ding2007_with_fatigue", 3), ("hmed2018", 5)])
def test_block_boundary_hessian_exact(name, T):
    """B = 257 on SoA device buffers: the second 256-thread block holds one instance.  Instances on both sides of
    the wave and block edges against the reference."""
    import torch

    cfg = HC.shooting_cfg(name, "RK2", T=T)
    ocp = cases.product_ocp(**cfg)
    pb = cases.oracle_problem(**cfg)
    B = 257
    v = HC.decision(pb, B)
    lam, of = HC.multipliers(pb, B)
    pick = np.array([0, 63, 64, 255, 256])
    ref, scale = HC.reference(f"block {name}", pb, v[pick], of[pick], lam[pick])
    h = ocp.nlp(batch=B, layout="soa")
    dev = lambda a: torch.tensor(np.ascontiguousarray(a), device="cuda")  # noqa: E731
    dv, dof, dlam = dev(v.T), dev(of), dev(lam.T)
    hh = h.eval_h(dv, dof, dlam, torch.empty((h.nnz_hess, B), dtype=torch.float64, device="cuda"))
    _, _, fh = h.eval_all_h(dv, dof, dlam)
    torch.cuda.synchronize()
    got_h, got_all = hh.cpu().numpy().T, fh.cpu().numpy().T
    h.close()
    tol = HC.tolerance(pb)
    e_h = AD.hessian_error(pb, got_h[pick], ref, scale)
    e_all = AD.hessian_error(pb, got_all[pick], ref, scale)
    print(f"\nblock boundary {name}: eval_h {e_h:.2e}  eval_all_h {e_all:.2e}  (tolerance {tol:.0e})")
    assert e_h <= tol and e_all <= tol, (e_h, e_all)
    assert np.all(np.isfinite(got_h)) and np.all(np.isfinite(got_all))


def _collocation(name, degree, method, B, T=4):
    from tests.oracle_handle import oracle_problem_from_ocp

    ocp = cases.product_collocation_ocp(name, HC.COL_STIMS, 0.5, T, degree=degree, method=method,
                                        objective=HC.COL_OBJECTIVE, n_shooting=3)
    pb = oracle_problem_from_ocp(ocp)
    return ocp, pb, HC.decision(pb, B, seed=degree), HC.multipliers(pb, B)


@pytest.mark.parametrize("B", [4, 3])
@pytest.mark.parametrize("method,degree", [("legendre", 1), ("legendre", 4), ("radau", 3), ("radau", 5),
                                           ("legendre", 9)])
@pytest.mark.parametrize("name", O.MODEL_NAMES)
def test_collocation_hessian_exact(name, method, degree, B):
    """k_colloc_hess, every model x scheme; the even batch takes the two-instances-per-lane path of the Ding families
    at degree <= 5, the odd batch one instance per lane."""
    ocp, pb, v, (lam, of) = _collocation(name, degree, method, B)
    h = ocp.nlp(batch=B, layout="aos")
    assert (h.nv, h.ng) == (pb.nv, pb.ng)
    try:
        _check(pb, h, v, of, lam, f"collocation {name} {method} {degree} B={B}")
    finally:
        h.close()


@pytest.mark.parametrize("T", [5, 17, 32])
@pytest.mark.parametrize("name", ["hmed2018", "hmed2018_with_fatigue"])
def test_collocation_hmed_buckets_hessian_exact(name, T):
    ocp, pb, v, (lam, of) = _collocation(name, 2, "radau", 3, T=T)
    h = ocp.nlp(batch=3, layout="aos")
    try:
        _check(pb, h, v, of, lam, f"collocation {name} radau 2 T={T}")
    finally:
        h.close()


@pytest.mark.parametrize("kind", ["ding", "hmed", "collocation"])
def test_degenerate_multipliers(kind):
    """lam = 0: exactly the objective diagonal obj_factor * 2 w, exactly 0 elsewhere (bitwise).  obj_factor = 0: the
    constraint part of the reference."""
    B = 3
    if kind == "collocation":
        ocp, pb, v, (lam, of) = _collocation("ding2007_with_fatigue", 3, "radau", B)
        M = CO
    else:
        cfg = HC.shooting_cfg("ding2003_with_fatigue" if kind == "ding" else "hmed2018", "RK2")
        ocp, pb = cases.product_ocp(**cfg), cases.oracle_problem(**cfg)
        v, (lam, of) = HC.decision(pb, B), HC.multipliers(pb, B)
        M = O
    h = ocp.nlp(batch=B, layout="aos")
    zero = np.zeros_like(lam)
    expect = np.zeros((B, h.nnz_hess))
    r, c = M.hess_structure(pb)
    diag = np.zeros((B, pb.nv))
    for w, _, _, off in O._obj_terms(pb, v):
        diag[:, off] += of * (2 * w)
    expect[:, r == c] = diag[:, r[r == c]]
    assert np.count_nonzero(expect) > 0
    got0, got0_all = h.eval_h(v, of, zero), h.eval_all_h(v, of, zero)[2]
    no_obj = np.zeros(B)
    got1, got1_all = h.eval_h(v, no_obj, lam), h.eval_all_h(v, no_obj, lam)[2]
    h.close()
    np.testing.assert_array_equal(got0, expect)
    np.testing.assert_array_equal(got0_all, expect)
    ref, scale = HC.reference(f"no objective {kind}", pb, v, no_obj, lam)
    tol = HC.tolerance(pb)
    e_h, e_all = AD.hessian_error(pb, got1, ref, scale), AD.hessian_error(pb, got1_all, ref, scale)
    print(f"\nobj_factor = 0, {kind}: eval_h {e_h:.2e}  eval_all_h {e_all:.2e}  (tolerance {tol:.0e})")
    assert e_h <= tol and e_all <= tol, (e_h, e_all)
