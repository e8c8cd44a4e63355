"""The musculoskeletal Lagrangian Hessian kernels (cfx_msk.h: k_msk_htan, k_msk_hadj, k_msk_hpair, k_msk_hproj,
k_msk_hproj_stage, k_msk_hproj_stage_lds, k_msk_hproj_sum, and the marker and objective terms) against an exact
second-order reference: oracle/msk_autodiff.py, torch float64 automatic differentiation of the oracle's own
recursion on the CPU, with no step size.

Every case scatters the product's (row, col, value) triplets into a dense symmetric matrix (repeated pairs summed,
the lower triangle mirrored) and compares it entry by entry, every interval, the node-N block and every instance,
with the dense reference under ``msk_autodiff.hessian_error``: |kernel - reference| over sum_r |lam_r| |d2 g_r| +
|obj_factor| |d2 f|, floored at 1e-6 of the largest reference entry of the same interval block and the same unordered
pair of variable groups (Cn, F, A, Tau1, Km, q, qdot, pulse width, intensity, residual torque, parameter).  A
reference entry at a position the product's structure does not list is compared with 0, an entry of a group pair whose
reference is identically zero must be matched exactly.  The tolerance is max(1e-9, 10 eps_ref)
(tests/msk_hessian_cases.py) = 1e-9: the project's first-order bound for this path; nothing of it comes from the
kernels.

Largest scaled error measured on an MI355X per group, both entry points (tolerance 1e-9 each): Ding families at
B = 3 5.8e-11 (the six-muscle marker case, whose reference noise is 6.7e-11; every other Ding case <= 2.8e-12), Hmed
at B = 3 3.7e-10 (hmed_f_rk4_residual; the other Hmed cases <= 9.1e-13), batch parity 1.8e-12, CFX_MSK_HPROJ=1 3.5e-13
(Ding) / 3.7e-10 (Hmed), B = 257 Ding 1.4e-12 / Hmed 1.6e-11, stage-data reuse 1.8e-13 / 3.7e-10, lam = 0 5.8e-16, obj_factor = 0
3.9e-13 / 3.7e-10.

The comparison exposed one kernel error, fixed with it: k_msk_hproj, k_msk_hproj_stage and k_msk_hproj_stage_lds sized
their per-thread column range as NX + pulse widths + residual torques, which leaves out the Hmed2018 intensity
controls, so on every Hmed problem all Hessian entries of the controls past that range (every intensity but the first
NQ, and the residual torques) were never written: scaled error 1.0 before, 3.7e-10 after.

The B = 257 batches are drawn by ``msk_hessian_cases.large_inputs``: on hmed_f_rk4_residual (RK4 at h / tau_c = 4.5)
about 3 % of the random envelope lies at a pole of the right-hand side (K_m + C_N = 0 at a negative stage calcium),
where the CPU oracle's own g is 1e8 .. inf and the kernels, like it, return non-finite second derivatives; those draws
are left out by the oracle's g alone.
"""

import numpy as np
import pytest

from oracle import msk_autodiff as MA
from tests import msk_hessian_cases as HC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _require_gpu():
    from cocofest_amd import _cfx

    lib = _cfx.load_library()  # raises if libcfx.so is missing: no silent fallback
    if lib.cfx_device_count() < 1:
        pytest.fail("no HIP device visible to libcfx")


def _compare(pb, what, got, ref, scale, entry, instances=None):
    tol = HC.tolerance(pb)
    e = MA.hessian_error(pb, got, ref, scale)
    print(f"\n{what} {entry}: {e:.2e}  (tolerance {tol:.0e})")
    if not e <= tol:
        print("\n".join(MA.worst_entries(pb, got, ref, scale, instances)))
    assert e <= tol, f"{what} {entry}: {e:.3e} > {tol:.1e}"
    return e


def _check(pb, h, v, of, lam, what, key=None):
    """Both Hessian entry points of a host AoS handle against the reference; returns the two dense results."""
    ref, scale = HC.reference(key or what, pb, v, of, lam)
    r, c = h.hess_structure()
    got_h = HC.dense(pb.nv, r, c, h.eval_h(v, of, lam))
    got_all = HC.dense(pb.nv, r, c, h.eval_all_h(v, of, lam)[2])
    _compare(pb, what, got_h, ref, scale, "eval_h")
    _compare(pb, what, got_all, ref, scale, "eval_all_h")
    return got_h, got_all


def _run(case, B, what=None, key=None):
    ocp, pb = HC.product(case), HC.problem(case)
    assert (ocp.nx, ocp.nu, ocp.nv) == (pb.nx, pb.nu, pb.nv)
    v, of, lam = HC.inputs(pb, B)
    h = ocp.nlp(batch=B, layout="aos")
    assert (h.nv, h.ng) == (pb.nv, pb.ng)
    try:
        return _check(pb, h, v, of, lam, what or f"{case} B={B}", key or (case, B))
    finally:
        h.close()


@pytest.mark.parametrize("case", list(HC.ALL_CASES))
def test_msk_hessian_exact(case):
    """Every musculoskeletal case at B = 3 (the small-batch path ending in k_msk_hproj_stage_lds): the Ding families,
    Hmed2018 at truncation 10 and 20, joints about x / y, no force-velocity, one and six muscles, one and two
    degrees of freedom, the legacy calcium sum, the fatigue objective, RK4 x 5."""
    _run(case, 3)


@pytest.mark.parametrize("B", [4, 1])
@pytest.mark.parametrize("case", ["cfg5_d07f_rk4", "hmed_biceps_1dof_rk2"])
def test_msk_hessian_exact_batch_parity(case, B):
    """An even batch (the direct-to-LDS staging of the tangent kernel) and a single instance."""
    _run(case, B)


PATH_CASES = ["cfg5_d07f_rk4", "hmed_f_rk4_residual", "arm26_6muscles_d03_rk1"]


@pytest.mark.parametrize("case", PATH_CASES)
def test_msk_hessian_exact_stage_projection_fallback(case, monkeypatch):
    """CFX_MSK_HPROJ=1: k_msk_hproj_stage + k_msk_hproj_sum (the path taken when the staged stages exceed 64 KiB of
    LDS) against the reference, and against the default k_msk_hproj_stage_lds path as before."""
    lds = _run(case, 3)
    monkeypatch.setenv("CFX_MSK_HPROJ", "1")  # read at every launch
    old = _run(case, 3, what=f"{case} CFX_MSK_HPROJ=1")
    for a, b_ in zip(lds, old):
        scale = np.abs(a) + 1e-9 * np.abs(a).max()
        assert np.max(np.abs(a - b_) / scale) < 1e-12


@pytest.mark.parametrize("case", PATH_CASES)
def test_msk_hessian_exact_large_batch(case):
    """B = 257 on SoA device buffers: the large-batch k_msk_hproj (B > 256), the second 256-thread block holding one
    instance.  Instances on both sides of the wave and block edges against the reference; everything finite; the
    small-batch path still gives the same values for those instances."""
    import torch

    ocp, pb = HC.product(case), HC.problem(case)
    B = 257
    v, of, lam = HC.large_inputs(pb, B)  # draws at a pole of the coarse RK step left out, by the CPU oracle alone
    pick = np.array([0, 63, 64, 255, 256])
    ref, scale = HC.reference((case, "large"), pb, v[pick], of[pick], lam[pick])
    h = ocp.nlp(batch=B, layout="soa")
    dev = lambda a: torch.tensor(np.ascontiguousarray(a), device="cuda")  # noqa: E731
    dv, dof, dlam = dev(v.T), dev(of), dev(lam.T)
    hh = h.eval_h(dv, dof, dlam, torch.empty((h.nnz_hess, B), dtype=torch.float64, device="cuda"))
    _, _, fh = h.eval_all_h(dv, dof, dlam)
    torch.cuda.synchronize()
    vals_h, vals_all = hh.cpu().numpy().T, fh.cpu().numpy().T
    r, c = h.hess_structure()
    h.close()
    assert np.all(np.isfinite(vals_h)) and np.all(np.isfinite(vals_all))
    got_h, got_all = HC.dense(pb.nv, r, c, vals_h[pick]), HC.dense(pb.nv, r, c, vals_all[pick])
    _compare(pb, f"{case} B=257", got_h, ref, scale, "eval_h", pick)
    _compare(pb, f"{case} B=257", got_all, ref, scale, "eval_all_h", pick)
    hs = ocp.nlp(batch=len(pick), layout="aos")
    small = hs.eval_h(v[pick].copy(), of[pick].copy(), lam[pick].copy())
    hs.close()
    sc = np.abs(small) + 1e-9 * np.abs(small).max()
    assert np.max(np.abs(vals_h[pick] - small) / sc) < 1e-12


@pytest.mark.parametrize("case,mode", [("cfg5_d07f_rk4", "fused"), ("hmed_f_rk4_residual", "split")])
def test_msk_hessian_exact_stage_data_reuse(case, mode, monkeypatch):
    """cfx_eval_all_h under CFX_MSK_TANGENTS=fused / split: the Hessian that follows g + J_g against the
    reference, not only against eval_h."""
    monkeypatch.setenv("CFX_MSK_TANGENTS", mode)
    _run(case, 3, what=f"{case} CFX_MSK_TANGENTS={mode}")


@pytest.mark.parametrize("case", list(HC.MARKER_CASES))
def test_msk_marker_hessian_exact(case):
    """SUPERIMPOSE_MARKERS rows with multipliers on all rows: the (q_node, q_node) marker terms on top of the
    dynamics curvature, node N included."""
    pb = HC.problem(case)
    assert pb.n_marker_rows > 0
    _run(case, 3)


@pytest.mark.parametrize("case", ["cfg5_d07f_rk4", "d07_rk1_residual", "hmed_f_rk4_residual"])
def test_msk_degenerate_multipliers(case):
    """lam = 0: the objective part alone (positions the reference has as exactly 0 bitwise 0; the fatigue and
    quadratic diagonals to the tolerance).  obj_factor = 0: the constraint part.  Both zero: all zeros."""
    B = 3
    ocp, pb = HC.product(case), HC.problem(case)
    v, of, lam = HC.inputs(pb, B)
    zero, no_obj = np.zeros_like(lam), np.zeros(B)
    h = ocp.nlp(batch=B, layout="aos")
    r, c = h.hess_structure()
    try:
        ref0, _ = HC.reference((case, "lam=0"), pb, v, of, zero)
        assert np.count_nonzero(ref0) > 0
        for entry, vals in (("eval_h", h.eval_h(v, of, zero)), ("eval_all_h", h.eval_all_h(v, of, zero)[2])):
            got = HC.dense(pb.nv, r, c, vals)
            assert np.all(got[ref0 == 0.0] == 0.0), entry
        _check(pb, h, v, of, zero, f"{case} lam=0", (case, "lam=0"))
        _check(pb, h, v, no_obj, lam, f"{case} obj_factor=0", (case, "of=0"))
        assert np.all(h.eval_h(v, no_obj, zero) == 0.0)
        assert np.all(h.eval_all_h(v, no_obj, zero)[2] == 0.0)
    finally:
        h.close()
