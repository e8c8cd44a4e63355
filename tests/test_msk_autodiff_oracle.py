"""The musculoskeletal automatic-differentiation oracle (oracle/msk_autodiff.py, torch float64 on the CPU) pinned to
the numpy oracle (oracle/fes_msk.py), its own rounding noise measured, and the teeth of the comparison that
tests/test_msk_hessian_exact.py makes on the GPU shown on the CPU.  No GPU.

Largest gaps measured between the two oracles over PIN_CASES (both are float64 evaluations of the same formulas; the
bounds asserted are 10x these, a margin for the different summation order of numpy and torch and nothing else):

    g (|Phi| + |x_{k+1}| scale)                          1.5e-14      asserted 1.5e-13
    continuity-Jacobian blocks (|ref| + 1e-9 row max)    1.8e-12      asserted 1.8e-11
    f (relative)                                         1.8e-16      asserted 1.8e-15
    grad f (|ref| + 1e-6 of the largest)                 2.5e-16     asserted 2.5e-15
    marker rows (absolute, metres)                       1.1e-16      asserted 1.1e-15
    marker-row Jacobian (absolute)                       8.3e-17     asserted 8.3e-16

The finite-difference block of test_msk_hessian_matches_oracle (``_lagrangian_block_fd``) against the exact one,
largest |fd - exact| over the block's largest entry: 4.3e-8 (cfg5_d07f_rk4, block max 8.35e9, so 3.6e2 absolute against the old test's 1.7e5) and 4.5e-8
(d07_rk1_residual): that is how loose the old reference was, on top of the
2e-5 the old test grants it.

Mutations of the reference against the unmutated one under ``msk_autodiff.hessian_error`` (GPU tolerance 1e-9):

    (a) force-velocity coefficient linearised (second derivative dropped)   5.0e-1
    (b) cross(w, I w) left out of the inverse dynamics                      9.1e-3    passes the old 2e-5 rule
    (c) two q-group entries of one block swapped                            1.15      passes the old 2e-5 rule
    (d) the fatigue objective's curvature replaced by a constant            3.9

Every test prints its measured figures (pytest -s shows them)."""

import numpy as np
import pytest
import torch

from oracle import fes_msk as M
from oracle import msk_autodiff as MA
from tests import msk_hessian_cases as HC
from tests.test_msk_gpu import _lagrangian_block_fd

PIN_CASES = ["cfg5_d07f_rk4", "d07_rk1_residual", "d07f_passive", "hmed_f_rk4_residual", "rotated_xy_d07f",
             "arm26_6muscles_d03_rk1", "cfg5_legacy", "d07_rk1_mid_xyz_end_y"]

BOUND_G, BOUND_J, BOUND_F, BOUND_GF, BOUND_M, BOUND_MJ = 1.5e-13, 1.8e-11, 1.8e-15, 2.5e-15, 1.1e-15, 8.3e-16

B = 3


def _ngk(pb):
    return pb.nx + pb.n_slide


@pytest.mark.parametrize("case", PIN_CASES)
def test_torch_oracle_matches_numpy_oracle(case):
    pb = HC.problem(case)
    v, _, _ = HC.inputs(pb, B)
    nx, nz, N = pb.nx, pb.nz, pb.n_shooting
    g = MA.eval_g(pb, v)
    ref_g = np.stack([M.eval_g(pb, v[b]) for b in range(B)])
    assert g.shape == ref_g.shape == (B, pb.ng)
    nxt = np.concatenate([np.concatenate([v[:, (k + 1) * nz:(k + 1) * nz + nx], np.full((B, pb.n_slide), 130.0)], axis=1)
                          for k in range(N)], axis=1)
    r0 = N * _ngk(pb)
    eg = float(np.max(np.abs(g[:, :r0] - ref_g[:, :r0]) / (np.abs(ref_g[:, :r0]) + np.abs(nxt))))
    J = MA.continuity_jacobian(pb, v)
    ej = 0.0
    for b, k in ((0, 1), (B - 1, N - 1)):  # the numpy oracle takes nz complex-step integrations per block
        ref = M.continuity_jacobian(pb, v[b], k)
        ej = max(ej, float(np.max(np.abs(J[b, k] - ref) / (np.abs(ref) + 1e-9 * np.max(np.abs(ref), axis=1, keepdims=True)))))
    f, gf = MA.eval_f(pb, v), MA.eval_grad_f(pb, v)
    ef = egf = 0.0
    for b in (0, B - 1):
        rf, rgf = M.eval_f(pb, v[b]), M.eval_grad_f(pb, v[b])
        ef = max(ef, abs(f[b] - rf) / abs(rf))
        egf = max(egf, float(np.max(np.abs(gf[b] - rgf) / (np.abs(rgf) + 1e-6 * np.max(np.abs(rgf))))))
    em = emj = 0.0
    if pb.marker_pairs:
        em = float(np.max(np.abs(g[:, r0:] - ref_g[:, r0:])))
        np.testing.assert_array_equal(MA.marker_rows(pb, v), g[:, r0:])
        Jm = MA.marker_jacobian(pb, v)
        qcols = sorted({pb.nz * c["node"] + pb.nxm + j for c in pb.marker_pairs for j in range(pb.nq)})
        for b in range(B):
            ref = np.zeros((pb.n_marker_rows, pb.nv))
            for c in qcols:
                vv = v[b].astype(complex)
                vv[c] += 1e-30j
                ref[:, c] = np.imag(M.marker_rows(pb, vv)) / 1e-30
            emj = max(emj, float(np.max(np.abs(Jm[b] - ref))))
    print(f"\n{case}: g {eg:.2e}  J blocks {ej:.2e}  f {ef:.2e}  grad f {egf:.2e}  marker rows {em:.2e}  "
          f"marker Jacobian {emj:.2e}")
    assert eg <= BOUND_G and ej <= BOUND_J, (eg, ej)
    assert ef <= BOUND_F and egf <= BOUND_GF, (ef, egf)
    assert em <= BOUND_M and emj <= BOUND_MJ, (em, emj)


@pytest.mark.parametrize("case", ["cfg5_d07f_rk4", "d07_rk1_residual"])
def test_finite_difference_block_against_exact(case):
    """How loose the old reference was: the central-difference block of test_msk_hessian_matches_oracle against the
    exact one, within the 2e-5 of the block's largest entry that the old test allows."""
    pb = HC.problem(case)
    v, of, lam = HC.inputs(pb, B)
    H = MA.hessian_blocks(pb, v, lam)
    b, k = 0, 1
    fd = _lagrangian_block_fd(pb, v[b], lam[b, k * _ngk(pb):k * _ngk(pb) + pb.nx], k)
    gap = float(np.max(np.abs(fd - H[b, k])) / np.max(np.abs(H[b, k])))
    print(f"\n{case}: finite-difference block vs exact {gap:.2e} of the block's largest entry "
          f"({np.max(np.abs(H[b, k])):.2e}); absolute tolerance of the old test {2e-5 * np.max(np.abs(H[b, k])):.2e}")
    assert gap < 2e-5


@pytest.mark.parametrize("case", list(HC.ALL_CASES) + list(HC.MARKER_CASES))
def test_reference_noise(case):
    """eps_ref: forward-over-forward against reverse-over-reverse under the GPU comparison's metric, every case the
    GPU tests use, below the figure recorded in tests/msk_hessian_cases.py."""
    pb = HC.problem(case)
    v, of, lam = HC.inputs(pb, B)
    ref, scale = HC.reference((case, B), pb, v, of, lam)
    ff, rr = MA.lagrangian_hessian(pb, v, of, lam, "ff"), MA.lagrangian_hessian(pb, v, of, lam, "rr")
    eps = MA.hessian_error(pb, ff, rr, scale)
    print(f"\n{case} ({HC.family(pb)} {pb.scheme} x {pb.m}): eps_ref {eps:.2e}  "
          f"fr against rr {MA.hessian_error(pb, ref, rr, scale):.2e}")
    assert eps <= HC.EPS_REF[HC.family(pb), pb.scheme], f"eps_ref {eps:.3e}"
    # the scale dominates the value entry by entry (triangle inequality), to the reference's own noise: value and scale
    # come from two differentiation passes, and an entry fed by one row alone has scale = |value| up to that noise
    excess = np.maximum(np.abs(ref) - scale, 0.0)
    assert MA.hessian_error(pb, scale + excess, scale, scale) <= HC.EPS_REF[HC.family(pb), pb.scheme]
    np.testing.assert_array_equal(ref, ref.transpose(0, 2, 1))


def test_tolerance_is_the_first_order_bound():
    assert all(10 * e <= HC.RTOL * (1 + 1e-12) for e in HC.EPS_REF.values())
    assert HC.tolerance(HC.problem("hmed_rk1_t20")) == 1e-9
    assert HC.tolerance(HC.problem("arm26_6muscles_reach")) == pytest.approx(1e-9, rel=1e-12)


@pytest.mark.parametrize("case", ["cfg5_d07f_rk4", "hmed_f_rk4_residual", "arm26_6muscles_d03_rk1"])
def test_large_batch_inputs_are_in_the_regular_regime(case):
    """The B = 257 batches of the GPU test: 257 of 514 draws remain, the oracle's g is below G_REGULAR on them and the
    reference Hessian of the compared instances is finite; the draws left out are printed."""
    pb = HC.problem(case)
    v, of, lam = HC.large_inputs(pb, 257)
    v2, _, _ = HC.inputs(pb, 514)
    with np.errstate(all="ignore"):
        g2 = np.abs(MA.eval_g(pb, v2)).max(axis=1)
    out = ~(np.isfinite(g2) & (g2 < HC.G_REGULAR))
    print(f"\n{case}: {out.sum()} of 514 draws left out, largest finite |g| among them "
          f"{np.max(g2[out & np.isfinite(g2)], initial=0.0):.2e}, {np.sum(~np.isfinite(g2))} not finite")
    assert v.shape == (257, pb.nv) and np.abs(MA.eval_g(pb, v)).max() < HC.G_REGULAR
    pick = np.array([0, 63, 64, 255, 256])
    ref, scale = HC.reference((case, "large"), pb, v[pick], of[pick], lam[pick])
    assert np.all(np.isfinite(ref)) and np.all(np.isfinite(scale))


def test_passive_clip_kink_is_not_sampled():
    """The passive-force clip has a kink at normalised length 1: no RK stage input of d07f_passive comes within 1e-6
    of it, so the reference differentiates a smooth function there."""
    pb = HC.problem("d07f_passive")
    assert pb.fp_on
    v, _, _ = HC.inputs(pb, B)
    nl = MA.normalised_lengths(pb, v)
    assert nl.size == B * pb.n_shooting * 4 * len(pb.muscles)
    print(f"\nd07f_passive: normalised lengths {nl.min():.3f} .. {nl.max():.3f}, closest to 1: {np.min(np.abs(nl - 1)):.2e}")
    assert np.min(np.abs(nl - 1)) > 1e-6
    assert nl.min() < 1 < nl.max()  # both sides of the clip are exercised


def test_zero_multipliers_leave_the_objective_and_sliding_rows_contribute_nothing():
    pb = HC.problem("hmed_f_rk4_residual")
    assert pb.n_slide and pb.fatigue_weight
    v, of, lam = HC.inputs(pb, B)
    H0 = MA.lagrangian_hessian(pb, v, of, np.zeros_like(lam))
    idx = np.arange(pb.nv)
    off = H0.copy()
    off[:, idx, idx] = 0.0
    assert np.all(off == 0.0)
    block, group = MA.variable_groups(pb)
    a_n = np.flatnonzero((block == pb.n_shooting) & (group == MA.GROUPS.index("A")))
    for b in range(B):  # 6 w a_rest^2 / A^4, differentiated by torch, against the closed form
        expect = of[b] * 6 * pb.fatigue_weight * np.array([m.c["a_rest"] for m in pb.muscles]) ** 2 / v[b, a_n] ** 4
        np.testing.assert_allclose(H0[b, a_n, a_n], expect, rtol=1e-14)
    lam2 = lam.copy()
    body = lam2[:, : pb.n_shooting * _ngk(pb)].reshape(B, pb.n_shooting, _ngk(pb))
    body[:, :, pb.nx:] = 7.0
    np.testing.assert_array_equal(MA.lagrangian_hessian(pb, v, of, lam2), HC.reference(("hmed_f_rk4_residual", B), pb, v, of, lam)[0])


def test_mutations_of_the_reference_are_caught(monkeypatch):
    """Four deliberate errors, each applied to the reference and compared with the unmutated one at the GPU
    tolerance.  (b) and (c) pass the rule of test_msk_hessian_matches_oracle (2e-5 of the block's largest entry, on
    the two blocks it looks at) and fail the new comparison."""
    case = "cfg5_d07f_rk4"
    pb = HC.problem(case)
    v, of, lam = HC.inputs(pb, B)
    good, scale = HC.reference((case, B), pb, v, of, lam)
    tol = HC.tolerance(pb)
    old_blocks = ((0, 1), (B - 1, pb.n_shooting - 1))
    nz, N = pb.nz, pb.n_shooting
    assert MA.hessian_error(pb, good, good, scale) == 0.0
    rr = MA.lagrangian_hessian(pb, v, of, lam, "rr")
    assert MA.hessian_error(pb, rr, good, scale) <= tol

    def old_rule(mut):
        return all(HC.old_rule_passes(pb, mut, good, b, k) for b, k in old_blocks)

    fv = MA.force_velocity

    # (b) cross(w, I w) left out of the inverse dynamics
    monkeypatch.setattr(MA, "_gyroscopic", lambda w, Iw: 0.0 * w)
    e_b_mut = MA.lagrangian_hessian(pb, v, of, lam, "rr")
    monkeypatch.undo()
    e_b, old_b = MA.hessian_error(pb, e_b_mut, good, scale), old_rule(e_b_mut)

    # (a) the force-velocity coefficient linearised at the point: value and first derivative (g, J_g) unchanged
    J_before = MA.continuity_jacobian(pb, v)
    monkeypatch.setattr(MA, "force_velocity", lambda vel: _linear_fv(fv, vel))
    J_after = MA.continuity_jacobian(pb, v)
    np.testing.assert_allclose(J_after, J_before, rtol=1e-12, atol=1e-14 * np.abs(J_before).max())
    e_a = MA.hessian_error(pb, MA.lagrangian_hessian(pb, v, of, lam, "rr"), good, scale)
    monkeypatch.undo()

    # (c) two q-group entries of one block swapped: (q0, q0) and (q1, q1) of interval 1, instance 0
    block, group = MA.variable_groups(pb)
    q = np.flatnonzero((block == 1) & (group == MA.GROUPS.index("q")))
    assert len(q) == 2
    swapped = good.copy()
    swapped[0, q[0], q[0]], swapped[0, q[1], q[1]] = good[0, q[1], q[1]], good[0, q[0], q[0]]
    e_c, old_c = MA.hessian_error(pb, swapped, good, scale), old_rule(swapped)

    # (d) the fatigue objective's curvature replaced by a constant: 6 w / a_rest^2, its value at A = a_rest
    a_n = np.flatnonzero((block == N) & (group == MA.GROUPS.index("A")))
    const = good.copy()
    a_rest = np.array([m.c["a_rest"] for m in pb.muscles])
    for b in range(B):
        exact = of[b] * 6 * pb.fatigue_weight * a_rest ** 2 / v[b, a_n] ** 4
        const[b, a_n, a_n] += of[b] * 6 * pb.fatigue_weight / a_rest ** 2 - exact
    e_d = MA.hessian_error(pb, const, good, scale)
    s = slice(nz, 2 * nz)
    print(f"\nmutations (tolerance {tol:.0e}): (a) fv'' dropped {e_a:.2e}  (b) no cross(w, I w) {e_b:.2e} "
          f"(old rule passes: {old_b})  (c) swapped q entries {e_c:.2e} (old rule passes: {old_c})  "
          f"(d) constant fatigue curvature {e_d:.2e};  block (0, 1): largest entry {np.max(np.abs(good[0, s, s])):.2e}, "
          f"largest q x q entry {np.max(np.abs(good[0][np.ix_(q, q)])):.2e}")
    assert min(e_a, e_b, e_c, e_d) > 1e3 * tol
    assert old_b and old_c


def _linear_fv(fv, velocity):
    """force_velocity with its second derivative dropped: fv(v0) + fv'(v0) (v - v0), v0 the detached input."""
    at = velocity.detach()
    d1, d2, d3 = -0.318, -8.149, -0.374
    u = d2 * (at / 10) + d3
    slope = d1 * (d2 / 10) / torch.sqrt(u * u + 1)
    return fv(at) + slope * (velocity - at)
