"""Cases, inputs, the recorded reference noise and the tolerance shared by tests/test_msk_autodiff_oracle.py (CPU)
and tests/test_msk_hessian_exact.py (GPU): the musculoskeletal problems on which the Lagrangian Hessian is compared
with the automatic-differentiation oracle (oracle/msk_autodiff.py).

Tolerance of the GPU comparison: max(RTOL, 10 * EPS_REF[family, scheme]) under ``msk_autodiff.hessian_error``.  RTOL
= 1e-9 is the project's first-order bound for this path (the J_g bound of tests/test_msk_gpu.py: dual numbers against
a different mass-matrix formulation).  EPS_REF is the reference's own rounding noise, measured on the CPU alone as the
gap between the forward-over-forward and the reverse-over-reverse Hessian of the same inputs (B = 3, every interval,
the node-N block); test_msk_autodiff_oracle.py re-measures it on every run and fails if it exceeds the figure recorded
here.  Largest measured values (float64; every case of ``ALL_CASES`` and ``MARKER_CASES`` of that row):

    family  scheme   measured    recorded EPS_REF
    ding    RK1      6.7e-11     1e-10     (arm26_6muscles_reach, six muscles with marker rows; every other case
                                            <= 2.3e-13: arm26_6muscles_d03_rk1 2.2e-13, d07_rk1_residual 1.3e-13)
    ding    RK2      2.3e-14     1e-13     (d07f_rk2)
    ding    RK4      2.7e-13     1e-12     (d03f_rk4_nofv; biceps_1dof_d07f 1.7e-13; RK4 x 5 1.4e-14)
    hmed    RK1      9.1e-14     1e-13     (truncation 20)
    hmed    RK2      1.3e-14     1e-13
    hmed    RK4      1.3e-13     1e-12

so 10 * EPS_REF <= RTOL everywhere and every GPU case is held to 1e-9.
"""

import numpy as np

from tests import msk_cases as MC
from tests.test_msk_gpu import CASES, MARKER_CASES  # noqa: F401  (unchanged; shared with the parity tests)

RTOL = 1e-9

EPS_REF = {("ding", "RK1"): 1e-10, ("ding", "RK2"): 1e-13, ("ding", "RK4"): 1e-12,
           ("hmed", "RK1"): 1e-13, ("hmed", "RK2"): 1e-13, ("hmed", "RK4"): 1e-12}

# every entry of CASES plus RK4 x 5 (20 stages per interval, the 16-instance blocks of the stage kernels)
ALL_CASES = dict(CASES, cfg5_rk4x5=MC.cfg5(m=5))

SEED = 3  # d07f_passive: no stage input within 1e-6 of the passive clip's kink (test_msk_autodiff_oracle.py)


def family(pb):
    return "hmed" if pb.muscles[0].model.startswith("hmed2018") else "ding"


def tolerance(pb):
    return max(RTOL, 10 * EPS_REF[family(pb), pb.scheme])


def problem(case):
    """The oracle problem of a name in ALL_CASES or MARKER_CASES (the latter with its marker rows)."""
    if case in MARKER_CASES:
        cfg, markers = MARKER_CASES[case]
        return MC.oracle_problem(**cfg, markers=markers)
    return MC.oracle_problem(**ALL_CASES[case])


def product(case):
    if case in MARKER_CASES:
        cfg, markers = MARKER_CASES[case]
        return MC.product_ocp(**cfg, markers=markers)
    return MC.product_ocp(**ALL_CASES[case])


def inputs(pb, B, seed=SEED):
    """Decision vectors, random normal multipliers on every row (sliding-window and marker rows included) and
    obj_factor in [0.5, 2].  At B = 3 the decision vectors and multipliers are those of
    test_msk_hessian_matches_oracle, so the figures of the two comparisons are of the same blocks."""
    v = MC.random_decision(pb, B, seed=seed)
    rng = np.random.default_rng(seed + 1)
    lam = rng.normal(size=(B, pb.ng))
    return v, rng.uniform(0.5, 2.0, B), lam


G_REGULAR = 1e6


def large_inputs(pb, B, seed=SEED):
    """``inputs`` for a large batch, restricted to the regime in which the problem is a function at all.  The random
    envelope of msk_cases.random_decision is wider than the stable range of a coarse RK step (at
    h / tau_c > 1 a stage calcium goes negative, and K_m + C_N then passes through 0, a pole of the right-hand side):
    on hmed_f_rk4_residual about 3 % of the draws put the numpy and the torch oracle's own g at 1e8 .. inf, and no
    implementation returns finite second derivatives there.  So 2 B instances are drawn and the first B kept whose
    constraint vector, evaluated by the CPU oracle alone (msk_autodiff.eval_g), is finite and below G_REGULAR = 1e6
    (its median over the draws is 4e2 .. 1e3, the largest of the Ding cases 6e4).  Nothing of the choice comes from
    the kernels; test_msk_autodiff_oracle.py checks that B instances remain and that the reference is finite on them."""
    from oracle import msk_autodiff as MA

    v, of, lam = inputs(pb, 2 * B, seed)
    with np.errstate(all="ignore"):
        g = np.abs(MA.eval_g(pb, v)).max(axis=1)
    keep = np.flatnonzero(np.isfinite(g) & (g < G_REGULAR))[:B]
    assert len(keep) == B, f"only {len(keep)} of {2 * B} draws are in the regular regime"
    return v[keep], of[keep], lam[keep]


def dense(nv, r, c, values):
    """The product's (row, col, value) triplets of a batch as dense symmetric matrices (B, nv, nv): repeated pairs
    summed, the lower triangle mirrored."""
    r, c, values = np.asarray(r), np.asarray(c), np.asarray(values)
    H = np.zeros((values.shape[0], nv, nv))
    for b in range(values.shape[0]):
        np.add.at(H[b], (r, c), values[b])
        off = r != c
        np.add.at(H[b], (c[off], r[off]), values[b][off])
    return H


_REF = {}


def reference(key, pb, v, of, lam):
    """(dense Hessian, scale) of the AD oracle, computed once per key and shared (read-only) among the tests."""
    from oracle import msk_autodiff as MA

    if key not in _REF:
        ref, scale = MA.lagrangian_hessian(pb, v, of, lam), MA.lagrangian_hessian_scale(pb, v, of, lam)
        ref.setflags(write=False)
        scale.setflags(write=False)
        _REF[key] = (ref, scale)
    return _REF[key]


def old_rule_passes(pb, got, ref, b, k):
    """The rule of test_msk_hessian_matches_oracle on interval block k of instance b: max |got - ref| < 2e-5 max |ref|
    over the block."""
    s = slice(k * pb.nz, (k + 1) * pb.nz)
    return bool(np.max(np.abs(got[b, s, s] - ref[b, s, s])) < 2e-5 * np.max(np.abs(ref[b, s, s])))

