"""Shapes, inputs and tolerances shared by tests/test_autodiff_oracle.py (CPU) and tests/test_hessian_exact.py
(GPU): the problems on which the Lagrangian Hessian is compared with the automatic-differentiation oracle
(oracle/fes_autodiff.py).

Tolerance of the GPU comparison: max(RTOL, 10 * EPS_REF[family, scheme]).  RTOL is the project's first-order bound
(1e-11; 1e-10 from 40 RK stages per interval on, tests/test_gpu_parity.py).  EPS_REF is the reference's own rounding
noise, measured on the CPU alone as the gap between the forward-over-forward and the reverse-over-reverse Hessian of
the same inputs under ``fes_autodiff.hessian_error``; test_autodiff_oracle.py re-measures it on every run and fails
if it exceeds the figure recorded here.  Largest measured values (float64, all cases of that row):

    family  scheme     measured     recorded EPS_REF
    ding    RK1        2.0e-15      1e-14
    ding    RK2        2.0e-15      1e-14
    ding    RK4        9.0e-16      1e-14
    hmed    RK1        3.0e-15      1e-13
    hmed    RK2        1.4e-14      1e-13      (T = 17 with fatigue: 1.4e-14; T = 32: 4.6e-15; T = 3: 9.9e-15)
    hmed    RK4        1.6e-15      1e-13      (T = 32, m = 2: 1.6e-15, with fatigue 8.3e-16)
    ding    legendre   3.0e-15      1e-14      (degree 9: 1.0e-15)
    ding    radau      2.5e-15      1e-14
    hmed    legendre   2.6e-15      1e-13      (degree 9: 1.4e-15)
    hmed    radau      3.2e-15      1e-13      (degree 2, T = 32: 3.2e-15)

so 10 * EPS_REF <= 1e-12 < RTOL everywhere and every GPU case is held to RTOL = 1e-11 (no case here reaches 40
stages per interval).
"""

import numpy as np

from oracle import fes_collocation as CO
from oracle import fes_oracle as O
from tests import cases

RTOL = 1e-11

EPS_REF = {(fam, s): (1e-14 if fam == "ding" else 1e-13)
           for fam in ("ding", "hmed") for s in ("RK1", "RK2", "RK4", "legendre", "radau")}


def family(name):
    return "hmed" if name.startswith("hmed2018") else "ding"


def n_stages(pb):
    return 0 if isinstance(pb, CO.ColProblem) else cases.SCHEMES[pb.scheme] * pb.n_steps


def tolerance(pb):
    scheme = pb.method if isinstance(pb, CO.ColProblem) else pb.scheme
    rtol = 1e-10 if n_stages(pb) >= 40 else RTOL
    return max(rtol, 10 * EPS_REF[family(pb.name), scheme])


_T = np.linspace(0, 1, 30)
TRACKING = {"force_tracking": [_T, 60 * np.sin(np.pi * _T) ** 2], "end_node_tracking": 50}
SHOOT_STIMS = [0.0, 0.02, 0.04, 0.06]
TRAIN12 = [round(0.02 * i, 2) for i in range(12)]
COL_STIMS = [0.0, 0.1, 0.2, 0.3, 0.4]
COL_OBJECTIVE = {"end_node_tracking": 40.0}


def shooting_cfg(name, scheme, T=3, m=2):
    """The shape of test_lagrangian_hessian_vs_oracle: 4 pulses 20 ms apart, force tracking + end node."""
    return dict(name=name, stims=SHOOT_STIMS, final_time=0.08, truncation=T, scheme=scheme, m=m, objective=TRACKING)


def bucket_cfg(name, T, scheme="RK2"):
    """The 12-pulse train of test_hmed_truncation_buckets (12 intervals; the CPU reference takes under 2 s at
    T = 32 under RK4, so the horizon is not cut)."""
    return dict(name=name, stims=TRAIN12, final_time=0.24, truncation=T, scheme=scheme, m=2, objective=TRACKING)


def edge_cfg(name):
    """test_edge_sizes: N = 1, T = 1, RK4 x 1."""
    return dict(name=name, stims=[0.0], final_time=0.1, truncation=1, scheme="RK4", m=1, objective=TRACKING)


def collocation_problem(name, degree, method, T=4, n_shooting=3):
    base = cases.oracle_problem(name, COL_STIMS, 0.5, T, scheme="RK1", m=1, n_shooting=n_shooting,
                                objective=COL_OBJECTIVE)
    return CO.ColProblem(**{f: getattr(base, f) for f in base.__dataclass_fields__}, degree=degree, method=method)


def multipliers(pb, B, seed=5):
    """Random normal multipliers over all rows (sliding-window rows included) and obj_factor in [0.5, 2]."""
    rng = np.random.default_rng(seed)
    return rng.normal(size=(B, pb.ng)), rng.uniform(0.5, 2.0, B)


def decision(pb, B, seed=4):
    if isinstance(pb, CO.ColProblem):
        return cases.random_collocation_decision(pb, B, seed)
    return cases.random_decision(pb, B, seed)


_REF = {}


def reference(key, pb, v, of, lam):
    """(values, scale) of the AD oracle, computed once per key and shared (read-only) among the tests."""
    from oracle import fes_autodiff as AD

    if key not in _REF:
        ref, scale = AD.hessian_values(pb, v, of, lam), AD.hessian_scale(pb, v, of, lam)
        ref.setflags(write=False)
        scale.setflags(write=False)
        _REF[key] = (ref, scale)
    return _REF[key]
