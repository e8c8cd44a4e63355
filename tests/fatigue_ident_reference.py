"""Exact-AD reference of the fatigue-parameter identification — TEST INFRASTRUCTURE ONLY (CPU, torch float64).

The single-shooting trajectory of a ``*_with_fatigue`` model from the five-state fatigue rest state
[0, 0, A_rest (Ding2007: a_scale), tau1_rest, km_rest] is rolled out as a function of the identified fatigue
parameters theta (keys among alpha_a, alpha_tau1, alpha_km, tau_fat) with ``oracle.fes_autodiff.rhs`` and ``_step``
unchanged (the four constants enter ``rhs`` as tensors), and differentiated with ``torch.func.jacfwd`` (``jacrev``
for the reference-noise measurement).  Everything else (``forces``, ``forces_and_sens``, ``normal``,
``lm_reference``, ``scaled_errors``) is ``tests/ident_reference.py``'s, on this rollout.
"""

from __future__ import annotations

import torch

from oracle import fes_autodiff as AD
from tests.ident_reference import F64, Setup, lm_reference, scaled_errors  # noqa: F401  (re-exported for the tests)

FATIGUE_KEYS = ["alpha_a", "alpha_tau1", "alpha_km", "tau_fat"]


class FatigueSetup(Setup):
    """One experiment on a fatigue model; ``name`` is the oracle's model name (``ding2003_with_fatigue`` ...)."""

    def __init__(self, name, *args, **kwargs):
        if not name.endswith("with_fatigue"):
            raise ValueError(f"{name} has no fatigue states")
        super().__init__(name, *args, **kwargs)

    def rest_state(self):
        a = self.c["a_scale"] if self.name.startswith("ding2007") else self.c["a_rest"]
        return torch.tensor([0.0, 0.0, a, self.c["tau1_rest"], self.c["km_rest"]], dtype=F64)

    def trajectory(self, keys):
        """theta (n_id,) -> node forces (N + 1,)."""
        h = self.dt / self.m
        x0 = self.rest_state()

        def traj(theta):
            c = dict(self.c)
            for j, k in enumerate(keys):
                c[k] = theta[j]
            x = x0 + 0.0 * theta[0]
            out = [x[1]]
            for k in range(self.N):
                u = None if self.controls is None else self.controls[k]
                row = self.rows[k]
                f = lambda t, xx: AD.rhs(self.name, c, t, xx, u, row)  # noqa: E731
                for j in range(self.m):
                    x = AD._step(self.scheme, f, k * self.dt + j * h, h, x)
                out.append(x[1])
            return torch.stack(out)

        return traj
