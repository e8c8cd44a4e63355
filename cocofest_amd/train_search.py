"""TrainSearch: choose the stimulation train itself.

``OcpFes`` optimises pulse widths and intensities on a fixed train; the train (frequency, doublets or triplets,
truncation, one constant width or intensity) is a discrete choice.  ``TrainSearch`` builds the Cartesian grid of
candidates, integrates and scores all of them against a target force in one launch (``IvpSweep.score``,
``cfx_sweep_score``) and ranks them, optionally under bounds on the final fatigue states or on the metrics.
"""

from __future__ import annotations

import itertools
from fractions import Fraction

import numpy as np

from .fes_models import DingModelPulseIntensityFrequency, DingModelPulseWidthFrequency
from .ivp import IvpSweep


class TrainSearchResult:
    """The candidate table of a ``TrainSearch`` with the arrays of ``IvpSweep.score`` (final states and metrics),
    each ``(n_candidates,)`` in the order of ``candidates``."""

    def __init__(self, candidates: list, scores: dict):
        self.candidates = candidates
        self.scores = {k: np.asarray(v) for k, v in scores.items()}
        for k, v in self.scores.items():
            if v.shape != (len(candidates),):
                raise ValueError(f"scores[{k!r}] must have shape ({len(candidates)},)")

    def __getitem__(self, key):
        return self.scores[key]

    def feasible(self, subject_to=None) -> np.ndarray:
        """Mask of the candidates inside every ``(lo, hi)`` of ``subject_to`` (None: unbounded on that side)."""
        mask = np.ones(len(self.candidates), dtype=bool)
        for key, bounds in (subject_to or {}).items():
            if key not in self.scores:
                raise ValueError(f"subject_to: unknown key {key!r}, the available keys are {sorted(self.scores)}")
            lo, hi = bounds
            if lo is not None:
                mask &= self.scores[key] >= lo
            if hi is not None:
                mask &= self.scores[key] <= hi
        return mask

    def ranking(self, metric: str = "track", subject_to=None) -> np.ndarray:
        """Indices of the feasible candidates with a finite ``metric``, smallest first (ties: grid order)."""
        if metric not in self.scores:
            raise ValueError(f"unknown metric {metric!r}, the available keys are {sorted(self.scores)}")
        values = self.scores[metric]
        keep = np.flatnonzero(self.feasible(subject_to) & np.isfinite(values))
        return keep[np.argsort(values[keep], kind="stable")]

    def row(self, index: int) -> dict:
        """Candidate ``index`` with its scores: {"index", the candidate's keys, every state and metric}."""
        index = int(index)
        return {"index": index, **self.candidates[index], **{k: v[index].item() for k, v in self.scores.items()}}

    def best(self, metric: str = "track", subject_to=None) -> dict:
        """The feasible candidate with the smallest ``metric`` (``row``); ``ValueError`` if none is feasible."""
        order = self.ranking(metric, subject_to)
        if order.size == 0:
            raise ValueError(f"no candidate satisfies the constraints {subject_to}")
        return self.row(order[0])


class TrainSearch:
    """Grid search over stimulation trains of one model.

    Candidates are the Cartesian product ``frequencies`` x ``pulse_modes`` x ``values`` x ``truncations`` (the last
    varies fastest).  A candidate's base train is ``[round(i / f, 3) for i in range(n)]`` with every pulse before
    ``final_time``; ``values`` are constant pulse widths (Ding2007) or intensities (Hmed2018) and must be None for
    Ding2003 (None otherwise: ``IvpFes``'s default); ``truncations`` None: the model's ``sum_stim_truncation``;
    ``n_shooting`` None: ``OcpFes.prepare_n_shooting`` per candidate.  The batch is packed by
    ``IvpSweep.from_trains``: no ``IvpFes`` is built."""

    def __init__(self, model, final_time, frequencies, pulse_modes=("single",), values=None, truncations=None,
                 n_shooting=None, ode_solver=None, device: int = 0):
        frequencies, pulse_modes = list(frequencies), list(pulse_modes)
        if not frequencies or not pulse_modes:
            raise ValueError("frequencies and pulse_modes must not be empty")
        for f in frequencies:
            if isinstance(f, bool) or not isinstance(f, int | float) or not f > 0:
                raise ValueError("frequencies must be positive numbers")
        self.value_key = None
        if isinstance(model, DingModelPulseWidthFrequency):
            self.value_key = "pulse_width"
        elif isinstance(model, DingModelPulseIntensityFrequency):
            self.value_key = "pulse_intensity"
        if values is not None and self.value_key is None:
            raise ValueError(f"values given for {type(model).__name__}, which has no pulse width or intensity")
        values = [None] if values is None else list(values)
        truncations = [None] if truncations is None else list(truncations)
        if not values or not truncations:
            raise ValueError("values and truncations must not be empty")
        self.model, self.final_time = model, final_time
        self.candidates, trains = [], []
        tf = Fraction(final_time).limit_denominator()
        for f, mode, value, T in itertools.product(frequencies, pulse_modes, values, truncations):
            q = tf * Fraction(f).limit_denominator()
            n = -((-q.numerator) // q.denominator)  # pulses with i / f < final_time
            T = model._sum_stim_truncation if T is None else T
            candidate = {"frequency": f, "pulse_mode": mode, "sum_stim_truncation": T}
            train = {"stim_time": [round(i / f, 3) for i in range(n)], "final_time": final_time,
                     "n_shooting": n_shooting, "pulse_mode": mode, "sum_stim_truncation": T}
            if self.value_key is not None and value is not None:
                candidate[self.value_key] = train[self.value_key] = value
            self.candidates.append(candidate)
            trains.append(train)
        try:
            self.sweep = IvpSweep.from_trains(model, trains, ode_solver=ode_solver, device=device)
        except (TypeError, ValueError, IndexError) as e:
            raise type(e)(str(e).replace("trains[", "candidates[", 1)) from None
        self.result = None

    def run(self, target, sample_dt=None) -> TrainSearchResult:
        """Score every candidate against ``target`` (a scalar, or samples every ``sample_dt``) in one launch."""
        self.result = TrainSearchResult(self.candidates, self.sweep.score(target, sample_dt))
        return self.result

    def best(self, metric: str = "track", subject_to=None) -> dict:
        """``TrainSearchResult.best`` of the last ``run``."""
        if self.result is None:
            raise ValueError("run(target) first")
        return self.result.best(metric, subject_to)

    def close(self):
        self.sweep.close()
