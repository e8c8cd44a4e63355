"""IvpFes: forward simulation of an FES model (reference: cocofest/integration/ivp_fes.py).

Same constructor dictionaries, defaults, pulse modes and validation messages as the reference.  The
integration itself (single shooting, every RK sub-step returned) runs on the GPU through
``cfx_integrate``; batches of independent instances use :meth:`IvpFes.handle`.  With
``OdeSolver.COLLOCATION`` the same call runs the implicit collocation integrator: every interval's node
state and collocation states are returned.

``IvpSweep`` integrates a list of ``IvpFes`` objects of one model in a single launch (``cfx_sweep_integrate``):
every instance keeps its own stimulation train, truncation, ``n_shooting`` and ``final_time``.
"""

from __future__ import annotations

from fractions import Fraction

import numpy as np

from . import _cfx
from .fes_models import (
    DingModelPulseIntensityFrequency,
    DingModelPulseIntensityFrequencyWithFatigue,
    DingModelPulseWidthFrequency,
    DingModelPulseWidthFrequencyWithFatigue,
    FesModel,
    PLACEHOLDER_INTENSITY,
    PLACEHOLDER_TIME,
)
from .ocp import OcpFes
from .ode_solver import OdeSolver


class IvpFes:
    def __init__(self, fes_parameters: dict = None, ivp_parameters: dict = None):
        self._fill_fes_dict(fes_parameters)
        self._fill_ivp_dict(ivp_parameters)
        self.dictionaries_check()

        self.model = self.fes_parameters["model"]
        self.stim_time = self.model.stim_time
        self.n_stim = len(self.stim_time)
        self.pulse_width = self.fes_parameters["pulse_width"]
        self.pulse_intensity = self.fes_parameters["pulse_intensity"]
        self.final_time = self.ivp_parameters["final_time"]
        # extension: ivp_parameters["n_shooting"] sets the node count (the reference always takes the LCM rule of
        # OcpFes.prepare_n_shooting, ivp_fes.py:73), e.g. BASELINE configs[0]'s n_shooting = 20 for 10 pulses
        self._n_shooting_given = self.ivp_parameters["n_shooting"]
        self.n_shooting = self._n_shooting_given or OcpFes.prepare_n_shooting(self.stim_time, self.final_time)
        self.pulse_mode = self.fes_parameters["pulse_mode"]
        self._pulse_mode_settings()
        self.dt = np.array([self.final_time / self.n_shooting])

        self.controls_keys = None
        if isinstance(self.model, DingModelPulseWidthFrequency):
            self.controls_keys = ["last_pulse_width"]
        if isinstance(self.model, DingModelPulseIntensityFrequency):
            self.controls_keys = ["pulse_intensity"]

        table, self.stim_idx_at_node_list = self.model.get_numerical_data_time_series(self.n_shooting,
                                                                                      self.final_time)
        self.stim_rows = table["stim_time"][:, 0, :].T.copy()
        self.controls = self._build_controls()
        self.ode_solver = self.ivp_parameters["ode_solver"]
        self.n_threads = self.ivp_parameters["n_threads"]

    # ---- dictionaries (ivp_fes.py:113-230) ----------------------------------------------------------
    def _fill_fes_dict(self, fes_parameters):
        default = {"model": FesModel, "stim_time": None, "pulse_width": 0.0003, "pulse_intensity": 50,
                   "pulse_mode": "single"}
        fes_parameters = {} if fes_parameters is None else fes_parameters
        for key in default:
            if key not in fes_parameters:
                fes_parameters[key] = default[key]
        self.fes_parameters = fes_parameters

    def _fill_ivp_dict(self, ivp_parameters):
        default = {"final_time": None, "ode_solver": OdeSolver.RK4(n_integration_steps=10), "n_threads": 1,
                   "n_shooting": None}
        ivp_parameters = {} if ivp_parameters is None else ivp_parameters
        for key in default:
            if key not in ivp_parameters:
                ivp_parameters[key] = default[key]
        self.ivp_parameters = ivp_parameters

    def dictionaries_check(self):
        fes, ivp = self.fes_parameters, self.ivp_parameters
        if not isinstance(fes, dict):
            raise ValueError("fes_parameters must be a dictionary")
        if not isinstance(ivp, dict):
            raise ValueError("ivp_parameters must be a dictionary")
        if not isinstance(fes["model"], FesModel):
            raise TypeError("model must be a FesModel type")
        check_pulse_values(fes["model"], fes["pulse_width"], fes["pulse_intensity"])
        if not isinstance(fes["pulse_mode"], str):
            raise ValueError("pulse_mode must be a string type")
        if not isinstance(ivp["final_time"], int | float):
            raise ValueError("final_time must be an int or float type")
        if not isinstance(ivp["ode_solver"], (OdeSolver.RK1, OdeSolver.RK2, OdeSolver.RK4, OdeSolver.COLLOCATION)):
            raise ValueError("ode_solver must be a OdeSolver type")
        if not isinstance(ivp["n_threads"], int):
            raise ValueError("n_thread must be a int type")
        ns = ivp["n_shooting"]
        if ns is not None and (isinstance(ns, bool) or not isinstance(ns, int) or ns < 1):
            raise ValueError("n_shooting must be a positive int (or None for the stimulation-time LCM rule)")

    def _pulse_mode_settings(self):
        """Doublets / triplets add pulses 5 and 10 ms after each one and write the list back into the model
        (ivp_fes.py:232-256; the write-back is the reference's behaviour)."""
        if self.pulse_mode == "single":
            return
        self.stim_time = expand_pulse_mode(self.stim_time, self.pulse_mode)
        self.model.stim_time = self.stim_time
        self.n_stim = len(self.stim_time)
        if self._n_shooting_given is None:
            self.n_shooting = OcpFes.prepare_n_shooting(self.stim_time, self.final_time)

    def _build_controls(self):
        """Per-interval controls, (nu, N).  Ding2007: width of the last pulse at or before the node
        (ivp_fes.py:344-351).  Hmed2018: the T intensities aligned with the node's stim row, history
        placeholders at 50 mA (equal to ivp_fes.py:324-342 whenever N == n_stim)."""
        N = self.n_shooting
        if isinstance(self.model, DingModelPulseWidthFrequency):
            pw = self.pulse_width
            if isinstance(pw, list) and len(pw) != 1:
                vals = [pw[self.stim_idx_at_node_list[k][-1]] for k in range(N)]
            else:
                vals = [pw[0] if isinstance(pw, list) else pw] * N
            return np.array([vals], dtype=float)
        if isinstance(self.model, DingModelPulseIntensityFrequency):
            T = self.model._sum_stim_truncation
            src = self.model._last_table_src
            n_prefix = len(self.model.previous_stim["time"])
            pi = self.pulse_intensity
            out = np.empty((T, N))
            for k in range(N):
                for j in range(T):
                    s = src[k, j] - n_prefix
                    if s < 0:
                        out[j, k] = PLACEHOLDER_INTENSITY
                    elif isinstance(pi, list):
                        out[j, k] = pi[s] if len(pi) != 1 else pi[0]
                    else:
                        out[j, k] = pi
            return out
        return np.zeros((0, N))

    # ---- integration ---------------------------------------------------------------------------------
    def handle(self, batch: int = 1, layout: str = "aos", device: int = 0) -> _cfx.Handle:
        return _cfx.Handle(model_id=self.model.cfx_model_id, constants=self.model.cfx_constants(),
                           scheme=self.ode_solver.scheme, n_steps=self.ode_solver.n_integration_steps,
                           n_shooting=self.n_shooting, truncation=self.model._sum_stim_truncation,
                           final_time=float(self.final_time), stim_rows=self.stim_rows, batch=batch,
                           layout=_cfx.LAYOUT_AOS if layout == "aos" else _cfx.LAYOUT_SOA, device=device)

    def integrate(self, shooting_type=None, integrator=None, to_merge=None, return_time=True,
                  duplicated_times=False):
        """Single-shooting integration from the rest state; returns {state: (1, N*m+1)} (and the time).

        ``OdeSolver.COLLOCATION`` (degree d): {state: (1, N*(d+1)+1)} — per interval the node state and the d
        collocation states, then the final state — at the times t_k + tau_j dt (tau_0 = 0), then ``final_time``.
        Raises ``RuntimeError`` if an interval's collocation equations did not converge."""
        if getattr(self, "_h1", None) is None:  # the handle (tables, buffers) is built once per IvpFes
            self._h1 = self.handle(batch=1)
            self._u1 = self.controls.T.reshape(1, -1).copy() if self.controls.shape[0] else None
        traj = self._h1.integrate(u=self._u1)
        m = self.ode_solver.n_integration_steps
        nx = self.model.nb_state
        traj = traj.reshape(self._h1.n_samples, nx)
        result = {name: traj[:, i][np.newaxis, :] for i, name in enumerate(self.model.name_dof)}
        if self._h1.collocation:
            status = int(self._h1.integrate_status()[0])
            if status < 0:
                raise RuntimeError(f"collocation integration did not converge in interval {-status - 1}")
            if not return_time:
                return result
            dt = self.final_time / self.n_shooting
            tau = self._h1.collocation_points()
            time = np.array([k * dt + t * dt for k in range(self.n_shooting) for t in tau] + [float(self.final_time)])
            return result, time
        if not return_time:
            return result
        hstep = self.final_time / self.n_shooting / m
        time = np.array([k * (self.final_time / self.n_shooting) + j * hstep for k in range(self.n_shooting)
                         for j in range(m)] + [float(self.final_time)])
        return result, time

    def close(self):
        if getattr(self, "_h1", None) is not None:
            self._h1.close()
            self._h1 = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @classmethod
    def from_frequency_and_final_time(cls, fes_parameters: dict = None, ivp_parameters: dict = None):
        """ivp_fes.py:359-405."""
        frequency = fes_parameters["frequency"]
        if not isinstance(frequency, int):
            raise ValueError("Frequency must be an int")
        round_down = fes_parameters["round_down"]
        if not isinstance(round_down, bool):
            raise ValueError("Round down must be a bool")
        final_time = ivp_parameters["final_time"]
        if not isinstance(final_time, int | float):
            raise ValueError("Final time must be an int or float")
        fes_parameters["n_stim"] = final_time * frequency
        if round_down or float(fes_parameters["n_stim"]).is_integer():
            fes_parameters["n_stim"] = int(fes_parameters["n_stim"])
        else:
            raise ValueError("The number of stimulation needs to be integer within the final time t, set round down "
                             "to True or set final_time * frequency to make the result an integer.")
        fes_parameters["stim_time"] = list(np.round([i * 1 / frequency for i in range(fes_parameters["n_stim"])], 3))
        return cls(fes_parameters, ivp_parameters)

    @classmethod
    def from_frequency_and_n_stim(cls, fes_parameters: dict = None, ivp_parameters: dict = None):
        """ivp_fes.py:407-443."""
        n_stim = fes_parameters["n_stim"]
        if not isinstance(n_stim, int):
            raise ValueError("n_stim must be an int")
        frequency = fes_parameters["frequency"]
        if not isinstance(frequency, int):
            raise ValueError("Frequency must be an int")
        ivp_parameters["final_time"] = n_stim / frequency
        fes_parameters["stim_time"] = list(np.round([i * 1 / frequency for i in range(n_stim)], 3))
        return cls(fes_parameters, ivp_parameters)


def check_pulse_values(model, pulse_width, pulse_intensity):
    """The pulse-width (Ding2007) / pulse-intensity (Hmed2018) checks of ``IvpFes.dictionaries_check``."""
    if isinstance(model, DingModelPulseWidthFrequency | DingModelPulseWidthFrequencyWithFatigue):
        pw = pulse_width
        if isinstance(pw, bool) or not isinstance(pw, int | float | list):
            raise TypeError("pulse_width must be int, float or list type")
        ok = all(p >= model.pd0 for p in pw) if isinstance(pw, list) else pw >= model.pd0
        if not ok:
            raise ValueError("pulse width must be greater than minimum pulse width")
    if isinstance(model, DingModelPulseIntensityFrequency | DingModelPulseIntensityFrequencyWithFatigue):
        pi = pulse_intensity
        if isinstance(pi, bool) or not isinstance(pi, int | float | list):
            raise TypeError("pulse_intensity must be int, float or list type")
        imin = model.min_pulse_intensity()
        ok = all(p >= imin for p in pi) if isinstance(pi, list) else bool(pi >= imin)
        if not ok:
            raise ValueError("Pulse intensity must be greater than minimum pulse intensity")


def expand_pulse_mode(stim_time: list, pulse_mode: str) -> list:
    """The train after its pulse mode: doublets / triplets add pulses 5 and 10 ms after each one (ivp_fes.py:232-256);
    a new sorted list ("single": the list itself)."""
    if pulse_mode == "single":
        return stim_time
    if pulse_mode == "doublet":
        extra = [[round(t + 0.005, 3) for t in stim_time]]
    elif pulse_mode == "triplet":
        extra = [[round(t + 0.005, 3) for t in stim_time], [round(t + 0.01, 3) for t in stim_time]]
    else:
        raise ValueError("Pulse mode not yet implemented")
    return sorted(stim_time + [t for e in extra for t in e])


def activation_nodes(stim_time, n_shooting: int, final_time) -> list:
    """Per pulse, the first node k with t_i <= k final_time / n_shooting, in the exact rational arithmetic of
    ``get_numerical_data_time_series`` (a pulse before t = 0 is visible from node 0; a value above ``n_shooting``
    means the pulse is never visible)."""
    tf = Fraction(final_time).limit_denominator()
    out = []
    for t in stim_time:
        q = Fraction(t).limit_denominator() * n_shooting / tf
        out.append(max(0, -((-q.numerator) // q.denominator)))  # ceil
    return out


def pack_train_fields(model, stim_time, n_shooting, final_time, truncation, pulse_width=None,
                      pulse_intensity=None) -> dict:
    """What the sweep kernel needs of one train (``stim_time`` after its pulse mode): pulse times, activation nodes,
    per-pulse widths (Ding2007) or intensities (Hmed2018), truncation, n_shooting, final_time.  Pulses that no node
    sees are left out.

    Ding2007: ``IvpFes._build_controls`` gives interval k the width ``pulse_width[min(v, N + 1) - 1]`` where v is the
    number of visible pulses (the reference's ``stim_idx_at_node_list`` is cut from a list of N + 1 nodes), so pulse i
    carries ``pulse_width[min(i, N)]``: the interval widths are the ones ``IvpFes.integrate`` uses."""
    times = [float(t) for t in stim_time]
    if any(b < a for a, b in zip(times, times[1:])):
        raise ValueError("stim_time must be sorted")
    N = int(n_shooting)
    act = activation_nodes(stim_time, N, final_time)
    n = sum(1 for a in act if a <= N)
    value = None
    if isinstance(model, DingModelPulseWidthFrequency):
        pw = pulse_width
        if isinstance(pw, list) and len(pw) != 1:
            value = [float(pw[min(i, N, len(pw) - 1)]) for i in range(n)]
        else:
            value = [float(pw[0] if isinstance(pw, list) else pw)] * n
    elif isinstance(model, DingModelPulseIntensityFrequency):
        pi = pulse_intensity
        if isinstance(pi, list) and len(pi) != 1:
            value = [float(pi[i]) for i in range(n)]
        else:
            value = [float(pi[0] if isinstance(pi, list) else pi)] * n
    return {"times": times[:n], "act_node": act[:n], "value": value, "truncation": int(truncation),
            "n_shooting": N, "final_time": float(final_time)}


def pack_train(ivp: IvpFes) -> dict:
    """``pack_train_fields`` of one ``IvpFes``."""
    return pack_train_fields(ivp.model, ivp.stim_time, ivp.n_shooting, ivp.final_time,
                             ivp.model._sum_stim_truncation, ivp.pulse_width, ivp.pulse_intensity)


_TRAIN_KEYS = {"stim_time", "final_time", "n_shooting", "pulse_mode", "sum_stim_truncation", "pulse_width",
               "pulse_intensity"}


def pack_train_dict(model, train: dict) -> dict:
    """``pack_train_fields`` of one train dict (keys: ``stim_time``, ``final_time``, and optionally ``n_shooting``
    (None: the ``OcpFes.prepare_n_shooting`` rule), ``pulse_mode``, ``sum_stim_truncation`` (None: the model's),
    ``pulse_width`` / ``pulse_intensity``), with ``IvpFes``'s defaults, checks and messages, and no ``IvpFes``."""
    if not isinstance(train, dict):
        raise TypeError("a train must be a dictionary")
    unknown = set(train) - _TRAIN_KEYS
    if unknown:
        raise ValueError(f"unknown keys {sorted(unknown)}")
    stim_time = train.get("stim_time")
    if not isinstance(stim_time, list):
        raise TypeError("stim_time must be a list")
    final_time = train.get("final_time")
    if isinstance(final_time, bool) or not isinstance(final_time, int | float):
        raise ValueError("final_time must be an int or float type")
    if not final_time > 0:
        raise ValueError("final_time must be positive")
    ns = train.get("n_shooting")
    if ns is not None and (isinstance(ns, bool) or not isinstance(ns, int) or ns < 1):
        raise ValueError("n_shooting must be a positive int (or None for the stimulation-time LCM rule)")
    pulse_mode = train.get("pulse_mode", "single")
    if not isinstance(pulse_mode, str):
        raise ValueError("pulse_mode must be a string type")
    T = train.get("sum_stim_truncation")
    T = model._sum_stim_truncation if T is None else T
    if isinstance(T, bool) or not isinstance(T, int) or T < 1:
        raise ValueError("sum_stim_truncation must be a positive int")
    pulse_width = train.get("pulse_width", 0.0003)  # IvpFes's defaults
    pulse_intensity = train.get("pulse_intensity", 50)
    check_pulse_values(model, pulse_width, pulse_intensity)
    stim_time = expand_pulse_mode(stim_time, pulse_mode)
    if ns is None:
        ns = OcpFes.prepare_n_shooting(stim_time, final_time)
    return pack_train_fields(model, stim_time, ns, final_time, T, pulse_width, pulse_intensity)


def sweep_order(work) -> np.ndarray:
    """Launch order of a sweep: instances sorted by their amount of work, heaviest first (stable), so that the
    lanes of a wave finish together.  ``order[j]`` is the caller's index of packed instance j."""
    return np.argsort(-np.asarray(work, dtype=np.int64), kind="stable")


class IvpSweep:
    """A batch of ``IvpFes`` problems of one model integrated in one launch, every instance with its own train.

    ``ivps``: ``IvpFes`` objects of the same model class, model constants and ``ode_solver`` (RK1 / RK2 / RK4);
    stimulation times, pulse mode, truncation, ``n_shooting``, ``final_time`` and pulse widths / intensities are
    free per instance.  ``ValueError`` names the first instance that does not fit."""

    def __init__(self, ivps, device: int = 0):
        ivps = list(ivps)
        if not ivps:
            raise ValueError("IvpSweep needs at least one IvpFes")
        first = ivps[0]
        if not isinstance(first, IvpFes):
            raise TypeError("IvpSweep takes a list of IvpFes")
        solver = first.ode_solver
        for i, ivp in enumerate(ivps):
            if not isinstance(ivp, IvpFes):
                raise TypeError("IvpSweep takes a list of IvpFes")
            if isinstance(ivp.ode_solver, OdeSolver.COLLOCATION):
                raise ValueError(f"ivps[{i}]: OdeSolver.COLLOCATION is not supported by IvpSweep")
            if type(ivp.model) is not type(first.model):
                raise ValueError(f"ivps[{i}]: model class {type(ivp.model).__name__} differs from "
                                 f"{type(first.model).__name__}")
            if ivp.model.cfx_constants() != first.model.cfx_constants():
                raise ValueError(f"ivps[{i}]: model constants differ from ivps[0]'s")
            if (type(ivp.ode_solver) is not type(solver)
                    or ivp.ode_solver.n_integration_steps != solver.n_integration_steps):
                raise ValueError(f"ivps[{i}]: ode_solver differs from ivps[0]'s")
            if any(t != PLACEHOLDER_TIME for t in ivp.model.previous_stim["time"]):
                raise ValueError(f"ivps[{i}]: previous_stim is not supported by IvpSweep")
        trains = []
        for i, ivp in enumerate(ivps):
            try:
                trains.append(pack_train(ivp))
            except ValueError as e:
                raise ValueError(f"ivps[{i}]: {e}") from None
        self._setup(first.model, solver, trains, device)

    @classmethod
    def from_trains(cls, model, trains, ode_solver=None, device: int = 0):
        """The sweep of a list of train dicts on one model, packed directly: no ``IvpFes`` is constructed.

        A train: ``{"stim_time": [...], "final_time": tf}`` and optionally ``"n_shooting"`` (None: the
        ``OcpFes.prepare_n_shooting`` rule on the train after its pulse mode), ``"pulse_mode"`` ("single"),
        ``"sum_stim_truncation"`` (None: the model's), ``"pulse_width"`` (Ding2007) / ``"pulse_intensity"`` (Hmed2018):
        a value or one per pulse.  The packed arrays are those of ``IvpSweep([IvpFes(...), ...])`` for the same
        trains; ``model.stim_time`` is not used and the model is not modified.  ``ode_solver``: RK1 / RK2 / RK4,
        default ``OdeSolver.RK4(n_integration_steps=10)``.  Errors name the offending ``trains[i]``."""
        if not isinstance(model, FesModel):
            raise TypeError("model must be a FesModel type")
        solver = OdeSolver.RK4(n_integration_steps=10) if ode_solver is None else ode_solver
        if not isinstance(solver, (OdeSolver.RK1, OdeSolver.RK2, OdeSolver.RK4)):
            raise ValueError("ode_solver must be an OdeSolver.RK1, RK2 or RK4 (OdeSolver.COLLOCATION is not supported "
                             "by IvpSweep)")
        if any(t != PLACEHOLDER_TIME for t in model.previous_stim["time"]):
            raise ValueError("previous_stim is not supported by IvpSweep")
        trains = list(trains)
        if not trains:
            raise ValueError("IvpSweep needs at least one train")
        packed = []
        for i, train in enumerate(trains):
            try:
                packed.append(pack_train_dict(model, train))
            except (TypeError, ValueError, IndexError) as e:
                raise type(e)(f"trains[{i}]: {e}") from None
        self = cls.__new__(cls)
        self._setup(model, solver, packed, device)
        return self

    def _setup(self, model, solver, trains, device):
        """Sort, pack and check the ``pack_train_fields`` dicts of the batch (in the caller's order)."""
        self.model = model
        self.ode_solver = solver
        self.batch = len(trains)
        self.device = device
        self.n_shooting = np.array([t["n_shooting"] for t in trains], dtype=np.int32)
        self.final_time = np.array([t["final_time"] for t in trains], dtype=np.float64)
        m = solver.n_integration_steps
        work = [t["n_shooting"] * m * max(1, min(t["truncation"], len(t["times"]))) for t in trains]
        self.order = sweep_order(work)
        self.max_pulses = max(1, max(len(t["times"]) for t in trains))
        self.max_shooting = int(self.n_shooting.max())
        self.trains = self._pack([trains[i] for i in self.order])
        _cfx.sweep_check(self.model.cfx_model_id, solver.scheme, m, self.batch, self.max_pulses, self.max_shooting,
                         self.trains)
        self._sweep = None

    def _pack(self, trains) -> dict:
        """SoA arrays of ``cfx_sweep_trains`` in launch order."""
        B, P = len(trains), self.max_pulses
        with_value = trains[0]["value"] is not None
        out = {"times": np.zeros((P, B)), "act_node": np.zeros((P, B), dtype=np.int32),
               "value": np.zeros((P, B)) if with_value else None,
               "n_pulses": np.array([len(t["times"]) for t in trains], dtype=np.int32),
               "truncation": np.array([t["truncation"] for t in trains], dtype=np.int32),
               "n_shooting": np.array([t["n_shooting"] for t in trains], dtype=np.int32),
               "final_time": np.array([t["final_time"] for t in trains], dtype=np.float64)}
        for b, t in enumerate(trains):
            n = len(t["times"])
            out["times"][:n, b] = t["times"]
            out["act_node"][:n, b] = t["act_node"]
            if with_value:
                out["value"][:n, b] = t["value"]
        return out

    def sweep(self) -> _cfx.Sweep:
        """The library object (created on first use)."""
        if self._sweep is None:
            self._sweep = _cfx.Sweep(model_id=self.model.cfx_model_id, constants=self.model.cfx_constants(),
                                     scheme=self.ode_solver.scheme, n_steps=self.ode_solver.n_integration_steps,
                                     batch=self.batch, max_pulses=self.max_pulses, max_shooting=self.max_shooting,
                                     device=self.device)
        return self._sweep

    def integrate(self, x0=None, nodes: bool = False) -> dict:
        """Single shooting of every instance from the rest state, or from ``x0`` ((nx,) for all, or (B, nx)).

        Returns {state: (B,)}, the final states, in the order of ``ivps``.  ``nodes=True``: {state: (B, N_max + 1)},
        the node states, NaN past an instance's own ``n_shooting``, plus ``"n_shooting"``: (B,)."""
        B = self.batch
        if x0 is not None:
            x0 = self._start_states(x0)
        final, traj = self.sweep().integrate(self.trains, x0=x0, nodes=nodes)
        inverse = np.empty(B, dtype=np.int64)
        inverse[self.order] = np.arange(B)
        names = self.model.name_dof
        if not nodes:
            return {name: final[i, inverse].copy() for i, name in enumerate(names)}
        result = {name: traj[:, i, :].T[inverse].copy() for i, name in enumerate(names)}
        result["n_shooting"] = self.n_shooting.copy()
        return result

    def _start_states(self, x0):
        """``x0`` ((nx,) for all, or (B, nx), caller's order) as the (nx, B) array of the launch order."""
        nx, B = self.model.nb_state, self.batch
        x0 = np.asarray(x0, dtype=np.float64)
        if x0.shape == (nx,):
            x0 = np.broadcast_to(x0, (B, nx))
        if x0.shape != (B, nx):
            raise ValueError(f"x0 must have shape ({nx},) or ({B}, {nx})")
        return np.ascontiguousarray(x0[self.order].T)

    def score(self, target, sample_dt=None, x0=None) -> dict:
        """Integrate every instance as ``integrate`` does and score its node forces F_0..F_N against a target force,
        on the device (``cfx_sweep_score``): no node trajectory is written.

        ``target``: a scalar (a constant target) or a 1-D array of samples at t = j ``sample_dt``, piecewise linear
        between them and held at the last one beyond the table.  Returns {state: (B,)}, the final states, plus
        ``track`` (dt sum_k (F_k - y(t_k))^2), ``impulse`` (the trapezoid of F over the nodes), ``peak`` and
        ``peak_node`` (int: the first node that attains it), ``end_error`` (F_N - y(final_time)) and ``mean_force``
        (impulse / final_time): each (B,), in the caller's order."""
        y = np.atleast_1d(np.asarray(target, dtype=np.float64))
        if y.ndim != 1 or y.size < 1:
            raise ValueError("target must be a scalar or a non-empty 1-D array")
        if y.size > 1 and sample_dt is None:
            raise ValueError("sample_dt must be given with a sampled target")
        x0 = None if x0 is None else self._start_states(x0)
        final, metrics = self.sweep().score(self.trains, y, 1.0 if sample_dt is None else float(sample_dt), x0=x0)
        inverse = np.empty(self.batch, dtype=np.int64)
        inverse[self.order] = np.arange(self.batch)
        result = {name: final[i, inverse].copy() for i, name in enumerate(self.model.name_dof)}
        for i, name in enumerate(_cfx.SWEEP_METRICS):
            result[name] = metrics[i, inverse].copy()
        result["peak_node"] = result["peak_node"].astype(np.int64)
        return result

    def close(self):
        if getattr(self, "_sweep", None) is not None:
            self._sweep.close()
            self._sweep = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
