"""FesIdentification: fit a muscle model's force parameters to a measured force curve (reference:
cocofest/identification/*_force_parameter_identification.py and cocofest/optimization/fes_identification_ocp.py).

The reference transcribes the fit as an OCP with the model constants as NLP parameters and gives it to Ipopt.  Here
the same least-squares problem, ``min_theta dt sum_k w_k (F_k(theta) - y_k)^2`` over a single-shooting trajectory
from the rest state, is solved by a batched, box-projected Levenberg-Marquardt over many starts at once: every
iteration is ONE ``cfx_id_normal`` launch (cost, gradient and Gauss-Newton matrix of every start, one GPU thread
each), followed by batched torch operations on the device for the tiny n_id x n_id damped solves, the gain ratio
and the damping update.  Models: Ding2003, Ding2007 and Hmed2018 without fatigue.

``FesMultiTrainIdentification`` fits ONE parameter set to several recordings at once (the reference's ``data_path``
lists: trains at different frequencies, pulse widths or intensities), ``min_theta sum_e dt_e sum_k w_ek (F_ek - y_ek)^2``:
every iteration is one ``cfx_idm_normal`` launch over all starts and all trains.

``FesFatigueIdentification`` is step 2 of the published protocol: with the force parameters fixed (the model's own
values), the four fatigue parameters alpha_a, alpha_tau1, alpha_km, tau_fat of a ``*WithFatigue`` model are fitted to
a fatiguing train the same way, one ``cfx_idf_normal`` launch per iteration.
``FesMultiTrainFatigueIdentification`` fits them jointly to several recordings (bursts, rest gaps of different
lengths, test bursts: what determines tau_fat sharply), one ``cfx_idfm_normal`` launch per iteration.
"""

from __future__ import annotations

import copy

import numpy as np

from . import _cfx
from .fes_models import DingModelPulseIntensityFrequency, DingModelPulseWidthFrequency, FesModel
from .ivp import PLACEHOLDER_TIME, IvpFes, pack_train, sweep_order
from .ode_solver import OdeSolver

# Default initial guesses and bounds of the identified parameters: the reference's ``_set_default_values`` tables
# (ding2003_force_parameter_identification.py:107-150, ding2007_...:105-148, hmed2018_...:103-160), as data.
DEFAULT_VALUES = {
    "ding2003": {
        "a_rest": (1000, 1, 10000), "km_rest": (0.5, 0.001, 1), "tau1_rest": (0.5, 0.0001, 1),
        "tau2": (0.5, 0.0001, 1),
    },
    "ding2007": {
        "tau1_rest": (0.5, 0.0001, 1), "tau2": (0.5, 0.0001, 1), "km_rest": (0.5, 0.001, 1),
        "a_scale": (5000, 1, 10000), "pd0": (1e-4, 1e-4, 6e-4), "pdt": (1e-4, 1e-4, 6e-4),
    },
    "hmed2018": {
        "a_rest": (1000, 1, 10000), "km_rest": (0.5, 0.001, 1), "tau1_rest": (0.5, 0.0001, 1),
        "tau2": (0.5, 0.0001, 1), "ar": (0.5, 0.01, 1), "bs": (0.05, 0.001, 0.1), "Is": (50, 1, 150),
        "cr": (1, 0.01, 2),
    },
}

# per-start status of FesIdentification.solve
# (STALLED: the damping grew, after rejected trials, until the step fell under xtol: no descent was found)
NOT_CONVERGED, CONVERGED_GRADIENT, CONVERGED_STEP, STALLED = 0, 1, 2, 3


def _family(model):
    if isinstance(model, DingModelPulseWidthFrequency):
        return "ding2007"
    if isinstance(model, DingModelPulseIntensityFrequency):
        return "hmed2018"
    return "ding2003"


def lm_solve(normal, theta0, lo, hi, max_iter=100, gtol=1e-8, xtol=1e-10, mu0=1e-3):
    """Batched, box-projected Levenberg-Marquardt in the scaled variables x = theta / |theta0|.

    ``normal(theta)`` -> (cost (B,), grad (n, B), gn (n (n + 1) / 2, B)) at theta (n, B) (one cfx_id_normal launch);
    theta0, lo, hi: (n, B) torch tensors.  Per instance and iteration:
      * active set: x at a bound with the gradient pointing outwards; those entries are fixed for the step;
      * step: (H + mu diag(H)) dx = -g on the free entries, x_trial = clip(x + dx, lo, hi);
      * gain ratio rho = (c - c_trial) / -(g.dx + dx.H.dx / 2) with the step actually taken; the trial is accepted
        when rho > 1e-4 (so the cost never increases), then mu *= max(1/3, 1 - (2 rho - 1)^3), nu = 2; otherwise
        mu *= nu, nu *= 2 (Nielsen's update);
      * stop: projected-gradient norm <= gtol max(1, c0) (status 1), or step norm <= xtol, both max-norms in the
        scaled variables: status 2 when that small step was accepted, status 3 (stalled) when it was rejected, i.e.
        the step is small only because rejected trials inflated the damping.
    Returns (theta, cost, iterations, status, cost_history (iterations + 1, B))."""
    import torch

    n, B = theta0.shape
    scale = theta0.abs().clamp_min(1e-300)
    x, xl, xu = theta0 / scale, lo / scale, hi / scale
    tri = torch.tril_indices(n, n)
    pk = tri[0] * (tri[0] + 1) // 2 + tri[1]

    def evaluate(xx):
        c, g, h = normal(xx * scale)
        H = torch.zeros((B, n, n), dtype=xx.dtype, device=xx.device)
        H[:, tri[0], tri[1]] = h[pk].T
        H[:, tri[1], tri[0]] = h[pk].T
        return c.clone(), (g * scale).T.clone(), H * (scale.T[:, :, None] * scale.T[:, None, :])

    xT = x.T.clone()  # (B, n)
    lT, uT = xl.T, xu.T
    c, g, H = evaluate(xT.T)
    c0 = c.clone()
    mu = torch.full((B,), mu0, dtype=x.dtype, device=x.device)
    nu = torch.full_like(mu, 2.0)
    status = torch.zeros(B, dtype=torch.int32, device=x.device)
    iters = torch.zeros(B, dtype=torch.int32, device=x.device)
    history = [c.clone()]
    for _ in range(max_iter):
        active = ((xT <= lT) & (g > 0)) | ((xT >= uT) & (g < 0))
        pg = torch.where(active, torch.zeros_like(g), g)
        done_g = (status == 0) & (pg.abs().amax(dim=1) <= gtol * c0.clamp_min(1.0))
        status = torch.where(done_g, torch.full_like(status, CONVERGED_GRADIENT), status)
        live = status == 0
        if not bool(live.any()):
            break
        free = (~active).to(x.dtype)
        Hf = H * free[:, :, None] * free[:, None, :]
        diag = torch.diagonal(Hf, dim1=1, dim2=2)
        floor = 1e-12 * diag.amax(dim=1, keepdim=True) + 1e-300  # a parameter the curve does not depend on
        damp = mu[:, None] * (diag + floor) + (1.0 - free)  # fixed entries: unit diagonal, zero step
        dx = torch.linalg.solve_ex(Hf + torch.diag_embed(damp), -pg[:, :, None])[0][:, :, 0]
        dx = torch.where(torch.isfinite(dx), dx, torch.zeros_like(dx))
        xt = torch.minimum(torch.maximum(xT + dx, lT), uT)
        dx = xt - xT
        ct, gt, Ht = evaluate(xt.T)
        pred = -((g * dx).sum(dim=1) + 0.5 * (dx * (H @ dx[:, :, None])[:, :, 0]).sum(dim=1))
        rho = (c - ct) / pred.clamp_min(1e-300)
        ok = live & torch.isfinite(ct) & (rho > 1e-4) & (ct <= c)
        small = live & (dx.abs().amax(dim=1) <= xtol)
        okv, okm = ok[:, None], ok[:, None, None]
        xT = torch.where(okv, xt, xT)
        g = torch.where(okv, gt, g)
        H = torch.where(okm, Ht, H)
        c = torch.where(ok, ct, c)
        shrink = (1.0 - (2.0 * rho - 1.0) ** 3).clamp(min=1.0 / 3.0)
        mu = torch.where(ok, mu * shrink, torch.where(live, mu * nu, mu)).clamp(1e-15, 1e15)
        nu = torch.where(ok, torch.full_like(nu, 2.0), torch.where(live, nu * 2.0, nu))
        iters = iters + live.to(iters.dtype)
        status = torch.where(small & ok, torch.full_like(status, CONVERGED_STEP), status)
        status = torch.where(small & ~ok, torch.full_like(status, STALLED), status)
        history.append(c.clone())
    return (xT * scale.T).T, c, iters, status, torch.stack(history)


class _MultistartIdentification:
    """What the two identification problems share: input checks, seeded starts, evaluation, the multistart fit.  A
    subclass names its parameter ids and libcfx calls and builds ``defaults`` {key: (guess, min, max)}."""

    _PARAM_IDS = _cfx.PARAM_IDS
    _CHECK, _FORCES, _NORMAL = "cfx_id_check", "id_forces", "id_normal"

    def _setup(self, model, defaults, stim_time, final_time, force_tracking, key_parameter_to_identify, pulse_width,
               pulse_intensity, ode_solver, bounds, initial_guess, n_starts, seed, start_spread, weight, device):
        if not isinstance(key_parameter_to_identify, list):
            raise TypeError(f"The given key_parameter_to_identify must be list type,"
                            f" the given value is {type(key_parameter_to_identify)} type")
        for key in key_parameter_to_identify:
            if key not in defaults:
                raise ValueError(f"The given key_parameter_to_identify is not valid,"
                                 f" the given value is {key},"
                                 f" the available values are {list(defaults.keys())}")
        if len(set(key_parameter_to_identify)) != len(key_parameter_to_identify) or not key_parameter_to_identify:
            raise ValueError("key_parameter_to_identify must list every parameter once, and at least one")
        # fes_identification_ocp.py:145-179
        if isinstance(final_time, bool) or not isinstance(final_time, int | float):
            raise TypeError("final_time must be int or float type.")
        if not isinstance(force_tracking, list):
            raise TypeError(f"force_tracking must be list type,"
                            f" currently force_tracking is {type(force_tracking)}) type.")
        if not all(isinstance(val, int | float) for val in force_tracking):
            raise TypeError("force_tracking must be list of int or float type.")
        fes = {"model": model}
        if self.family == "ding2007":
            if not isinstance(pulse_width, dict):
                raise TypeError(f"pulse_width must be dict type, currently pulse_width is {type(pulse_width)}) type.")
            if "fixed" not in pulse_width:
                raise ValueError("pulse_width must hold the key 'fixed' (a value, or one value per pulse)")
            fes["pulse_width"] = pulse_width["fixed"]
        if self.family == "hmed2018":
            if not isinstance(pulse_intensity, dict):
                raise TypeError(f"pulse_intensity must be dict type,"
                                f" currently pulse_intensity is {type(pulse_intensity)}) type.")
            if "fixed" not in pulse_intensity:
                raise ValueError("pulse_intensity must hold the key 'fixed' (a value, or one value per pulse)")
            if isinstance(pulse_intensity["fixed"], bool) or not isinstance(pulse_intensity["fixed"],
                                                                              int | float | list):
                raise ValueError("fixed pulse_intensity must be a int, float or list type.")
            fes["pulse_intensity"] = pulse_intensity["fixed"]
        if not isinstance(ode_solver, (OdeSolver.RK1, OdeSolver.RK2, OdeSolver.RK4)):
            raise TypeError("ode_solver must be a OdeSolver.RK1, RK2 or RK4 type")
        if isinstance(n_starts, bool) or not isinstance(n_starts, int) or n_starts < 1:
            raise ValueError("n_starts must be a positive int")
        if stim_time is not None:
            model.stim_time = list(stim_time)
        if not model.stim_time:
            raise ValueError("stim_time must be given, here or in the model")
        self.model = model
        self.keys = list(key_parameter_to_identify)
        self.param_ids = [self._PARAM_IDS[k] for k in self.keys]
        self._ivp = IvpFes(fes, {"final_time": final_time, "ode_solver": ode_solver})
        self.n_shooting, self.final_time = self._ivp.n_shooting, final_time
        if len(force_tracking) != self.n_shooting + 1:
            raise ValueError(f"force_tracking has {len(force_tracking)} values, expected one per node: n_shooting + 1 "
                             f"= {self.n_shooting + 1}")
        self.target = np.asarray(force_tracking, dtype=np.float64)
        self.weight = np.ones(self.n_shooting + 1) if weight is None else np.asarray(weight, dtype=np.float64)
        if self.weight.shape != self.target.shape:
            raise ValueError("weight must hold one value per node")
        self.controls = self._ivp.controls.T.reshape(-1).copy()  # [N * nu], interval-major
        self.n_starts, self.seed, self.start_spread, self.device = n_starts, seed, float(start_spread), device
        bounds, initial_guess = bounds or {}, initial_guess or {}
        for key in list(bounds) + list(initial_guess):
            if key not in self.keys:
                raise ValueError(f"bounds / initial_guess given for {key}, which is not identified")
        self.lower = np.array([bounds.get(k, defaults[k][1:])[0] for k in self.keys], dtype=np.float64)
        self.upper = np.array([bounds.get(k, defaults[k][1:])[1] for k in self.keys], dtype=np.float64)
        guess = np.array([initial_guess.get(k, defaults[k][0]) for k in self.keys], dtype=np.float64)
        self.initial_guess = np.clip(guess, self.lower, self.upper)
        # parameter-list checks of libcfx, before any handle (and device) exists
        lib = _cfx.load_library()
        ids = np.asarray(self.param_ids, dtype=np.int32)
        import ctypes as C

        check = getattr(lib, self._CHECK)
        rc = check(model.cfx_model_id, ids.size, ids.ctypes.data_as(C.POINTER(C.c_int32)))
        if rc != _cfx.OK:
            raise _cfx.CfxError(rc, lib.cfx_last_error(None).decode())
        self._handles = {}

    # ---- starts ---------------------------------------------------------------------------------------
    def starts(self) -> np.ndarray:
        """(n_id, n_starts): start 0 the initial guess, the others log-uniform around it (seeded), in bounds."""
        rng = np.random.default_rng(self.seed)
        z = rng.uniform(-1.0, 1.0, size=(len(self.keys), self.n_starts))
        z[:, 0] = 0.0
        th = self.initial_guess[:, None] * np.exp(self.start_spread * z)
        return np.clip(th, self.lower[:, None], self.upper[:, None])

    def _handle(self, batch):
        if batch not in self._handles:
            self._handles[batch] = self._ivp.handle(batch=batch, layout="soa", device=self.device)
        return self._handles[batch]

    # ---- evaluation -----------------------------------------------------------------------------------
    def forces(self, theta, with_sensitivities=False):
        """Node forces (N+1, B) for parameters theta (n_id, B) (cfx_id_forces); with ``with_sensitivities`` also
        dF_k / dtheta_j (N+1, n_id, B).  numpy in, numpy out; CUDA tensors in, CUDA tensors out."""
        if _cfx._is_tensor(theta):
            B, u = theta.shape[1], None
            if self.controls.size:
                import torch

                u = torch.as_tensor(self.controls, device=theta.device)
        else:
            theta = np.ascontiguousarray(theta, dtype=np.float64).reshape(len(self.keys), -1)
            B, u = theta.shape[1], (self.controls if self.controls.size else None)
        call = getattr(self._handle(B), self._FORCES)
        force, sens = call(self.param_ids, theta, u=u, n_data=1, with_sens=with_sensitivities)
        return (force, sens) if with_sensitivities else force

    def solve(self, max_iter=100, gtol=1e-8, xtol=1e-10):
        """Levenberg-Marquardt from every start (``lm_solve``).  Returns the best start's parameters as a dict over
        ``model.identifiable_parameters`` (identified values replace the model's), plus "cost", "best_start" and
        "starts": {"theta" (n_starts, n_id), "cost", "iterations", "status", "cost_history"} as numpy arrays."""
        import torch

        dev = torch.device("cuda", self.device)
        call = getattr(self._handle(self.n_starts), self._NORMAL)
        n, B = len(self.keys), self.n_starts
        on = lambda a: torch.as_tensor(np.ascontiguousarray(a, dtype=np.float64), device=dev)  # noqa: E731
        y, w = on(self.target), on(self.weight)
        u = on(self.controls) if self.controls.size else None
        cost = torch.empty(B, dtype=torch.float64, device=dev)
        grad = torch.empty((n, B), dtype=torch.float64, device=dev)
        gn = torch.empty((n * (n + 1) // 2, B), dtype=torch.float64, device=dev)

        def normal(theta):
            return call(self.param_ids, theta.contiguous(), y, w, u=u, n_data=1, cost=cost, grad=grad, gn=gn)

        with torch.cuda.device(dev):
            theta, c, iters, status, hist = lm_solve(
                normal, on(self.starts()), on(np.repeat(self.lower[:, None], B, 1)),
                on(np.repeat(self.upper[:, None], B, 1)), max_iter=max_iter, gtol=gtol, xtol=xtol)
            theta, c, iters, status, hist = (t.cpu().numpy() for t in (theta, c, iters, status, hist))
        ok = np.where(np.isfinite(c), c, np.inf)
        best = int(np.argmin(ok))
        result = dict(self.model.identifiable_parameters)
        for j, key in enumerate(self.keys):
            result[key] = float(theta[j, best])
        result["cost"] = float(c[best])
        result["best_start"] = best
        result["starts"] = {"theta": theta.T.copy(), "cost": c, "iterations": iters, "status": status,
                            "cost_history": hist}
        return result

    def close(self):
        for h in self._handles.values():
            h.close()
        self._handles = {}
        self._ivp.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class FesIdentification(_MultistartIdentification):
    """Force-parameter identification of one muscle from one measured force curve, over ``n_starts`` starts.

    ``force_tracking``: the measured force at every node (n_shooting + 1 values, n_shooting from
    ``OcpFes.prepare_n_shooting``); ``key_parameter_to_identify``: keys of ``model.identifiable_parameters``;
    ``pulse_width`` / ``pulse_intensity``: ``{"fixed": value or one value per pulse}`` as the reference's OcpFesId;
    ``bounds``: ``{key: (min, max)}`` and ``initial_guess``: ``{key: value}`` override the reference's defaults
    (``DEFAULT_VALUES``); start 0 is the initial guess, every other start draws each parameter log-uniformly within
    a factor ``exp(start_spread)`` of it (seeded), clipped to the bounds; ``weight``: per-node weights (default 1).
    """

    def __init__(self, model=None, stim_time=None, final_time=None, force_tracking=None,
                 key_parameter_to_identify=None, pulse_width=None, pulse_intensity=None,
                 ode_solver=OdeSolver.RK4(n_integration_steps=10), bounds=None, initial_guess=None, n_starts=64,
                 seed=0, start_spread=0.5, weight=None, device=0):
        if not isinstance(model, FesModel):
            raise TypeError("model must be a FesModel type")
        if model._with_fatigue:
            raise ValueError("The given model is not valid and should not be including the fatigue equation in the "
                             "model")
        model = copy.deepcopy(model)  # the caller's model is left as it is (stim_time, stimulation history)
        self.family = _family(model)
        defaults = DEFAULT_VALUES[self.family]
        self._setup(model, defaults, stim_time, final_time, force_tracking, key_parameter_to_identify, pulse_width,
                    pulse_intensity, ode_solver, bounds, initial_guess, n_starts, seed, start_spread, weight, device)


FATIGUE_KEYS = ("alpha_a", "alpha_tau1", "alpha_km", "tau_fat")


class FesFatigueIdentification(_MultistartIdentification):
    """Fatigue-parameter identification of one muscle from one measured force curve of a fatiguing train, over
    ``n_starts`` starts: step 2 of the protocol, after ``FesIdentification`` on the fresh muscle.

    ``model``: a ``*WithFatigue`` model holding the identified force parameters, which stay fixed;
    ``key_parameter_to_identify``: keys among alpha_a, alpha_tau1, alpha_km, tau_fat (a key left out keeps the
    model's value).  Default initial guess: the model's own value; default bounds: 0.01 x to 100 x that value, in
    increasing order (alpha_a is negative); both can be overridden.  Every other argument, ``starts``, ``forces``,
    ``solve`` and ``close`` are as ``FesIdentification``; the trajectory starts from the fatigue rest state."""

    _PARAM_IDS = _cfx.FATIGUE_PARAM_IDS
    _CHECK, _FORCES, _NORMAL = "cfx_idf_check", "idf_forces", "idf_normal"

    def __init__(self, model=None, stim_time=None, final_time=None, force_tracking=None,
                 key_parameter_to_identify=None, pulse_width=None, pulse_intensity=None,
                 ode_solver=OdeSolver.RK4(n_integration_steps=10), bounds=None, initial_guess=None, n_starts=64,
                 seed=0, start_spread=0.5, weight=None, device=0):
        if not isinstance(model, FesModel):
            raise TypeError("model must be a FesModel type")
        if not model._with_fatigue:
            raise ValueError("The given model is not valid and should be including the fatigue equation in the model")
        model = copy.deepcopy(model)  # the caller's model is left as it is (stim_time, stimulation history)
        self.family = _family(model)
        own = model.identifiable_parameters
        defaults = {k: (own[k], *sorted((0.01 * own[k], 100.0 * own[k]))) for k in FATIGUE_KEYS}
        self._setup(model, defaults, stim_time, final_time, force_tracking, key_parameter_to_identify, pulse_width,
                    pulse_intensity, ode_solver, bounds, initial_guess, n_starts, seed, start_spread, weight, device)


def force_at_node(time, force, n_shooting, final_time):
    """A recorded force curve (samples ``time``, ``force``) at the n_shooting + 1 nodes of [0, final_time], by linear
    interpolation (the reference's ``force_at_node_in_ocp``, identification_method.py:253-278)."""
    return [float(v) for v in np.interp(np.linspace(0, final_time, n_shooting + 1), time, force)]


class _MultiTrainIdentification(_MultistartIdentification):
    """What the two multi-train identification problems share: the per-train checks, packing in launch order, the
    device copy of the trains, evaluation and the joint fit with its per-train results.  A subclass checks the model,
    builds ``defaults`` {key: (guess, min, max)} and names its parameter ids, its libcfx object and its check."""

    _HANDLE, _TRAIN_CHECK = _cfx.Idm, staticmethod(_cfx.idm_check)

    def _setup_trains(self, model, defaults, trains, key_parameter_to_identify, ode_solver, bounds, initial_guess,
                      n_starts, seed, start_spread, device):
        if not isinstance(trains, list) or not trains or not all(isinstance(t, dict) for t in trains):
            raise TypeError("trains must be a non-empty list of dict")
        self.family = _family(model)
        if not isinstance(key_parameter_to_identify, list):
            raise TypeError(f"The given key_parameter_to_identify must be list type,"
                            f" the given value is {type(key_parameter_to_identify)} type")
        for key in key_parameter_to_identify:
            if key not in defaults:
                raise ValueError(f"The given key_parameter_to_identify is not valid,"
                                 f" the given value is {key},"
                                 f" the available values are {list(defaults.keys())}")
        if len(set(key_parameter_to_identify)) != len(key_parameter_to_identify) or not key_parameter_to_identify:
            raise ValueError("key_parameter_to_identify must list every parameter once, and at least one")
        if not isinstance(ode_solver, (OdeSolver.RK1, OdeSolver.RK2, OdeSolver.RK4)):
            raise TypeError("ode_solver must be a OdeSolver.RK1, RK2 or RK4 type")
        if isinstance(n_starts, bool) or not isinstance(n_starts, int) or n_starts < 1:
            raise ValueError("n_starts must be a positive int")
        self.model = copy.deepcopy(model)  # the caller's model is left as it is
        self.ode_solver = ode_solver
        self.keys = list(key_parameter_to_identify)
        self.param_ids = [self._PARAM_IDS[k] for k in self.keys]
        self.n_starts, self.seed, self.start_spread, self.device = n_starts, seed, float(start_spread), device
        self._ivps, packed, self.targets, self.weights = [], [], [], []
        for e, train in enumerate(trains):
            try:
                ivp, target, weight = self._train(train)
                packed.append(pack_train(ivp))
            except (TypeError, ValueError) as err:
                raise type(err)(f"trains[{e}]: {err}") from None
            self._ivps.append(ivp)
            self.targets.append(target)
            self.weights.append(weight)
        self.n_trains = len(trains)
        self.n_shooting = [t["n_shooting"] for t in packed]
        self.final_time = [t["final_time"] for t in packed]
        m = ode_solver.n_integration_steps
        # launch order: heaviest train first (a block is one train); results are returned in the caller's order
        self.order = sweep_order([t["n_shooting"] * m * max(1, min(t["truncation"], len(t["times"]))) for t in packed])
        self.max_pulses = max(1, max(len(t["times"]) for t in packed))
        self.max_shooting = max(self.n_shooting)
        self.trains = self._pack([packed[i] for i in self.order])
        bounds, initial_guess = bounds or {}, initial_guess or {}
        for key in list(bounds) + list(initial_guess):
            if key not in self.keys:
                raise ValueError(f"bounds / initial_guess given for {key}, which is not identified")
        self.lower = np.array([bounds.get(k, defaults[k][1:])[0] for k in self.keys], dtype=np.float64)
        self.upper = np.array([bounds.get(k, defaults[k][1:])[1] for k in self.keys], dtype=np.float64)
        guess = np.array([initial_guess.get(k, defaults[k][0]) for k in self.keys], dtype=np.float64)
        self.initial_guess = np.clip(guess, self.lower, self.upper)
        # every argument check of libcfx, before any handle (and device) exists
        self._TRAIN_CHECK(self.model.cfx_model_id, ode_solver.scheme, m, n_starts, self.n_trains, self.max_pulses,
                          self.max_shooting, self.param_ids, self.trains)
        self._handles, self._dev_trains = {}, {}

    def _train(self, train):
        """(IvpFes, target, weight) of one train, with FesIdentification's checks and messages."""
        unknown = set(train) - {"stim_time", "final_time", "force_tracking", "time", "force", "pulse_width",
                                "pulse_intensity", "weight", "pulse_mode", "sum_stim_truncation"}
        if unknown:
            raise ValueError(f"unknown keys {sorted(unknown)}")
        final_time = train.get("final_time")
        if isinstance(final_time, bool) or not isinstance(final_time, int | float):
            raise TypeError("final_time must be int or float type.")
        if not train.get("stim_time"):
            raise ValueError("stim_time must be given, here or in the model")
        model = copy.deepcopy(self.model)
        model.stim_time = list(train["stim_time"])
        if any(t != PLACEHOLDER_TIME for t in model.previous_stim["time"]):
            raise ValueError("previous_stim is not supported: every train starts from the rest state")
        model.previous_stim = {k: [] for k in model.previous_stim}
        if train.get("sum_stim_truncation") is not None:
            T = train["sum_stim_truncation"]
            if isinstance(T, bool) or not isinstance(T, int) or T < 1:
                raise ValueError("sum_stim_truncation must be a positive int")
            model._sum_stim_truncation = T
        fes = {"model": model, "pulse_mode": train.get("pulse_mode", "single")}
        if self.family == "ding2007":
            pulse_width = train.get("pulse_width")
            if not isinstance(pulse_width, dict):
                raise TypeError(f"pulse_width must be dict type, currently pulse_width is {type(pulse_width)}) type.")
            if "fixed" not in pulse_width:
                raise ValueError("pulse_width must hold the key 'fixed' (a value, or one value per pulse)")
            fes["pulse_width"] = pulse_width["fixed"]
        if self.family == "hmed2018":
            pulse_intensity = train.get("pulse_intensity")
            if not isinstance(pulse_intensity, dict):
                raise TypeError(f"pulse_intensity must be dict type,"
                                f" currently pulse_intensity is {type(pulse_intensity)}) type.")
            if "fixed" not in pulse_intensity:
                raise ValueError("pulse_intensity must hold the key 'fixed' (a value, or one value per pulse)")
            if isinstance(pulse_intensity["fixed"], bool) or not isinstance(pulse_intensity["fixed"],
                                                                              int | float | list):
                raise ValueError("fixed pulse_intensity must be a int, float or list type.")
            fes["pulse_intensity"] = pulse_intensity["fixed"]
        ivp = IvpFes(fes, {"final_time": final_time, "ode_solver": self.ode_solver})
        force_tracking = train.get("force_tracking")
        if force_tracking is None and "time" in train and "force" in train:
            force_tracking = force_at_node(train["time"], train["force"], ivp.n_shooting, final_time)
        if not isinstance(force_tracking, list):
            raise TypeError(f"force_tracking must be list type,"
                            f" currently force_tracking is {type(force_tracking)}) type.")
        if not all(isinstance(val, int | float) for val in force_tracking):
            raise TypeError("force_tracking must be list of int or float type.")
        if len(force_tracking) != ivp.n_shooting + 1:
            raise ValueError(f"force_tracking has {len(force_tracking)} values, expected one per node: n_shooting + 1 "
                             f"= {ivp.n_shooting + 1}")
        target = np.asarray(force_tracking, dtype=np.float64)
        weight = np.ones(ivp.n_shooting + 1) if train.get("weight") is None else np.asarray(train["weight"],
                                                                                            dtype=np.float64)
        if weight.shape != target.shape:
            raise ValueError("weight must hold one value per node")
        return ivp, target, weight

    def _pack(self, packed) -> dict:
        """SoA arrays of ``cfx_idm_trains`` in launch order (``packed``: ``pack_train`` dicts, already ordered)."""
        E, P, nn = len(packed), self.max_pulses, self.max_shooting + 1
        with_value = packed[0]["value"] is not None
        out = {"times": np.zeros((P, E)), "act_node": np.zeros((P, E), dtype=np.int32),
               "value": np.zeros((P, E)) if with_value else None,
               "n_pulses": np.array([len(t["times"]) for t in packed], dtype=np.int32),
               "truncation": np.array([t["truncation"] for t in packed], dtype=np.int32),
               "n_shooting": np.array([t["n_shooting"] for t in packed], dtype=np.int32),
               "final_time": np.array([t["final_time"] for t in packed], dtype=np.float64),
               "target": np.zeros((nn, E)), "weight": np.zeros((nn, E))}
        for j, t in enumerate(packed):
            n, e = len(t["times"]), int(self.order[j])
            out["times"][:n, j] = t["times"]
            out["act_node"][:n, j] = t["act_node"]
            if with_value:
                out["value"][:n, j] = t["value"]
            out["target"][: t["n_shooting"] + 1, j] = self.targets[e]
            out["weight"][: t["n_shooting"] + 1, j] = self.weights[e]
        return out

    def _handle(self, batch):
        if batch not in self._handles:
            self._handles[batch] = self._HANDLE(
                model_id=self.model.cfx_model_id, constants=self.model.cfx_constants(), scheme=self.ode_solver.scheme,
                n_steps=self.ode_solver.n_integration_steps, batch=batch, n_trains=self.n_trains,
                max_pulses=self.max_pulses, max_shooting=self.max_shooting, device=self.device)
        return self._handles[batch]

    def _device_trains(self, dev):
        """The packed trains on ``dev``, uploaded once per device."""
        import torch

        key = str(torch.device(dev))
        if key not in self._dev_trains:
            self._dev_trains[key] = {k: (None if v is None else torch.as_tensor(v, device=dev))
                                     for k, v in self.trains.items()}
        return self._dev_trains[key]

    # ---- evaluation -----------------------------------------------------------------------------------
    def forces(self, theta, with_sensitivities=False):
        """Per train, in the caller's order: node forces (N_e + 1, B) for parameters theta (n_id, B)
        (cfx_idm_forces); with ``with_sensitivities`` also the list of dF_k / dtheta_j (N_e + 1, n_id, B).  numpy in,
        numpy out; CUDA tensors in, CUDA tensors out."""
        if _cfx._is_tensor(theta):
            B, trains = theta.shape[1], self._device_trains(theta.device)
        else:
            theta = np.ascontiguousarray(theta, dtype=np.float64).reshape(len(self.keys), -1)
            B, trains = theta.shape[1], self.trains
        force, sens = self._handle(B).forces(trains, self.param_ids, theta, with_sens=with_sensitivities)
        inverse = np.argsort(self.order)
        F = [force[int(inverse[e]), : self.n_shooting[e] + 1] for e in range(self.n_trains)]
        if not with_sensitivities:
            return F
        return F, [sens[int(inverse[e]), : self.n_shooting[e] + 1] for e in range(self.n_trains)]

    def solve(self, max_iter=100, gtol=1e-8, xtol=1e-10):
        """Levenberg-Marquardt from every start (``lm_solve``) on the joint cost.  Returns what
        ``FesIdentification.solve`` returns, plus "cost_per_train" (n_trains,), the best start's, and
        ``starts["cost_per_train"]`` (n_starts, n_trains), both in the caller's order of the trains."""
        import torch

        dev = torch.device("cuda", self.device)
        idm = self._handle(self.n_starts)
        n, B = len(self.keys), self.n_starts
        on = lambda a: torch.as_tensor(np.ascontiguousarray(a, dtype=np.float64), device=dev)  # noqa: E731
        with torch.cuda.device(dev):
            trains = self._device_trains(dev)
            new = lambda *sh: torch.empty(sh, dtype=torch.float64, device=dev)  # noqa: E731
            out = (new(B), new(n, B), new(n * (n + 1) // 2, B), None)

            def normal(theta):
                return idm.normal(trains, self.param_ids, theta.contiguous(), out=out)[:3]

            theta, c, iters, status, hist = lm_solve(
                normal, on(self.starts()), on(np.repeat(self.lower[:, None], B, 1)),
                on(np.repeat(self.upper[:, None], B, 1)), max_iter=max_iter, gtol=gtol, xtol=xtol)
            cpt = idm.normal(trains, self.param_ids, theta.contiguous(), per_train=True)[3]
            theta, c, iters, status, hist, cpt = (t.cpu().numpy() for t in (theta, c, iters, status, hist, cpt))
        cpt = cpt[np.argsort(self.order)].T.copy()  # (n_starts, n_trains), caller's order
        ok = np.where(np.isfinite(c), c, np.inf)
        best = int(np.argmin(ok))
        result = dict(self.model.identifiable_parameters)
        for j, key in enumerate(self.keys):
            result[key] = float(theta[j, best])
        result["cost"] = float(c[best])
        result["cost_per_train"] = cpt[best].copy()
        result["best_start"] = best
        result["starts"] = {"theta": theta.T.copy(), "cost": c, "iterations": iters, "status": status,
                            "cost_history": hist, "cost_per_train": cpt}
        return result

    def close(self):
        for h in getattr(self, "_handles", {}).values():
            h.close()
        self._handles, self._dev_trains = {}, {}
        for ivp in getattr(self, "_ivps", []):
            ivp.close()


class FesMultiTrainIdentification(_MultiTrainIdentification):
    """Force-parameter identification of one muscle from SEVERAL measured force curves, each under its own
    stimulation train, over ``n_starts`` starts: one parameter set for all trains (the reference's ``data_path``
    list of recordings).

    ``trains``: a list of dicts, one per recording:
      * ``stim_time``, ``final_time``; ``pulse_width`` (Ding2007) or ``pulse_intensity`` (Hmed2018):
        ``{"fixed": value or one value per pulse}``;
      * ``force_tracking``: the measured force at every node of that train's own ``OcpFes.prepare_n_shooting``,
        or recorded samples ``time`` and ``force`` (interpolated onto the nodes by ``force_at_node``);
      * optional ``weight`` (per node, default 1), ``pulse_mode`` (default "single"), ``sum_stim_truncation``
        (default the model's; no upper limit).
    Every train starts from the rest state.  Every other argument, ``starts``, ``forces``, ``solve`` and ``close``
    are as ``FesIdentification``; ``forces`` returns one array per train, and ``solve`` adds ``"cost_per_train"``
    (the best start's) and ``starts["cost_per_train"]`` (n_starts, n_trains)."""

    def __init__(self, model=None, trains=None, key_parameter_to_identify=None,
                 ode_solver=OdeSolver.RK4(n_integration_steps=10), bounds=None, initial_guess=None, n_starts=64,
                 seed=0, start_spread=0.5, device=0):
        if not isinstance(model, FesModel):
            raise TypeError("model must be a FesModel type")
        if model._with_fatigue:
            raise ValueError("The given model is not valid and should not be including the fatigue equation in the "
                             "model")
        self._setup_trains(model, DEFAULT_VALUES[_family(model)], trains, key_parameter_to_identify, ode_solver,
                           bounds, initial_guess, n_starts, seed, start_spread, device)


class FesMultiTrainFatigueIdentification(_MultiTrainIdentification):
    """Fatigue-parameter identification of one muscle from SEVERAL measured force curves: one set of alpha_a,
    alpha_tau1, alpha_km, tau_fat for all recordings, the force parameters fixed at the model's own values.  This is
    the fit for the recovery time constant: a short fatiguing train holds no recovery (tau_fat is not identifiable
    from 1 s of data, and only loosely from a 5 s burst), a protocol of recordings with a fatiguing burst, rest gaps of
    different lengths and a test burst determines it about 100 x more sharply.

    ``model``: a ``*WithFatigue`` model; ``trains``: the list of dicts of ``FesMultiTrainIdentification`` (a
    recording may hold thousands of nodes; ``sum_stim_truncation`` has no upper limit); keys, default initial guess
    (the model's own value) and default bounds (0.01 x to 100 x that value, in increasing order) are those of
    ``FesFatigueIdentification``.  ``starts``, ``forces`` (one array per train), ``solve`` (with ``"cost_per_train"``)
    and ``close`` are as ``FesMultiTrainIdentification``; every iteration is one ``cfx_idfm_normal`` launch.

    Every train starts from the fatigue rest state [0, 0, A_rest (Ding2007: a_scale), tau1_rest, km_rest].  A
    recording that begins already fatigued is out of scope: its start state would depend on the parameters being
    identified.  Put the rest gap and the test burst into the same recording as the fatiguing burst instead."""

    _PARAM_IDS = _cfx.FATIGUE_PARAM_IDS
    _HANDLE, _TRAIN_CHECK = _cfx.Idfm, staticmethod(_cfx.idfm_check)

    def __init__(self, model=None, trains=None, key_parameter_to_identify=None,
                 ode_solver=OdeSolver.RK4(n_integration_steps=10), bounds=None, initial_guess=None, n_starts=64,
                 seed=0, start_spread=0.5, device=0):
        if not isinstance(model, FesModel):
            raise TypeError("model must be a FesModel type")
        if not model._with_fatigue:
            raise ValueError("The given model is not valid and should be including the fatigue equation in the model")
        own = model.identifiable_parameters
        defaults = {k: (own[k], *sorted((0.01 * own[k], 100.0 * own[k]))) for k in FATIGUE_KEYS}
        self._setup_trains(model, defaults, trains, key_parameter_to_identify, ode_solver, bounds, initial_guess,
                           n_starts, seed, start_spread, device)
