"""The session that cfx_sweep, cfx_idm and cfx_idfm share (device, stream, staging buffers, error string), through
every entry point that stages trains: host arrays and CUDA tensors give the same bits, a session can be called again,
a call refused on the host leaves the session usable, and close() twice is harmless.

The smallest shapes with every staging branch: B = 3 starts or instances, E = 2 trains of an identification,
max_pulses = 3, max_shooting = 4, trains with 4 and with 2 intervals, one train without a pulse, RK4 x 2 sub-steps, a
model that reads a per-pulse value (Ding2007) and one that does not (Ding2003: ``value`` is NULL).  Every comparison is
bitwise, so there is no tolerance; every bad input is refused on the host before any launch."""

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

B, E, P, NMAX, M = 3, 2, 3, 4, 2
CALLS = ("sweep.integrate", "sweep.score", "idm.forces", "idm.normal", "idfm.forces", "idfm.normal")
MODEL = {("sweep", False): "ding2003", ("sweep", True): "ding2007_with_fatigue",
         ("idm", False): "ding2003", ("idm", True): "ding2007",
         ("idfm", False): "ding2003_with_fatigue", ("idfm", True): "ding2007_with_fatigue"}


def _trains(n, value):
    """n trains: 4 intervals and 3 pulses, 2 intervals (n = 3: and 2 pulses), the last one without a pulse."""
    tr = {"times": np.tile(np.array([[0.0], [0.1], [0.2]]), (1, n)),
          "act_node": np.tile(np.array([[0], [1], [2]], dtype=np.int32), (1, n)),
          "n_pulses": np.array([3, 0] if n == 2 else [3, 2, 0], dtype=np.int32),
          "truncation": np.full(n, 2, dtype=np.int32),
          "n_shooting": np.array([4, 2, 4][:n], dtype=np.int32), "final_time": np.full(n, 0.4)}
    tr["times"][:, 1] = [0.0, 0.2, 0.3]  # two intervals of 0.2: the second pulse is visible from node 1
    if value:
        tr["value"] = np.array([[3e-4, 4e-4, 5e-4][:n], [4e-4, 5e-4, 6e-4][:n], [5e-4, 6e-4, 3e-4][:n]])
    return tr


def _setup(call, value):
    """(object, trains, the call's other arguments, the C entry point's name)."""
    from cocofest_amd import _cfx
    from oracle import fes_oracle as O

    family, kind = call.split(".")
    name = MODEL[family, value]
    c = dict(O.model_constants(name), fl=1.0, fv=1.0, fp=0.0)
    common = dict(model_id=_cfx.MODEL_IDS[name], constants=c, scheme=_cfx.RK4, n_steps=M, batch=B, max_pulses=P,
                  max_shooting=NMAX)
    if family == "sweep":
        obj = _cfx.Sweep(**common)
        rest = [0.01, 5.0] + ([c["a_scale" if value else "a_rest"], c["tau1_rest"], c["km_rest"]] if obj.nx == 5 else [])
        args = {"x0": np.array(rest)[:, None] * np.array([1.0, 1.1, 0.9])}
        if kind == "score":
            args["target"] = np.array([0.0, 20.0, 40.0, 30.0, 10.0])
        return obj, _trains(B, value), args, f"cfx_sweep_{kind}"
    obj = (_cfx.Idm if family == "idm" else _cfx.Idfm)(n_trains=E, **common)
    keys, table = (("km_rest", "tau2"), _cfx.PARAM_IDS) if family == "idm" else (("alpha_a", "tau_fat"),
                                                                                 _cfx.FATIGUE_PARAM_IDS)
    trains = _trains(E, value)
    if kind == "normal":
        trains["target"] = np.linspace(0.0, 50.0, (NMAX + 1) * E).reshape(NMAX + 1, E)
        trains["weight"] = np.linspace(0.5, 1.5, (NMAX + 1) * E).reshape(NMAX + 1, E)
    args = {"ids": [table[k] for k in keys],
            "theta": np.array([[c[k]] for k in keys]) * np.array([1.0, 1.1, 0.9])}
    return obj, trains, args, f"cfx_{family}_{kind}"


def _bytes(call, obj, trains, args):
    """Every output of the call, as bytes."""
    if call == "sweep.integrate":
        out = obj.integrate(trains, x0=args["x0"], nodes=True)
    elif call == "sweep.score":
        out = obj.score(trains, args["target"], 0.1, x0=args["x0"])
    elif call.endswith("forces"):
        out = obj.forces(trains, args["ids"], args["theta"], with_sens=True)
    else:
        out = obj.normal(trains, args["ids"], args["theta"], per_train=True)
    assert all(o is not None for o in out)
    return tuple((o if isinstance(o, np.ndarray) else o.cpu().numpy()).tobytes() for o in out)


def _on_device(d):
    import torch

    return {k: torch.as_tensor(v, device="cuda:0") if isinstance(v, np.ndarray) else v for k, v in d.items()}


@pytest.mark.parametrize("value", [False, True], ids=["no-value", "value"])
@pytest.mark.parametrize("call", CALLS)
def test_session(call, value):
    from cocofest_amd import CfxError, _cfx

    obj, trains, args, entry = _setup(call, value)
    assert ("value" in trains) == value
    host = _bytes(call, obj, trains, args)
    # (a) CUDA tensors, used in place on torch's stream, against the staged host arrays
    assert _bytes(call, obj, _on_device(trains), _on_device(args)) == host
    # (b) the staging buffers a second time
    assert _bytes(call, obj, trains, args) == host
    # (c) a call refused on the host, then a good one
    bad_key = "x0" if call.startswith("sweep") else "theta"
    bad = dict(args, **{bad_key: args[bad_key].copy()})
    bad[bad_key][-1, 1] = np.inf
    with pytest.raises(CfxError) as exc:
        _bytes(call, obj, trains, bad)
    assert exc.value.code == _cfx.EINVAL
    assert str(exc.value) == f"libcfx error {_cfx.EINVAL}: {entry}: {bad_key} is not finite"
    assert _bytes(call, obj, trains, args) == host
    # (d)
    obj.close()
    obj.close()
