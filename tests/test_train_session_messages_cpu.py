"""The argument checks that the three stimulation-train families share (cfx_sweep_check, cfx_sweep_target_check,
cfx_idm_check, cfx_idfm_check), without a device: every bad input gives exactly this code and this message.  The
families reuse one set of train rules; the rows pin what each family makes of them (an "instance" of a sweep is a
"train" of an identification, the parameter-list messages carry the caller's name).  Cases that the families' own CPU
tests already assert are not repeated here."""

import ctypes as C

import numpy as np
import pytest

EINVAL, EUNSUPPORTED = -1, -4  # CFX_EINVAL, CFX_EUNSUPPORTED of include/cfx.h (checked against _cfx below)
B, E, P, NMAX, M = 3, 2, 3, 4, 2
D03, D03F, D07, D07F, H18F = 0, 1, 2, 3, 5


def _arrays(n):
    """Valid arrays of n trains (a sweep: n instances): three pulses, four intervals."""
    return {"times": np.tile(np.array([[0.0], [0.1], [0.2]]), (1, n)),
            "act_node": np.tile(np.array([[0], [1], [2]], dtype=np.int32), (1, n)),
            "value": np.full((P, n), 4e-4),
            "n_pulses": np.full(n, P, dtype=np.int32), "truncation": np.full(n, 2, dtype=np.int32),
            "n_shooting": np.full(n, NMAX, dtype=np.int32), "final_time": np.full(n, 0.4),
            "target": np.full((NMAX + 1, n), 10.0), "weight": np.ones((NMAX + 1, n))}


def _run(family, args, edit, ids):
    """(code, message) of the family's check.  args: the scalar arguments that differ from a valid call; edit:
    (array, index, value), (array, None) for a NULL array, "no trains" or None."""
    from cocofest_amd import _cfx

    assert (_cfx.EINVAL, _cfx.EUNSUPPORTED) == (EINVAL, EUNSUPPORTED)
    lib = _cfx.load_library()
    if family == "target":
        y = np.asarray(args["y"], dtype=np.float64)
        tg = _cfx.SweepTarget(_cfx._ptr(y) if args.get("y_given", True) else None, args.get("n", y.size), args["dt"])
        return lib.cfx_sweep_target_check(C.byref(tg)), lib.cfx_last_error(None).decode()
    sweep = family == "sweep"
    n = B if sweep else E
    a = dict(model=D07 if family != "idfm" else D07F, scheme=4, n_steps=M, batch=B, n_trains=E, max_pulses=P,
             max_shooting=NMAX)
    a.update(args)
    arr = _arrays(n)
    st = (_cfx.SweepTrains if sweep else _cfx.IdmTrains)()
    null = edit[0] if edit not in (None, "no trains") and edit[1] is None else None
    if null is None and edit not in (None, "no trains"):
        arr[edit[0]][edit[1]] = edit[2]
    for name, _ in st._fields_:
        if name != null:
            setattr(st, name, _cfx._ptr(arr[name]))
    trains = None if edit == "no trains" else C.byref(st)
    if sweep:
        rc = lib.cfx_sweep_check(a["model"], a["scheme"], a["n_steps"], a["batch"], a["max_pulses"], a["max_shooting"],
                                 trains)
    else:
        idv = np.asarray(ids, dtype=np.int32)
        rc = getattr(lib, f"cfx_{family}_check")(a["model"], a["scheme"], a["n_steps"], a["batch"], a["n_trains"],
                                                 a["max_pulses"], a["max_shooting"], idv.size,
                                                 idv.ctypes.data_as(C.POINTER(C.c_int32)), trains)
    return rc, lib.cfx_last_error(None).decode()


POS = "n_steps, batch, max_pulses and max_shooting must be positive"
# family, scalar arguments, edit of the arrays, parameter ids, code, message
ROWS = [
    # creation arguments
    ("sweep", dict(model=7), "no trains", None, EINVAL, "cfx_sweep_check: unknown model"),
    ("idm", dict(model=-2), "no trains", [1], EINVAL, "cfx_idm_check: unknown model"),
    ("idfm", dict(model=9), None, [1], EINVAL, "cfx_idfm_check: unknown model"),
    ("idm", dict(model=H18F), None, [1], EUNSUPPORTED,
     "cfx_idm_check: identification is not available for the fatigue models"),
    ("idfm", dict(model=D03), None, [1], EUNSUPPORTED,
     "cfx_idfm_check: fatigue-parameter identification is only available for the fatigue models"),
    ("sweep", dict(scheme=0), None, None, EINVAL,
     "cfx_sweep_check: unknown scheme (must be CFX_RK1, CFX_RK2 or CFX_RK4)"),
    ("idm", dict(scheme=17), None, [1], EINVAL, "cfx_idm_check: unknown scheme (must be CFX_RK1, CFX_RK2 or CFX_RK4)"),
    ("idfm", dict(scheme=5), None, [1], EINVAL, "cfx_idfm_check: unknown scheme (must be CFX_RK1, CFX_RK2 or CFX_RK4)"),
    ("sweep", dict(batch=0), "no trains", None, EINVAL, "cfx_sweep_check: " + POS),
    ("idm", dict(batch=-1), None, [1], EINVAL, "cfx_idm_check: " + POS),
    ("idfm", dict(batch=0), None, [1], EINVAL, "cfx_idfm_check: " + POS),
    ("idm", dict(max_pulses=0), "no trains", [1], EINVAL, "cfx_idm_check: " + POS),
    ("idm", dict(n_trains=-3), "no trains", [1], EINVAL, "cfx_idm_check: n_trains must be positive"),
    ("idm", dict(n_trains=65536), "no trains", [1], EINVAL, "cfx_idm_check: n_trains must be <= 65535"),
    ("idfm", dict(n_trains=-1), "no trains", [1], EINVAL, "cfx_idfm_check: n_trains must be positive"),
    ("idfm", dict(n_trains=70000), "no trains", [1], EINVAL, "cfx_idfm_check: n_trains must be <= 65535"),
    ("sweep", dict(max_shooting=70000), "no trains", None, EINVAL, "cfx_sweep_check: max_shooting must be <= 65535"),
    ("idm", dict(max_shooting=65536), "no trains", [1], EINVAL, "cfx_idm_check: max_shooting must be <= 65535"),
    ("idfm", dict(max_shooting=65536), "no trains", [1], EINVAL, "cfx_idfm_check: max_shooting must be <= 65535"),
    # the order of the checks: the family before the train count, the parameter list before the batch
    ("idm", dict(model=D03F, n_trains=0), None, [1], EUNSUPPORTED,
     "cfx_idm_check: identification is not available for the fatigue models"),
    ("idfm", dict(batch=0), None, [1, 1], EINVAL, "cfx_idfm_check: duplicate parameter id 1"),
    # a NULL array
    ("sweep", {}, ("times", None), None, EINVAL, "cfx_sweep_check: a train array is NULL"),
    ("sweep", {}, ("value", None), None, EINVAL, "cfx_sweep_check: a train array is NULL"),
    ("idm", {}, ("n_shooting", None), [1], EINVAL, "cfx_idm_check: a train array is NULL"),
    ("idm", {}, ("value", None), [1], EINVAL, "cfx_idm_check: a train array is NULL"),
    ("idfm", {}, ("final_time", None), [1], EINVAL, "cfx_idfm_check: a train array is NULL"),
    # the train rules: "instance" for a sweep, "train" for an identification
    ("sweep", {}, ("n_shooting", 2, 0), None, EINVAL,
     "cfx_sweep_check: instance 2: n_shooting must be in [1, max_shooting]"),
    ("idm", {}, ("n_shooting", 1, 5), [1], EINVAL, "cfx_idm_check: train 1: n_shooting must be in [1, max_shooting]"),
    ("idfm", {}, ("n_shooting", 0, 0), [1], EINVAL, "cfx_idfm_check: train 0: n_shooting must be in [1, max_shooting]"),
    ("idm", {}, ("n_shooting", 1, 65536), [1], EINVAL, "cfx_idm_check: train 1: n_shooting must be <= 65535"),
    ("sweep", {}, ("n_pulses", 1, 4), None, EINVAL, "cfx_sweep_check: instance 1: n_pulses must be in [0, max_pulses]"),
    ("idm", {}, ("n_pulses", 0, 4), [1], EINVAL, "cfx_idm_check: train 0: n_pulses must be in [0, max_pulses]"),
    ("idfm", {}, ("n_pulses", 1, -1), [1], EINVAL, "cfx_idfm_check: train 1: n_pulses must be in [0, max_pulses]"),
    ("idm", {}, ("truncation", 1, 0), [1], EINVAL, "cfx_idm_check: train 1: truncation must be >= 1"),
    ("idfm", {}, ("final_time", 0, np.inf), [1], EINVAL,
     "cfx_idfm_check: train 0: final_time must be positive and finite"),
    ("sweep", {}, ("times", (1, 2), -0.5), None, EINVAL, "cfx_sweep_check: instance 2: pulse 1: time decreases"),
    ("idm", {}, ("times", (2, 1), 0.05), [1], EINVAL, "cfx_idm_check: train 1: pulse 2: time decreases"),
    ("idfm", {}, ("times", (1, 0), -1.0), [1], EINVAL, "cfx_idfm_check: train 0: pulse 1: time decreases"),
    ("idm", {}, ("times", (0, 1), np.nan), [1], EINVAL, "cfx_idm_check: train 1: pulse 0: time is not finite"),
    ("sweep", {}, ("act_node", (2, 0), 0), None, EINVAL,
     "cfx_sweep_check: instance 0: pulse 2: activation node decreases"),
    ("idm", {}, ("act_node", (1, 1), -1), [1], EINVAL,
     "cfx_idm_check: train 1: pulse 1: activation node is negative"),
    ("idm", {}, ("act_node", (2, 0), 0), [1], EINVAL, "cfx_idm_check: train 0: pulse 2: activation node decreases"),
    ("idfm", {}, ("act_node", (2, 1), 0), [1], EINVAL, "cfx_idfm_check: train 1: pulse 2: activation node decreases"),
    ("sweep", {}, ("act_node", (2, 1), 5), None, EINVAL,
     "cfx_sweep_check: instance 1: pulse 2: activation node past n_shooting"),
    ("idm", {}, ("act_node", (2, 1), 5), [1], EINVAL,
     "cfx_idm_check: train 1: pulse 2: activation node past n_shooting"),
    ("idfm", {}, ("act_node", (2, 0), 7), [1], EINVAL,
     "cfx_idfm_check: train 0: pulse 2: activation node past n_shooting"),
    ("sweep", {}, ("value", (2, 2), np.nan), None, EINVAL, "cfx_sweep_check: instance 2: pulse 2: value is not finite"),
    ("idm", {}, ("value", (0, 1), np.inf), [1], EINVAL, "cfx_idm_check: train 1: pulse 0: value is not finite"),
    ("idfm", dict(model=H18F), ("value", (1, 0), -np.inf), [1], EINVAL,
     "cfx_idfm_check: train 0: pulse 1: value is not finite"),
    # target and weight of an identification
    ("idm", {}, ("target", (3, 1), np.nan), [1], EINVAL, "cfx_idm_check: train 1: node 3: target is not finite"),
    ("idfm", {}, ("target", (0, 0), np.inf), [1], EINVAL, "cfx_idfm_check: train 0: node 0: target is not finite"),
    ("idm", {}, ("weight", (4, 0), -1e-9), [1], EINVAL, "cfx_idm_check: train 0: node 4: weight must be finite and >= 0"),
    ("idfm", {}, ("weight", (2, 1), np.nan), [1], EINVAL,
     "cfx_idfm_check: train 1: node 2: weight must be finite and >= 0"),
    # the parameter lists: cfx_id_check's and cfx_idf_check's messages under the caller's name
    ("idm", {}, None, [3, 3], EINVAL, "cfx_idm_check: duplicate parameter id 3"),
    ("idm", {}, None, [1, -1], EINVAL, "cfx_idm_check: unknown parameter id -1"),
    ("idm", {}, None, [7], EINVAL, "cfx_idm_check: parameter id 7 is not a parameter of model 2"),
    ("idm", {}, None, list(range(9)), EINVAL, "cfx_idm_check: n_id must be in [1, 8]"),
    ("idfm", {}, None, [2, 0, 2], EINVAL, "cfx_idfm_check: duplicate parameter id 2"),
    ("idfm", {}, None, [-1], EINVAL, "cfx_idfm_check: unknown parameter id -1"),
    # the target force of a score
    ("target", dict(y=[1.0, np.nan, 2.0], dt=0.1), None, None, EINVAL,
     "cfx_sweep_target_check: target: y[1] is not finite"),
    ("target", dict(y=[np.inf], dt=0.0), None, None, EINVAL, "cfx_sweep_target_check: target: y[0] is not finite"),
    ("target", dict(y=[1.0, 2.0], dt=-0.5), None, None, EINVAL,
     "cfx_sweep_target_check: target: sample_dt must be positive"),
    ("target", dict(y=[1.0], n=0, dt=0.1), None, None, EINVAL, "cfx_sweep_target_check: target: n_samples must be >= 1"),
    ("target", dict(y=[1.0], y_given=False, dt=0.1), None, None, EINVAL, "cfx_sweep_target_check: target: y is NULL"),
]


@pytest.mark.parametrize("row", ROWS, ids=[f"{i:02d}-{r[0]}" for i, r in enumerate(ROWS)])
def test_code_and_message(row):
    family, args, edit, ids, code, message = row
    got = _run(family, args, edit, ids)
    print(got)
    assert got == (code, message)


def test_valid_inputs_pass():
    """The unedited arrays of the table are accepted by every family, with and without the optional arrays."""
    for family, ids in (("sweep", None), ("idm", [1, 3]), ("idfm", [0, 3])):
        assert _run(family, {}, None, ids)[0] == 0
        assert _run(family, {}, "no trains", ids)[0] == 0
    assert _run("sweep", dict(model=D03), ("value", None), None)[0] == 0  # Ding2003 reads no per-pulse value
    assert _run("idm", dict(model=D03), ("value", None), [1])[0] == 0
    assert _run("idfm", dict(model=D03F), ("value", None), [1])[0] == 0
    assert _run("idm", {}, ("target", None), [1])[0] == 0  # cfx_idm_forces takes no target
    assert _run("target", dict(y=[1.0, 2.0], dt=0.5), None, None)[0] == 0
