"""Automatic-differentiation oracle for the musculoskeletal NLP callbacks — TEST INFRASTRUCTURE ONLY (CPU, torch
float64).

Nothing in the product imports this module.  It restates, in torch float64 on the CPU, what ``fes_msk`` states in
numpy: the tree kinematics over the parsed bioMod (axes, RT matrices and ancestor sets are plain constants), the
muscle geometry, the De Groote coefficients, the recursive Newton-Euler inverse dynamics in world coordinates with the
mass matrix by unit accelerations (the kernels form M from body Jacobians: the two stay independent), the
``FesMskModel`` right-hand side (the muscle ODEs are ``fes_autodiff.rhs``), the RK sub-stepping
(``fes_autodiff._step``), the sliding-window and marker rows and the objective, fatigue term included.  Everything
is a pure function of tensors built with ``torch.stack`` / ``torch.cat`` and no in-place write, so ``vmap``, ``jacfwd``
and ``jacrev`` go through.

Why it exists: ``fes_msk``'s first derivatives are complex-step and exact to rounding, but the only second-order
reference it allows is a central difference of those gradients (about 1e-7 of a block's largest entry, and an
interval block spans 1e-9 .. 8e9).  ``torch.func`` differentiates the same recursion twice with no step size.

    eval_g(pb, v)                                   (B, ng), fes_msk.eval_g's order
    continuity_jacobian(pb, v)                      (B, N, nx, nz) dense d Phi_k / d z_k
    marker_rows(pb, v), marker_jacobian(pb, v)      (B, n_marker_rows), (B, n_marker_rows, nv)
    eval_f(pb, v), eval_grad_f(pb, v)               (B,), (B, nv)
    lagrangian_hessian(pb, v, obj_factor, lam)      dense symmetric (B, nv, nv): per-interval second-order AD of
                                                    lam_k . Phi_k(z_k), the marker rows' (q_node, q_node) terms and
                                                    the objective (quadratic terms and the fatigue term, differentiated)
    lagrangian_hessian_scale(pb, v, obj_factor, lam)  sum_r |lam_r| |d2 g_r| + |obj_factor| |d2 f|, same shape
    hessian_error(pb, got, ref, scale)              max |got - ref| / max(scale, floor); the floor of an entry is 1e-6
                                                    of the largest reference entry of the same interval block and the
                                                    same unordered pair of variable groups (``variable_groups``), so
                                                    the 8e9 pulse-width entries do not hide the q entries (<= 44)
    worst_entries(pb, got, ref, scale)              the per-entry report of the worst few entries

``mode`` as in ``fes_autodiff``: "fr" (default), "ff", "rr"; the gap between "ff" and "rr" is the reference's noise.
"""

from __future__ import annotations

import numpy as np
import torch
from torch.func import grad, jacfwd, vmap

from . import fes_autodiff as AD
from . import fes_msk as M
from . import fes_oracle as O
from .fes_autodiff import F64, _MODES, _t

GROUPS = ("Cn", "F", "A", "Tau1", "Km", "q", "qdot", "pulse width", "intensity", "residual torque", "parameter")

# --------------------------------------------------------------------------------------
# tree kinematics (fes_msk.forward_kinematics and friends); q: (nq,) tensor
# --------------------------------------------------------------------------------------


def _cross(a, b):
    return torch.stack([a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]])


def _rot4(axis, a):
    c, s = torch.cos(a), torch.sin(a)
    one, zero = torch.ones_like(a), torch.zeros_like(a)
    i, j = {"x": (1, 2), "y": (2, 0), "z": (0, 1)}[axis]
    rows = [[one if r == cc else zero for cc in range(4)] for r in range(4)]
    rows[i][i], rows[i][j], rows[j][i], rows[j][j] = c, -s, s, c
    return torch.stack([torch.stack(r) for r in rows])


def forward_kinematics(bm, q):
    """Global 4x4 frame of every segment, and per dof (global order) its world axis, origin and segment."""
    frames, dofs = {}, []
    qi = 0
    for seg in bm["segments"]:
        T = frames[seg["parent"]] if seg["parent"] else torch.eye(4, dtype=F64)
        T = T @ _t(seg["RT"])
        for ax in seg["rotations"]:
            e = {"x": 0, "y": 1, "z": 2}[ax]
            dofs.append({"axis": T[:3, e], "origin": T[:3, 3], "segment": seg["name"]})
            T = T @ _rot4(ax, q[qi])
            qi += 1
        frames[seg["name"]] = T
    return frames, dofs


def _point_world(frames, seg, p):
    T = frames[seg]
    return T[:3, :3] @ _t(p) + T[:3, 3]


def _point_jacobian(bm, dofs, seg, P):
    """dP/dq (3 x nq) of a point fixed in segment ``seg``: axis_k x (P - origin_k) for the dofs above it."""
    anc = M._ancestors(bm, seg)
    cols = [_cross(d["axis"], P - d["origin"]) if d["segment"] in anc else torch.zeros(3, dtype=F64) for d in dofs]
    return torch.stack(cols, dim=1)


def marker_position(bm, name, q):
    for mk in bm.get("markers", []):
        if mk["name"] == name:
            frames, _ = forward_kinematics(bm, q)
            return _point_world(frames, mk["parent"], mk["position"])
    raise ValueError(f"marker {name!r} is not in the bioMod")


def muscle_geometry(bm, mus, q, qdot, kin=None):
    """(muscle-tendon length, length Jacobian dL/dq (nq,), fibre length, muscle-tendon velocity).  ``kin``: the
    ``forward_kinematics(bm, q)`` of the same q, when the caller already has it."""
    frames, dofs = kin or forward_kinematics(bm, q)
    path = M.muscle_path(mus)
    pts = [_point_world(frames, s, p) for s, p in path]
    jac = [_point_jacobian(bm, dofs, s, P) for (s, _), P in zip(path, pts)]
    L, JL = 0.0, 0.0
    for i in range(len(pts) - 1):
        d = pts[i + 1] - pts[i]
        n = torch.sqrt((d * d).sum())
        L = L + n
        JL = JL + (d @ (jac[i + 1] - jac[i])) / n
    fibre = (L - mus["tendonslacklength"]) / float(np.cos(mus["pennationangle"]))
    vel = JL @ qdot
    return L, JL, fibre, vel


# --------------------------------------------------------------------------------------
# De Groote coefficients (fes_msk.force_length / force_velocity / passive_force)
# --------------------------------------------------------------------------------------


def force_length(norm_length):
    b11, b21, b31, b41 = 0.815, 1.055, 0.162, 0.063
    b12, b22, b32, b42 = 0.433, 0.717, -0.030, 0.200
    b13, b23, b33, b43 = 0.100, 1.000, 0.354, 0.0
    nl = norm_length
    return (b11 * torch.exp((-0.5 * ((nl - b21) * (nl - b21))) / ((b31 + b41 * nl) * (b31 + b41 * nl)))
            + b12 * torch.exp((-0.5 * ((nl - b22) * (nl - b22))) / ((b32 + b42 * nl) * (b32 + b42 * nl)))
            + b13 * torch.exp((-0.5 * ((nl - b23) * (nl - b23))) / ((b33 + b43 * nl) * (b33 + b43 * nl))))


def force_velocity(velocity):
    nv = velocity / 10
    d1, d2, d3, d4 = -0.318, -8.149, -0.374, 0.886
    return d1 * torch.log((d2 * nv + d3) + torch.sqrt((d2 * nv + d3) * (d2 * nv + d3) + 1)) + d4


def passive_force(norm_length):
    """Clipped at 0 on the value: the kink is at norm_length = 1."""
    kpe, e0 = 4, 0.6
    fp = (torch.exp(kpe * (norm_length - 1) / e0) - 1) / (float(np.exp(kpe)) - 1)
    return torch.where(fp > 0, fp, 0 * fp)


# --------------------------------------------------------------------------------------
# rigid-body dynamics (fes_msk._inverse_dynamics: recursive Newton-Euler in world coordinates)
# --------------------------------------------------------------------------------------


def _gyroscopic(w, Iw):
    """The velocity-product term of a body's moment balance."""
    return _cross(w, Iw @ w)


def _link_parents(bm, dofs):
    seg_last_dof = {}
    parent_of = {s["name"]: s["parent"] for s in bm["segments"]}
    link_parent = []
    for k, d in enumerate(dofs):
        s = d["segment"]
        p = k - 1 if (k > 0 and dofs[k - 1]["segment"] == s) else None
        if p is None:
            a = parent_of[s]
            while a is not None and a not in seg_last_dof:
                a = parent_of[a]
            p = seg_last_dof.get(a) if a is not None else None
        link_parent.append(p)
        seg_last_dof[s] = k
    return link_parent, seg_last_dof, parent_of


def _inverse_dynamics(bm, q, qdot, qddot, gravity=True, kin=None):
    """``qdot`` / ``qddot``: tensors (nq,) or sequences of floats."""
    frames, dofs = kin or forward_kinematics(bm, q)
    nq = len(dofs)
    z3 = torch.zeros(3, dtype=F64)
    g = _t(bm["gravity"]) if gravity else z3
    link_parent, seg_last_dof, parent_of = _link_parents(bm, dofs)
    w, al, acc = [], [], []
    for k, d in enumerate(dofs):
        p = link_parent[k]
        wp, alp, ap = (z3, z3, -g) if p is None else (w[p], al[p], acc[p])
        op = z3 if p is None else dofs[p]["origin"]
        r = d["origin"] - op
        w.append(wp + d["axis"] * qdot[k])
        al.append(alp + d["axis"] * qddot[k] + _cross(wp, d["axis"] * qdot[k]))
        acc.append(ap + _cross(alp, r) + _cross(wp, _cross(wp, r)))
    tau = [0.0] * nq
    for seg in bm["segments"]:
        if seg["mass"] == 0 and not np.any(seg["inertia"]):
            continue
        a = seg["name"]
        while a is not None and a not in seg_last_dof:
            a = parent_of[a]
        if a is None:
            continue  # fixed to the ground
        k = seg_last_dof[a]
        T = frames[seg["name"]]
        R = T[:3, :3]
        c = R @ _t(seg["com"]) + T[:3, 3]
        Iw = R @ _t(seg["inertia"]) @ R.T
        r = c - dofs[k]["origin"]
        ac = acc[k] + _cross(al[k], r) + _cross(w[k], _cross(w[k], r))
        Fb = seg["mass"] * ac
        Nb = Iw @ al[k] + _gyroscopic(w[k], Iw)
        j = k
        while j is not None:
            tau[j] = tau[j] + dofs[j]["axis"] @ (_cross(c - dofs[j]["origin"], Fb) + Nb)
            j = link_parent[j]
    return torch.stack([t if torch.is_tensor(t) else torch.zeros((), dtype=F64) + t for t in tau])


def mass_matrix(bm, q, kin=None):
    nq = M.nb_q(bm)
    z = [0.0] * nq
    kin = kin or forward_kinematics(bm, q)
    g0 = _inverse_dynamics(bm, q, z, z, gravity=False, kin=kin)
    cols = [_inverse_dynamics(bm, q, z, [1.0 if i == j else 0.0 for i in range(nq)], gravity=False, kin=kin) - g0
            for j in range(nq)]
    return torch.stack(cols, dim=1)


def _solve(A, b):
    """A x = b by elimination without pivoting (A symmetric positive definite), written out so that the nested
    transforms go through."""
    n = b.shape[0]
    a = [[A[i, j] for j in range(n)] for i in range(n)]
    y = [b[i] for i in range(n)]
    for i in range(n):
        for r in range(i + 1, n):
            f = a[r][i] / a[i][i]
            for c in range(i + 1, n):
                a[r][c] = a[r][c] - f * a[i][c]
            y[r] = y[r] - f * y[i]
    x = [None] * n
    for i in reversed(range(n)):
        s = y[i]
        for c in range(i + 1, n):
            s = s - a[i][c] * x[c]
        x[i] = s / a[i][i]
    return torch.stack(x)


def forward_dynamics(bm, q, qdot, tau, kin=None):
    """qddot = M^-1 (tau - h(q, qdot)), h = ID(q, qdot, 0)."""
    kin = kin or forward_kinematics(bm, q)
    h = _inverse_dynamics(bm, q, qdot, [0.0] * M.nb_q(bm), kin=kin)
    return _solve(mass_matrix(bm, q, kin), tau - h)


# --------------------------------------------------------------------------------------
# FesMskModel right-hand side and one interval's Phi
# --------------------------------------------------------------------------------------


def msk_rhs(pb, t, x, u, row, record=None):
    """fes_msk.msk_rhs for one node: x (nx,), u (nu,), row (T,).  ``record``: a list that receives every muscle's
    normalised fibre length (the kink guard of the passive-force clip)."""
    nq = pb.nq
    q = x[pb.nxm: pb.nxm + nq]
    qdot = x[pb.nxm + nq:]
    JL_rows, F, dx = [], [], []
    off, pw = 0, 0
    kin = forward_kinematics(pb.bm, q)  # one walk of the tree per node, shared by the geometry and the dynamics
    for mus in pb.muscles:
        nxm = O.n_states(mus.model)
        xm = x[off: off + nxm]
        bio = M._bio_muscle(pb, mus.name)
        _, JL, fibre, vel = muscle_geometry(pb.bm, bio, q, qdot, kin)
        nl = fibre / bio["optimallength"]
        if record is not None:
            record.append(nl)
        fl = force_length(nl) if pb.fv_on else 1.0
        fv = force_velocity(vel) if pb.fv_on else 1.0
        fp = passive_force(nl) if pb.fp_on else 0.0
        um = None
        if O.control_kind(mus.model) == "pulse_width":
            um = u[pw: pw + 1]
            pw += 1
        elif O.control_kind(mus.model) == "pulse_intensity":
            um = u[pw: pw + pb.T]
            pw += pb.T
        dx.append(AD.rhs(mus.model, mus.c, t, xm, um, row, fl=fl, fv=fv, fp=fp, legacy=pb.legacy))
        JL_rows.append(JL)
        F.append(xm[1])
        off += nxm
    tau = -(torch.stack(JL_rows).T @ torch.stack(F))
    if pb.residual:
        tau = tau + u[pb.n_pw + pb.n_int: pb.n_pw + pb.n_int + nq]
    qddot = forward_dynamics(pb.bm, q, qdot, tau, kin)
    return torch.cat(dx + [qdot, qddot])


def _interval(pb, record=None):
    """phi(z, t0, row) = Phi_m(x_k, u_k) (nx,); the -x_{k+1} of the continuity rows is added by the callers."""
    nx, h = pb.nx, pb.dt / pb.m

    def phi(z, t0, row):
        x, u = z[:nx], z[nx:]
        f = lambda t, xx: msk_rhs(pb, t, xx, u, row, record)  # noqa: E731
        for j in range(pb.m):
            x = AD._step(pb.scheme, f, t0 + j * h, h, x)
        return x

    return phi


def _interval_inputs(pb, v):
    """z (L, nz), t0 (L,), stim rows (L, T) of every (instance, interval), L = B * N."""
    B, N, nz = v.shape[0], pb.n_shooting, pb.nz
    z = _t(v[:, : N * nz]).reshape(B * N, nz)
    t0 = _t(np.tile(np.arange(N) * pb.dt, B))
    rows = _t(np.tile(pb.rows[:N], (B, 1)))
    return z, t0, rows


def normalised_lengths(pb, v):
    """Every muscle's normalised fibre length at every RK stage input of every (instance, interval), flat."""
    z, t0, rows = _interval_inputs(pb, np.asarray(v, dtype=np.float64))
    rec = []
    phi = _interval(pb, rec)
    for i in range(z.shape[0]):
        phi(z[i], t0[i], rows[i])
    return torch.stack(rec).numpy()


# --------------------------------------------------------------------------------------
# g, its Jacobian blocks, the marker rows
# --------------------------------------------------------------------------------------


def _ngk(pb):
    return pb.nx + pb.n_slide


def _x_off(pb, k):
    return k * pb.nz


def _q_off(pb, node):
    return node * pb.nz + pb.nxm


def sliding_rows(pb, vt, k):
    """fes_msk.sliding_rows on a torch vt (B, nv): (B, n_slide)."""
    B = vt.shape[0]
    P = vt[:, pb.n_shooting * pb.nz + pb.nx:]
    out, off = [], pb.n_pw
    floor = torch.full((B,), float(O.min_pulse_intensity(pb.muscles[0].c)), dtype=F64)
    for mi in range(len(pb.muscles)):
        cols = [P[:, pb.param_offset[mi] + i] for i in range(pb.last_stim_idx[k] + 1)]
        while len(cols) < pb.T:
            cols.insert(0, floor)
        win = torch.stack(cols[len(cols) - pb.T:], dim=1)
        out.append(vt[:, k * pb.nz + pb.nx + off: k * pb.nz + pb.nx + off + pb.T] - win)
        off += pb.T
    return torch.cat(out, dim=1)


def _marker_fns(pb):
    """Per marker pair: (node, fn) with fn(q) the pair's rows (len(axes),)."""
    out = []
    for c in pb.marker_pairs:
        def fn(q, c=c):
            d = marker_position(pb.bm, c["second"], q) - marker_position(pb.bm, c["first"], q)
            return torch.stack([d[a] for a in c["axes"]])
        out.append((c["node"], fn))
    return out


def _q_node(pb, vt, node):
    return vt[:, _q_off(pb, node): _q_off(pb, node) + pb.nq]


def marker_rows(pb, v):
    vt = _t(np.asarray(v, dtype=np.float64))
    return torch.cat([vmap(fn)(_q_node(pb, vt, node)) for node, fn in _marker_fns(pb)], dim=1).numpy()


def marker_jacobian(pb, v):
    """Dense (B, n_marker_rows, nv): forward-mode AD of every pair's rows over q_node."""
    vt = _t(np.asarray(v, dtype=np.float64))
    J = np.zeros((vt.shape[0], pb.n_marker_rows, pb.nv))
    r = 0
    for node, fn in _marker_fns(pb):
        blk = vmap(jacfwd(fn))(_q_node(pb, vt, node)).numpy()
        J[:, r: r + blk.shape[1], _q_off(pb, node): _q_off(pb, node) + pb.nq] = blk
        r += blk.shape[1]
    return J


def eval_g(pb, v):
    """Constraint vector in fes_msk.eval_g's order, (B, ng)."""
    v = np.asarray(v, dtype=np.float64)
    B, N, nx, nz = v.shape[0], pb.n_shooting, pb.nx, pb.nz
    z, t0, rows = _interval_inputs(pb, v)
    r = vmap(_interval(pb))(z, t0, rows).reshape(B, N, nx)
    vt = _t(v)
    nxt = torch.stack([vt[:, (k + 1) * nz: (k + 1) * nz + nx] for k in range(N)], dim=1)
    r = r - nxt
    if pb.n_slide:
        r = torch.cat([r, torch.stack([sliding_rows(pb, vt, k) for k in range(N)], dim=1)], dim=2)
    g = r.reshape(B, -1).numpy()
    return np.concatenate([g, marker_rows(pb, v)], axis=1) if pb.marker_pairs else g


def continuity_jacobian(pb, v):
    """Dense d Phi(x_k, u_k) / d(x_k, u_k) of every interval, (B, N, nx, nz), forward mode."""
    v = np.asarray(v, dtype=np.float64)
    z, t0, rows = _interval_inputs(pb, v)
    return vmap(jacfwd(_interval(pb)))(z, t0, rows).reshape(v.shape[0], pb.n_shooting, pb.nx, pb.nz).numpy()


# --------------------------------------------------------------------------------------
# objective: the quadratic terms and fatigue_weight * sum (a_rest / A_N)^2
# --------------------------------------------------------------------------------------


def _objective(pb):
    N, nx, nz = pb.n_shooting, pb.nx, pb.nz
    offs, ws, tgts = [], [], []
    for o in pb.objectives:
        for k in range(o["node_first"], o["node_last"] + 1):
            tgt = o["target"][k] if o.get("target") is not None else o.get("target_value", 0.0)
            offs.append(k * nz + o["var_index"] + (0 if o["var_kind"] == 0 else nx))
            ws.append(o["weight"] * (pb.dt if o["kind"] == 0 else 1.0))
            tgts.append(float(tgt))
    offs = torch.tensor(offs, dtype=torch.int64)
    ws, tgts = torch.tensor(ws, dtype=F64), torch.tensor(tgts, dtype=F64)
    fat, off = [], 0
    for mus in pb.muscles:
        if O.n_states(mus.model) == 5:
            fat.append((N * nz + off + 2, mus.c["a_rest"]))
        off += O.n_states(mus.model)

    def f(v):
        out = (ws * (v[offs] - tgts) ** 2).sum() if len(offs) else (v * 0.0).sum()
        if pb.fatigue_weight:
            for i, a_rest in fat:
                out = out + pb.fatigue_weight * (a_rest / v[i]) ** 2
        return out

    return f


def eval_f(pb, v):
    return vmap(_objective(pb))(_t(np.asarray(v, dtype=np.float64))).numpy()


def eval_grad_f(pb, v):
    return vmap(grad(_objective(pb)))(_t(np.asarray(v, dtype=np.float64))).numpy()


def objective_hessian(pb, v, mode="fr"):
    """(B, nv, nv), second-order AD of the objective."""
    outer, inner = _MODES[mode]
    return vmap(outer(inner(_objective(pb))))(_t(np.asarray(v, dtype=np.float64))).numpy()


# --------------------------------------------------------------------------------------
# Lagrangian Hessian, dense
# --------------------------------------------------------------------------------------


def _lam_parts(pb, lam):
    """Multipliers of the continuity rows (L, nx) and of the marker rows (B, n_marker_rows)."""
    lam = np.asarray(lam, dtype=np.float64)
    B, N = lam.shape[0], pb.n_shooting
    body = lam[:, : N * _ngk(pb)].reshape(B, N, _ngk(pb))[:, :, : pb.nx]
    return _t(body).reshape(B * N, pb.nx), _t(lam[:, N * _ngk(pb):])


def hessian_blocks(pb, v, lam, mode="fr"):
    """(B, N, nz, nz): Hessian over z_k of lam_k . Phi_k(z_k), by second-order AD."""
    v = np.asarray(v, dtype=np.float64)
    outer, inner = _MODES[mode]
    fn = _interval(pb)
    z, t0, rows = _interval_inputs(pb, v)
    w, _ = _lam_parts(pb, lam)
    scalar = lambda zz, ww, tt, rr: (ww * fn(zz, tt, rr)).sum()  # noqa: E731
    H = vmap(outer(inner(scalar)))(z, w, t0, rows)
    return H.reshape(v.shape[0], pb.n_shooting, pb.nz, pb.nz).numpy()


def _assemble(pb, blocks, marker_blocks, obj):
    B, N, nz = blocks.shape[0], pb.n_shooting, pb.nz
    H = np.array(obj, dtype=np.float64, copy=True)
    for k in range(N):
        H[:, k * nz: (k + 1) * nz, k * nz: (k + 1) * nz] += blocks[:, k]
    for node, blk in marker_blocks:
        o = _q_off(pb, node)
        H[:, o: o + pb.nq, o: o + pb.nq] += blk
    assert H.shape == (B, pb.nv, pb.nv)
    return H


def lagrangian_hessian(pb, v, obj_factor, lam, mode="fr"):
    """obj_factor * Hess(f) + sum_r lam_r Hess(g_r), dense symmetric (B, nv, nv)."""
    v = np.asarray(v, dtype=np.float64)
    of = np.broadcast_to(np.asarray(obj_factor, dtype=np.float64), (v.shape[0],))
    outer, inner = _MODES[mode]
    _, wm = _lam_parts(pb, lam)
    vt = _t(v)
    mk, r = [], 0
    for node, fn in _marker_fns(pb):
        n = len(fn(torch.zeros(pb.nq, dtype=F64)))
        scalar = lambda q, ww, fn=fn: (ww * fn(q)).sum()  # noqa: E731
        mk.append((node, vmap(outer(inner(scalar)))(_q_node(pb, vt, node), wm[:, r: r + n]).numpy()))
        r += n
    H = _assemble(pb, hessian_blocks(pb, v, lam, mode), mk, of[:, None, None] * objective_hessian(pb, v, mode))
    return 0.5 * (H + H.transpose(0, 2, 1))


def lagrangian_hessian_scale(pb, v, obj_factor, lam):
    """sum_r |lam_r| |d2 g_r / dv_i dv_j| + |obj_factor| |d2 f / dv_i dv_j| from the per-row Hessians, (B, nv, nv)."""
    v = np.asarray(v, dtype=np.float64)
    of = np.broadcast_to(np.asarray(obj_factor, dtype=np.float64), (v.shape[0],))
    jf, jr = _MODES["fr"]
    z, t0, rows = _interval_inputs(pb, v)
    w, wm = _lam_parts(pb, lam)
    Hr = vmap(jf(jr(_interval(pb))))(z, t0, rows)  # (L, nx, nz, nz)
    S = torch.einsum("lr,lrij->lij", w.abs(), Hr.abs()).reshape(v.shape[0], pb.n_shooting, pb.nz, pb.nz).numpy()
    vt = _t(v)
    mk, r = [], 0
    for node, fn in _marker_fns(pb):
        Hm = vmap(jf(jr(fn)))(_q_node(pb, vt, node))  # (B, rows, nq, nq)
        n = Hm.shape[1]
        mk.append((node, torch.einsum("br,brij->bij", wm[:, r: r + n].abs(), Hm.abs()).numpy()))
        r += n
    return _assemble(pb, S, mk, np.abs(of)[:, None, None] * np.abs(objective_hessian(pb, v)))


# --------------------------------------------------------------------------------------
# the comparison
# --------------------------------------------------------------------------------------


def variable_groups(pb):
    """(block, group) of every decision variable: block k for z_k, N for x_N and the parameters; group an index into
    ``GROUPS`` (muscle states by kind across muscles)."""
    node = []
    for mus in pb.muscles:
        node += list(range(O.n_states(mus.model)))
    node += [5] * pb.nq + [6] * pb.nq
    ctrl = [7] * pb.n_pw + [8] * pb.n_int + [9] * (pb.nq if pb.residual else 0)
    N = pb.n_shooting
    group = (node + ctrl) * N + node + [10] * pb.n_params
    block = [k for k in range(N) for _ in range(pb.nz)] + [N] * (pb.nx + pb.n_params)
    assert len(group) == pb.nv == len(block)
    return np.array(block), np.array(group)


def _entry_keys(pb):
    """An integer per (i, j) naming (block_i, block_j, unordered group pair), made dense by np.unique."""
    block, group = variable_groups(pb)
    G, nb = len(GROUPS), pb.n_shooting + 1
    lo, hi = np.minimum.outer(group, group), np.maximum.outer(group, group)
    bl, bh = np.minimum.outer(block, block), np.maximum.outer(block, block)
    key = ((bl * nb + bh) * G + lo) * G + hi
    _, inv = np.unique(key.ravel(), return_inverse=True)
    return inv.reshape(-1), int(inv.max()) + 1


def _scaled_error(pb, got, ref, scale, floor):
    got, ref, scale = np.asarray(got), np.asarray(ref), np.asarray(scale)
    inv, nkey = _entry_keys(pb)
    out = np.empty_like(ref)
    for b in range(ref.shape[0]):
        mx = np.zeros(nkey)
        np.maximum.at(mx, inv, np.abs(ref[b]).ravel())
        s = np.maximum(scale[b], (floor * mx[inv]).reshape(ref[b].shape)) + 1e-300
        out[b] = np.abs(got[b] - ref[b]) / s
    return out


def hessian_error(pb, got, ref, scale, floor=1e-6):
    """max over entries of |got - ref| / max(scale, floor * largest |ref| among the entries of the same interval
    block with the same unordered pair of variable groups).  Where both are zero (a group pair whose reference is
    identically zero, an entry that couples two blocks) the match must be exact."""
    return float(np.max(_scaled_error(pb, got, ref, scale, floor)))


def worst_entries(pb, got, ref, scale, instances=None, n=5, floor=1e-6):
    """Lines naming the n worst entries: instance, interval, group pair, variable indices, got, ref, scale."""
    e = _scaled_error(pb, got, ref, scale, floor)
    block, group = variable_groups(pb)
    lines = []
    for flat in np.argsort(e, axis=None)[::-1][:n]:
        b, i, j = np.unravel_index(flat, e.shape)
        inst = b if instances is None else instances[b]
        lines.append(f"instance {inst} interval {block[i]}/{block[j]} ({GROUPS[group[i]]}, {GROUPS[group[j]]}) "
                     f"v[{i}], v[{j}] (in block {i - block[i] * pb.nz}, {j - block[j] * pb.nz}): "
                     f"got {np.asarray(got)[b, i, j]:.17g} ref {ref[b, i, j]:.17g} scale {scale[b, i, j]:.3e} "
                     f"error {e[b, i, j]:.3e}")
    return lines
