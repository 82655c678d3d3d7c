"""torch.autograd through the batched dynamics: ``rnea`` and ``aba`` as differentiable functions of (q, qd, qdd | tau), ``integrate`` and
``step`` (forward dynamics, then the integrator) as differentiable functions of the state, and the maps between velocity-space gradients
and the raw coordinates.

The forward passes are ``HipModel.rnea`` / ``HipModel.aba`` / ``HipModel.integrate`` / ``HipModel.step`` unchanged; a backward pass is ONE
call of ``HipModel.rnea_vjp`` / ``HipModel.aba_vjp`` / ``HipModel.integrate_vjp`` / ``HipModel.step_vjp`` (no nv x nv matrix is formed)
plus ``chart_pullback`` for q, and ``chart_cotangent`` at the new configuration for the two steps.
``rnea_parameters`` and ``aba_parameters`` are the per-configuration-parameter calls as differentiable functions of **pi**: their backward
is ONE call of ``HipModel.rnea_parameters_vjp`` / ``HipModel.aba_parameters_vjp`` (no regressor is formed).  They are not differentiable
with respect to the state: a q, qd, qdd or tau that requires grad raises NotImplementedError.
``rnea_parameters_state``, ``aba_parameters_state`` and ``step_parameters`` are the same calls as differentiable functions of the state
AND pi: their backward is ONE call of ``HipModel.rnea_parameters_state_vjp`` / ``HipModel.aba_parameters_state_vjp`` that asks for exactly
the gradients needed, plus ``chart_pullback`` for q.  Use them where the state requires grad -- a rollout of robots whose parameters
are being learned.
``body_poses`` carries gradients from where the bodies are back to q: the forward pass is ``HipModel.body_poses`` unchanged, the backward
pass ONE call of ``HipModel.body_poses_vjp`` (no 6 K x nv Jacobian is formed) plus ``chart_pullback``.
AoS device tensors, fp64 or fp32.  gravity and f_ext are not differentiated.  Once differentiable: the backward pass is not itself a
graph of torch operations, and a second backward raises.
"""
from __future__ import annotations

import torch
from torch.autograd.function import once_differentiable

REVOLUTE, PRISMATIC, SIXDOF, FIXED, PLANAR, SPHERICAL = range(6)
_NDOF = {REVOLUTE: 1, PRISMATIC: 1, SIXDOF: 6, FIXED: 0, PLANAR: 3, SPHERICAL: 3}
_NCFG = {REVOLUTE: 1, PRISMATIC: 1, SIXDOF: 7, FIXED: 0, PLANAR: 3, SPHERICAL: 4}


def chart_maps(desc):
    """Index lists of ``chart_pullback`` from a ModelDesc: per joint kind the entries of q and of a velocity-space vector."""
    m = dict(one_q=[], one_v=[], quat_q=[], quat_v=[], lin_quat=[], lin_q=[], lin_v=[], pl_q=[], pl_v=[])
    d = c = 0
    for t in (int(t) for t in desc.joint_type):
        dj, cj = [int(x) for x in desc.dof_indices[d:d + _NDOF[t]]], [int(x) for x in desc.cfg_indices[c:c + _NCFG[t]]]
        d, c = d + _NDOF[t], c + _NCFG[t]
        if t in (REVOLUTE, PRISMATIC):
            m["one_q"] += cj
            m["one_v"] += dj
        elif t in (SIXDOF, SPHERICAL):
            if t == SIXDOF:
                m["lin_quat"].append(len(m["quat_q"]))
                m["lin_q"].append(cj[4:7])
                m["lin_v"].append(dj[3:6])
            m["quat_q"].append(cj[:4])
            m["quat_v"].append(dj[:3])
        elif t == PLANAR:
            m["pl_q"].append(cj)
            m["pl_v"].append(dj)
    return m


def chart_pullback(desc, q, g, maps=None):
    """The gradient with respect to the raw coordinates q [B, nq] from a velocity-space gradient g [B, nv] (gq of ``rnea_vjp`` /
    ``aba_vjp``, or u^T D for a matrix D of the derivative calls): exact for q_raw -> L(q_raw), given that the engine normalises
    quaternions on input.  Plain torch operations on the model's index maps (AoS, any device):
      1-DoF joints and the planar pitch       pass through;
      SixDoF and planar translations          R(Q) g_lin -- the step q (+) dq moves p by R(Q) dp;
      a quaternion Q = (x, y, z, s)           (2 / |Q|) Qn o (g_ang, 0) with Qn = Q / |Q|: Q' = Q exp(dth) gives dQn = Qn o (dth, 0) / 2, left
                                              multiplication by a unit quaternion is orthogonal, and the result is orthogonal to Q, so the
                                              projection of the normalisation leaves it alone;
      entries of q no joint owns              0."""
    nq, nv = int(desc.nq), int(desc.nv)
    if q.ndim != 2 or g.ndim != 2 or q.shape[1] != nq or g.shape[1] != nv or q.shape[0] != g.shape[0]:
        raise ValueError(f"expected q [B, {nq}] and g [B, {nv}], got {tuple(q.shape)} and {tuple(g.shape)}")
    m = chart_maps(desc) if maps is None else maps
    idx = lambda rows: torch.as_tensor(rows, dtype=torch.long, device=q.device)
    out = torch.zeros_like(q)
    if m["one_q"]:
        out[:, idx(m["one_q"])] = g[:, idx(m["one_v"])]
    if m["quat_q"]:
        Q, ga = q[:, idx(m["quat_q"])], g[:, idx(m["quat_v"])]  # [B, J, 4], [B, J, 3]
        norm = Q.norm(dim=-1, keepdim=True)
        Qn = Q / norm
        v, s = Qn[..., :3], Qn[..., 3:]
        out[:, idx(m["quat_q"])] = (2.0 / norm) * torch.cat([s * ga + torch.cross(v, ga, dim=-1), -(v * ga).sum(-1, keepdim=True)], dim=-1)
        if m["lin_q"]:
            x, y, z, s = Qn[:, idx(m["lin_quat"])].unbind(-1)
            R = torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - z * s), 2 * (x * z + y * s),
                             2 * (x * y + z * s), 1 - 2 * (x * x + z * z), 2 * (y * z - x * s),
                             2 * (x * z - y * s), 2 * (y * z + x * s), 1 - 2 * (x * x + y * y)], dim=-1).reshape(*x.shape, 3, 3)
            out[:, idx(m["lin_q"])] = (R @ g[:, idx(m["lin_v"])].unsqueeze(-1)).squeeze(-1)
    if m["pl_q"]:
        P, gp = q[:, idx(m["pl_q"])], g[:, idx(m["pl_v"])]  # (pitch, x, z), (w_y, v_x, v_z)
        c, s = torch.cos(P[..., 0]), torch.sin(P[..., 0])
        out[:, idx(m["pl_q"])] = torch.stack([gp[..., 0], c * gp[..., 1] + s * gp[..., 2], c * gp[..., 2] - s * gp[..., 1]], dim=-1)
    return out


def chart_cotangent(desc, q, g_raw, maps=None):
    """The velocity-space cotangent [B, nv] at q [B, nq] from a gradient g_raw [B, nq] with respect to the raw coordinates: the transpose
    of the tangent map of q (+) dq at dq = 0, the other direction of ``chart_pullback``.  Plain torch operations (AoS, any device):
      1-DoF joints and the planar pitch       pass through;
      a quaternion Q = (x, y, z, s), raw      vec(conj(Q) o g_Q) / 2 -- Q' = Q exp(dth) moves the raw Q by Q o (dth, 0) / 2, not normalised;
      SixDoF translations                     R(Q)^T g_p -- the step moves p by R(Q) dp, R of the normalised Q;
      planar translations                     (c g_x - s g_z, s g_x + c g_z), c and s of the pitch;
      DoF entries no joint owns               0."""
    nq, nv = int(desc.nq), int(desc.nv)
    if q.ndim != 2 or g_raw.ndim != 2 or q.shape[1] != nq or tuple(g_raw.shape) != tuple(q.shape):
        raise ValueError(f"expected q and g_raw [B, {nq}], got {tuple(q.shape)} and {tuple(g_raw.shape)}")
    m = chart_maps(desc) if maps is None else maps
    idx = lambda rows: torch.as_tensor(rows, dtype=torch.long, device=q.device)
    out = torch.zeros((q.shape[0], nv), dtype=q.dtype, device=q.device)
    if m["one_q"]:
        out[:, idx(m["one_v"])] = g_raw[:, idx(m["one_q"])]
    if m["quat_q"]:
        Q, gQ = q[:, idx(m["quat_q"])], g_raw[:, idx(m["quat_q"])]  # [B, J, 4] each
        v, s, gv, gs = Q[..., :3], Q[..., 3:], gQ[..., :3], gQ[..., 3:]
        out[:, idx(m["quat_v"])] = 0.5 * (s * gv - gs * v - torch.cross(v, gv, dim=-1))
        if m["lin_q"]:
            x, y, z, s = (Q / Q.norm(dim=-1, keepdim=True))[:, idx(m["lin_quat"])].unbind(-1)
            R = torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - z * s), 2 * (x * z + y * s),
                             2 * (x * y + z * s), 1 - 2 * (x * x + z * z), 2 * (y * z - x * s),
                             2 * (x * z - y * s), 2 * (y * z + x * s), 1 - 2 * (x * x + y * y)], dim=-1).reshape(*x.shape, 3, 3)
            out[:, idx(m["lin_v"])] = (R.transpose(-1, -2) @ g_raw[:, idx(m["lin_q"])].unsqueeze(-1)).squeeze(-1)
    if m["pl_q"]:
        P, gp = q[:, idx(m["pl_q"])], g_raw[:, idx(m["pl_q"])]  # (pitch, x, z) each
        c, s = torch.cos(P[..., 0]), torch.sin(P[..., 0])
        out[:, idx(m["pl_v"])] = torch.stack([gp[..., 0], c * gp[..., 1] - s * gp[..., 2], s * gp[..., 1] + c * gp[..., 2]], dim=-1)
    return out


def radial_passthrough(desc, q, q_next, g_raw_next, maps=None):
    """What the raw quaternions of q receive through their LENGTH from a gradient g_raw_next [B, nq] with respect to the raw q_next of
    ``integrate`` / ``step``, [B, nq]: the integrator forms Q' = Q exp(r) from the raw Q without normalising while everything else reads
    Q / |Q|, so scaling Q scales Q' and nothing else, which is (g_Q' . Q') Q / |Q|^2.  Zero everywhere but the quaternions; orthogonal to
    what ``chart_pullback`` returns there."""
    m = chart_maps(desc) if maps is None else maps
    out = torch.zeros_like(q)
    if m["quat_q"]:
        at = torch.as_tensor(m["quat_q"], dtype=torch.long, device=q.device)
        Q = q[:, at]
        out[:, at] = (g_raw_next[:, at] * q_next[:, at]).sum(-1, keepdim=True) * Q / (Q * Q).sum(-1, keepdim=True)
    return out


def _wanted(ctx, first, like):
    """One new output tensor per input of ctx.needs_input_grad[first : first + 3] that wants a gradient, None for the others."""
    return tuple(torch.empty_like(like) if need else None for need in ctx.needs_input_grad[first:first + 3])


class _Rnea(torch.autograd.Function):
    @staticmethod
    def forward(ctx, model, q, qd, qdd, gravity, f_ext):
        ctx.model, ctx.gravity, ctx.f_ext = model, gravity, f_ext
        ctx.save_for_backward(q, qd, qdd)
        return model.rnea(q, qd, qdd, gravity, f_ext)

    @staticmethod
    @once_differentiable
    def backward(ctx, u):
        q, qd, qdd = ctx.saved_tensors
        gq, gqd, gqdd = ctx.model.rnea_vjp(q, qd, qdd, u.contiguous(), ctx.gravity, ctx.f_ext, out=_wanted(ctx, 1, qd))
        return None, (None if gq is None else ctx.model.chart_pullback(q, gq)), gqd, gqdd, None, None


class _Aba(torch.autograd.Function):
    @staticmethod
    def forward(ctx, model, q, qd, tau, gravity, f_ext):
        ctx.model, ctx.gravity, ctx.f_ext = model, gravity, f_ext
        ctx.save_for_backward(q, qd, tau)
        return model.aba(q, qd, tau, gravity, f_ext)

    @staticmethod
    @once_differentiable
    def backward(ctx, w):
        q, qd, tau = ctx.saved_tensors
        _, gq, gqd, gtau = ctx.model.aba_vjp(q, qd, tau, w.contiguous(), ctx.gravity, ctx.f_ext, out=(None,) + _wanted(ctx, 1, qd))
        return None, (None if gq is None else ctx.model.chart_pullback(q, gq)), gqd, gtau, None, None


class _BodyPoses(torch.autograd.Function):
    @staticmethod
    def forward(ctx, model, q, targets, poses):
        ctx.model, ctx.targets, ctx.poses = model, targets, poses
        ctx.save_for_backward(q)
        return model.body_poses(q, targets, poses)

    @staticmethod
    @once_differentiable
    def backward(ctx, g_pose):
        q, = ctx.saved_tensors
        gq = ctx.model.body_poses_vjp(q, g_pose.contiguous(), ctx.targets, ctx.poses)
        return None, ctx.model.chart_pullback(q, gq), None, None


class _RneaParameters(torch.autograd.Function):
    @staticmethod
    def forward(ctx, model, q, qd, qdd, pi, gravity, f_ext):
        ctx.model, ctx.gravity = model, gravity
        ctx.save_for_backward(q, qd, qdd, pi)
        return model.rnea_parameters(q, qd, qdd, pi, gravity, f_ext)

    @staticmethod
    @once_differentiable
    def backward(ctx, u):
        q, qd, qdd, pi = ctx.saved_tensors
        return None, None, None, None, ctx.model.rnea_parameters_vjp(q, qd, qdd, pi, u.contiguous(), ctx.gravity), None, None


class _AbaParameters(torch.autograd.Function):
    @staticmethod
    def forward(ctx, model, q, qd, tau, pi, gravity, f_ext):
        ctx.model, ctx.gravity, ctx.f_ext = model, gravity, f_ext
        ctx.save_for_backward(q, qd, tau, pi)
        return model.aba_parameters(q, qd, tau, pi, gravity, f_ext)

    @staticmethod
    @once_differentiable
    def backward(ctx, w):
        q, qd, tau, pi = ctx.saved_tensors
        gpi = ctx.model.aba_parameters_vjp(q, qd, tau, pi, w.contiguous(), ctx.gravity, ctx.f_ext, out=(None, None, torch.empty_like(pi)))[2]
        return None, None, None, None, gpi, None, None


def _wanted_with_pi(ctx, first, like, pi):
    """``_wanted`` for three state inputs, and one more tensor like pi where pi wants a gradient."""
    return _wanted(ctx, first, like) + (torch.empty_like(pi) if ctx.needs_input_grad[first + 3] else None,)


class _RneaParametersState(torch.autograd.Function):
    @staticmethod
    def forward(ctx, model, q, qd, qdd, pi, gravity, f_ext):
        ctx.model, ctx.gravity, ctx.f_ext = model, gravity, f_ext
        ctx.save_for_backward(q, qd, qdd, pi)
        return model.rnea_parameters(q, qd, qdd, pi, gravity, f_ext)

    @staticmethod
    @once_differentiable
    def backward(ctx, u):
        q, qd, qdd, pi = ctx.saved_tensors
        gq, gqd, gqdd, gpi = ctx.model.rnea_parameters_state_vjp(q, qd, qdd, pi, u.contiguous(), ctx.gravity, ctx.f_ext,
                                                                 out=_wanted_with_pi(ctx, 1, qd, pi))
        return None, (None if gq is None else ctx.model.chart_pullback(q, gq)), gqd, gqdd, gpi, None, None


class _AbaParametersState(torch.autograd.Function):
    @staticmethod
    def forward(ctx, model, q, qd, tau, pi, gravity, f_ext):
        ctx.model, ctx.gravity, ctx.f_ext = model, gravity, f_ext
        ctx.save_for_backward(q, qd, tau, pi)
        return model.aba_parameters(q, qd, tau, pi, gravity, f_ext)

    @staticmethod
    @once_differentiable
    def backward(ctx, w):
        q, qd, tau, pi = ctx.saved_tensors
        _, gq, gqd, gtau, gpi = ctx.model.aba_parameters_state_vjp(q, qd, tau, pi, w.contiguous(), ctx.gravity, ctx.f_ext,
                                                                   out=(None,) + _wanted_with_pi(ctx, 1, qd, pi))
        return None, (None if gq is None else ctx.model.chart_pullback(q, gq)), gqd, gtau, gpi, None, None


def _raw_gradient(model, q, q_next, gq, g_raw_next):
    """chart_pullback at q plus the quaternions' radial pass-through: the gradient of the raw map q -> (q_next, qd_next)."""
    if gq is None:
        return None
    return model.chart_pullback(q, gq) + radial_passthrough(model.desc, q, q_next, g_raw_next, getattr(model, "_chart_index", None))


class _Integrate(torch.autograd.Function):
    @staticmethod
    def forward(ctx, model, dt, q, qd, qdd):
        q_next, qd_next = model.integrate(dt, q, qd, qdd)[:2]
        ctx.model, ctx.dt = model, dt
        ctx.save_for_backward(q, qd, qdd, q_next)
        return q_next, qd_next

    @staticmethod
    @once_differentiable
    def backward(ctx, g_q_next, g_qd_next):
        q, qd, qdd, q_next = ctx.saved_tensors
        gth = ctx.model.chart_cotangent(q_next, g_q_next)
        gq, gqd, gqdd = ctx.model.integrate_vjp(ctx.dt, qd, qdd, gth, g_qd_next.contiguous(), out=_wanted(ctx, 2, qd))
        return None, None, _raw_gradient(ctx.model, q, q_next, gq, g_q_next), gqd, gqdd


class _Step(torch.autograd.Function):
    @staticmethod
    def forward(ctx, model, dt, q, qd, tau, gravity, f_ext):
        if q.dtype == torch.float64:
            q_next, qd_next, _ = model.step(dt, q, qd, tau, gravity, f_ext)
        else:  # (the fused entry point is fp64 only)
            q_next, qd_next = model.integrate(dt, q, qd, model.aba(q, qd, tau, gravity, f_ext))[:2]
        ctx.model, ctx.dt, ctx.gravity, ctx.f_ext = model, dt, gravity, f_ext
        ctx.save_for_backward(q, qd, tau, q_next)
        return q_next, qd_next

    @staticmethod
    @once_differentiable
    def backward(ctx, g_q_next, g_qd_next):
        q, qd, tau, q_next = ctx.saved_tensors
        gth = ctx.model.chart_cotangent(q_next, g_q_next)
        _, gq, gqd, gtau = ctx.model.step_vjp(ctx.dt, q, qd, tau, gth, g_qd_next.contiguous(), ctx.gravity, ctx.f_ext,
                                              out=(None,) + _wanted(ctx, 2, qd))
        return None, None, _raw_gradient(ctx.model, q, q_next, gq, g_q_next), gqd, gtau, None, None


def integrate(model, dt, q, qd, qdd):
    """(q_next, qd_next) = ``model.integrate(dt, q, qd, qdd)``, differentiable with respect to q (raw coordinates), qd and qdd."""
    return _Integrate.apply(model, dt, q, qd, qdd)


def step(model, dt, q, qd, tau, gravity=(0.0, 0.0, -9.81), f_ext=None):
    """(q_next, qd_next) of one simulation step, ``model.aba`` then ``model.integrate`` with step ``dt`` (fp64: ``model.step``),
    differentiable with respect to q (raw coordinates), qd and tau: the backward pass is ONE ``model.step_vjp``."""
    return _Step.apply(model, dt, q, qd, tau, gravity, f_ext)


def rnea(model, q, qd, qdd, gravity=(0.0, 0.0, -9.81), f_ext=None):
    """tau = ``model.rnea(q, qd, qdd, gravity, f_ext)``, differentiable with respect to q (raw coordinates), qd and qdd."""
    return _Rnea.apply(model, q, qd, qdd, gravity, f_ext)


def aba(model, q, qd, tau, gravity=(0.0, 0.0, -9.81), f_ext=None):
    """qdd = ``model.aba(q, qd, tau, gravity, f_ext)``, differentiable with respect to q (raw coordinates), qd and tau."""
    return _Aba.apply(model, q, qd, tau, gravity, f_ext)


def body_poses(model, q, targets=None, poses=None):
    """[B, K, 12] = ``model.body_poses(q, targets, poses)``, differentiable with respect to q (raw coordinates): the backward pass is ONE
    ``model.body_poses_vjp`` (no Jacobian is formed) plus ``chart_pullback``.  Every task-space loss lives on this output."""
    return _BodyPoses.apply(model, q, targets, poses)


def _state_is_constant(call, **state):
    for name, t in state.items():
        if t.requires_grad:
            raise NotImplementedError(f"{call} is differentiable with respect to pi only: {name} requires grad (the state gradients at "
                                      "per-configuration parameters are not provided)")


def rnea_parameters(model, q, qd, qdd, pi, gravity=(0.0, 0.0, -9.81), f_ext=None):
    """tau = ``model.rnea_parameters(q, qd, qdd, pi, gravity, f_ext)``, differentiable with respect to pi ([B, n_joints, 10] or
    [B, 10 n_joints]) and to nothing else: a q, qd or qdd that requires grad raises NotImplementedError.  A pi made by
    ``shared.expand(B, n, 10).contiguous()`` hands the sum over the batch to ``shared`` through torch's own expand backward."""
    _state_is_constant("rnea_parameters", q=q, qd=qd, qdd=qdd)
    return _RneaParameters.apply(model, q, qd, qdd, pi, gravity, f_ext)


def aba_parameters(model, q, qd, tau, pi, gravity=(0.0, 0.0, -9.81), f_ext=None):
    """qdd = ``model.aba_parameters(q, qd, tau, pi, gravity, f_ext)``, differentiable with respect to pi as ``rnea_parameters`` is: a q,
    qd or tau that requires grad raises NotImplementedError."""
    _state_is_constant("aba_parameters", q=q, qd=qd, tau=tau)
    return _AbaParameters.apply(model, q, qd, tau, pi, gravity, f_ext)


def rnea_parameters_state(model, q, qd, qdd, pi, gravity=(0.0, 0.0, -9.81), f_ext=None):
    """tau = ``model.rnea_parameters(q, qd, qdd, pi, gravity, f_ext)``, differentiable with respect to q (raw coordinates), qd, qdd AND pi
    in one backward call: ONE ``model.rnea_parameters_state_vjp`` that forms only the gradients ``needs_input_grad`` asks for."""
    return _RneaParametersState.apply(model, q, qd, qdd, pi, gravity, f_ext)


def aba_parameters_state(model, q, qd, tau, pi, gravity=(0.0, 0.0, -9.81), f_ext=None):
    """qdd = ``model.aba_parameters(q, qd, tau, pi, gravity, f_ext)``, differentiable with respect to q (raw coordinates), qd, tau AND pi
    in one backward call: ONE ``model.aba_parameters_state_vjp``."""
    return _AbaParametersState.apply(model, q, qd, tau, pi, gravity, f_ext)


def step_parameters(model, dt, q, qd, tau, pi, gravity=(0.0, 0.0, -9.81), f_ext=None):
    """(q_next, qd_next) of one simulation step of B different robots: ``aba_parameters_state`` then ``integrate`` with step ``dt``,
    differentiable with respect to q (raw coordinates), qd, tau and pi, so that rollouts chain across quaternions."""
    return integrate(model, dt, q, qd, aba_parameters_state(model, q, qd, tau, pi, gravity, f_ext))
