"""torch.autograd through the batched dynamics: ``rnea`` and ``aba`` as differentiable functions of (q, qd, qdd | tau), and the pullback
from velocity-space gradients to the raw coordinates.

The forward passes are ``HipModel.rnea`` / ``HipModel.aba`` unchanged; a backward pass is ONE call of ``HipModel.rnea_vjp`` /
``HipModel.aba_vjp`` (the O(n) adjoint sweep of mh_rnea_vjp_kernels.h: no nv x nv matrix is formed) plus ``chart_pullback`` for q.
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


def rnea(model, q, qd, qdd, gravity=(0.0, 0.0, -9.81), f_ext=None):
    """tau = ``model.rnea(q, qd, qdd, gravity, f_ext)``, differentiable with respect to q (raw coordinates), qd and qdd."""
    return _Rnea.apply(model, q, qd, qdd, gravity, f_ext)


def aba(model, q, qd, tau, gravity=(0.0, 0.0, -9.81), f_ext=None):
    """qdd = ``model.aba(q, qd, tau, gravity, f_ext)``, differentiable with respect to q (raw coordinates), qd and tau."""
    return _Aba.apply(model, q, qd, tau, gravity, f_ext)
