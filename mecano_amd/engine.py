"""Thin object wrapper over the C-ABI: a device-resident model plus batched rnea / aba / crba calls.

Device inputs are torch tensors on a HIP device (torch is used for device memory and streams only); numpy
inputs go through the host-pointer entry points.  Every compute goes through libmecano_hip.so: nothing here
computes dynamics in Python.
"""
from __future__ import annotations

import ctypes
from typing import Optional, Sequence

import numpy as np

from . import _lib
from .multibody import ModelDesc


def _np(a, dtype):
    return np.ascontiguousarray(a, dtype=dtype)


class HipModel:
    """mh_model_t: the flattened MultiBodySystemReadOnly, uploaded once (replaces the calculators' constructors)."""

    def __init__(self, desc: ModelDesc):
        lib = _lib.load()
        self.desc = desc
        self._arrays = dict(
            parent=_np(desc.parent, np.int32), joint_type=_np(desc.joint_type, np.int32), axis=_np(desc.axis, np.float64),
            X_before=_np(desc.X_before, np.float64), X_com=_np(desc.X_com, np.float64), inertia_J=_np(desc.inertia_J, np.float64),
            inertia_mass=_np(desc.inertia_mass, np.float64), inertia_com=_np(desc.inertia_com, np.float64),
            dof_indices=_np(desc.dof_indices, np.int32), cfg_indices=_np(desc.cfg_indices, np.int32))
        d = _lib.MhModelDesc()
        d.n_joints, d.nq, d.nv = int(desc.n_joints), int(desc.nq), int(desc.nv)
        for k, a in self._arrays.items():
            setattr(d, k, a.ctypes.data_as(ctypes.c_void_p))
        handle = ctypes.c_void_p()
        _lib.check(lib.mh_model_create(ctypes.byref(d), ctypes.byref(handle)))
        self._h = handle
        self._ctx = None       # mh_context_t of a view made by context(); None: the model's default context
        self._parent = None    # the HipModel a context view was made from (kept alive: it owns the handle)
        self.nq, self.nv, self.n_joints = desc.nq, desc.nv, desc.n_joints

    def context(self) -> "HipModel":
        """A view of this model with a context of its own (mh_context_create): the handle is read-only and shared, everything compute
        calls write besides their outputs -- workspace, scratch, staging buffers, hand-off flags, error word -- belongs to the view.  One
        view per host thread / per stream; views and the model itself may then be used at the same time (include/mecano_hip.h, Threading)."""
        import copy
        ctx = ctypes.c_void_p()
        _lib.check(_lib.load().mh_context_create(self._h, ctypes.byref(ctx)))
        view = copy.copy(self)
        view._ctx, view._parent = ctx, (self._parent or self)
        return view

    def check(self, stream=None):
        """mh_model_check: synchronises `stream` and raises what this model's (view's) asynchronous calls left behind on the device."""
        _lib.check(_lib.load().mh_model_check(self._h, self._ctx, stream))

    def close(self):
        if getattr(self, "_ctx", None):
            _lib.load().mh_context_destroy(self._ctx)
            self._ctx = None
            self._h = None  # (a view: the handle belongs to the model it was made from)
            return
        if getattr(self, "_parent", None) is not None:
            return
        if getattr(self, "_h", None):
            _lib.load().mh_model_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def kernel_variant(self) -> str:
        return _lib.load().mh_model_kernel_variant(self._h).decode()

    @property
    def warnings(self) -> int:
        """MH_WARN_* bits (include/mecano_hip.h): the two model classes in which the engine consciously departs from Mecano."""
        return int(_lib.load().mh_model_warnings(self._h))

    @property
    def warning_text(self) -> str:
        return _lib.load().mh_model_warning_text(self._h).decode()

    def reserve(self, max_batch: int):
        if self._ctx:
            _lib.check(_lib.load().mh_context_reserve(self._ctx, int(max_batch)))
        else:
            _lib.check(_lib.load().mh_reserve(self._h, int(max_batch)))

    # ------------------------------------------------------------------ helpers
    def _options(self, layout, consider_coriolis=True, consider_accelerations=True, stream=None, root_acceleration=None):
        o = _lib.MhOptions()
        o.context = self._ctx
        o.consider_coriolis = int(bool(consider_coriolis))
        o.consider_accelerations = int(bool(consider_accelerations))
        o.layout = int(layout)
        o.use_root_acceleration = 0 if root_acceleration is None else 1
        o.stream = stream
        for k in range(6):
            o.root_acceleration[k] = 0.0 if root_acceleration is None else float(root_acceleration[k])
        return o

    @staticmethod
    def _root(gravity):
        """The `gravity` argument of the compute calls: a 3-vector g (the root body accelerates with (0, -g): setGravity,
        InverseDynamicsCalculator.java:318-348) or a 6-vector, the root's spatial acceleration itself, angular then linear
        (setRootAcceleration, InverseDynamicsCalculator.java:413-427; mh_options.root_acceleration).  Returns (g[3] for the C call, the 6 or None)."""
        a = [float(v) for v in np.asarray(gravity, dtype=np.float64).reshape(-1)]
        if len(a) == 6:
            return (ctypes.c_double * 3)(0.0, 0.0, 0.0), a
        if len(a) != 3:
            raise _lib.MecanoHipError(2, f"gravity must have 3 entries (or 6: a root acceleration), got {len(a)}")
        return (ctypes.c_double * 3)(*a), None

    @staticmethod
    def _is_torch(x):
        return type(x).__module__.startswith("torch")

    def _batch(self, x, n, layout):
        if x.ndim != 2:
            raise _lib.MecanoHipError(2, f"expected a 2-D state matrix, got shape {tuple(x.shape)}")
        rows, B = (x.shape[1], x.shape[0]) if layout == _lib.LAYOUT_AOS else (x.shape[0], x.shape[1])
        if rows != n:
            # the MatrixDimensionException of ForwardDynamicsCalculator.java:522-533
            raise _lib.MecanoHipError(2, f"state matrix has {rows} rows per configuration, the system needs {n}")
        return B

    def _check_f_ext(self, f_ext, B, layout):
        """External wrenches are [B, n_joints, 6] (SoA: [n_joints * 6, B]): a wrong shape would be an out-of-bounds device read."""
        if f_ext is None:
            return
        want = (B, self.n_joints, 6) if layout == _lib.LAYOUT_AOS else (self.n_joints * 6, B)
        if tuple(f_ext.shape) != want and not (layout == _lib.LAYOUT_AOS and tuple(f_ext.shape) == (B, self.n_joints * 6)):
            raise _lib.MecanoHipError(2, f"external wrenches have shape {tuple(f_ext.shape)}, expected {want}")

    def _device_tensor(self, t, dt):
        if not self._is_torch(t) or not t.is_cuda or t.dtype != dt or not t.is_contiguous():
            raise ValueError("device tensors must be contiguous, on the HIP device and of one dtype")

    def _output(self, out, shape, dt, device, name=""):
        """``out`` checked as an output of ``shape``, or a new tensor where it is None."""
        import torch
        if out is None:
            return torch.empty(shape, dtype=dt, device=device)
        self._device_tensor(out, dt)
        if tuple(out.shape) != shape:
            raise _lib.MecanoHipError(2, f"{name and name + ' '}output has shape {tuple(out.shape)}, expected {shape}")
        return out

    def _outputs(self, out, shapes, names, dt, device):
        """The outputs of a call that returns several: ``out`` a tuple with None for what is not wanted, or None for all of them."""
        if out is None:
            return tuple(self._output(None, s, dt, device) for s in shapes)
        if len(out) != len(names):
            raise _lib.MecanoHipError(2, f"out must hold {len(names)} entries ({', '.join(names)})")
        return tuple(t if t is None else self._output(t, s, dt, device, name) for t, s, name in zip(out, shapes, names))

    def _run(self, kind, q, qd, x3, gravity, f_ext, layout, consider_coriolis, consider_accelerations):
        lib = _lib.load()
        g, ra = self._root(gravity)
        if self._is_torch(q):
            import torch
            dt = q.dtype
            if dt not in (torch.float64, torch.float32):
                raise TypeError("state tensors must be float64 or float32")
            tensors = [q] if kind == "crba" else [q, qd, x3]
            if f_ext is not None:
                tensors.append(f_ext)
            for t in tensors:
                if not t.is_cuda or t.dtype != dt or not t.is_contiguous():
                    raise ValueError("device tensors must be contiguous, on the HIP device and of one dtype")
            B = self._batch(q, self.nq, layout)
            if kind != "crba":
                if self._batch(qd, self.nv, layout) != B or self._batch(x3, self.nv, layout) != B:
                    raise _lib.MecanoHipError(2, "batch sizes of the state matrices differ")
            self._check_f_ext(f_ext, B, layout)
            stream = torch.cuda.current_stream(q.device).cuda_stream
            opts = self._options(layout, consider_coriolis, consider_accelerations, stream, root_acceleration=ra)
            sfx = "f64" if dt == torch.float64 else "f32"
            if kind == "crba":
                shape = (B, self.nv, self.nv) if layout == _lib.LAYOUT_AOS else (self.nv * self.nv, B)
                out = torch.empty(shape, dtype=dt, device=q.device)
                _lib.check(getattr(lib, f"mh_crba_{sfx}")(self._h, B, q.data_ptr(), ctypes.byref(opts), out.data_ptr()))
            else:
                out = torch.empty_like(qd)
                fp = f_ext.data_ptr() if f_ext is not None else None
                _lib.check(getattr(lib, f"mh_{kind}_{sfx}")(self._h, B, q.data_ptr(), qd.data_ptr(), x3.data_ptr(), g, fp, ctypes.byref(opts),
                                                            out.data_ptr()))
            return out
        # numpy: host-pointer entry points (fp64; float32 arrays go to the fp32 ones)
        ndt = np.float32 if getattr(q, "dtype", None) == np.float32 else np.float64
        sfx = "f32" if ndt == np.float32 else "f64"
        q = _np(q, ndt)
        B = self._batch(q, self.nq, layout)
        opts = self._options(layout, consider_coriolis, consider_accelerations, None, root_acceleration=ra)
        if kind == "crba":
            out = np.empty((B, self.nv, self.nv) if layout == _lib.LAYOUT_AOS else (self.nv * self.nv, B), dtype=ndt)
            _lib.check(getattr(lib, f"mh_crba_{sfx}_host")(self._h, B, q.ctypes.data, ctypes.byref(opts), out.ctypes.data))
            return out
        qd, x3 = _np(qd, ndt), _np(x3, ndt)
        if self._batch(qd, self.nv, layout) != B or self._batch(x3, self.nv, layout) != B:
            raise _lib.MecanoHipError(2, "batch sizes of the state matrices differ")
        f = None if f_ext is None else _np(f_ext, ndt)
        self._check_f_ext(f, B, layout)
        out = np.empty_like(qd)
        _lib.check(getattr(lib, f"mh_{kind}_{sfx}_host")(self._h, B, q.ctypes.data, qd.ctypes.data, x3.ctypes.data, g,
                                                        None if f is None else f.ctypes.data, ctypes.byref(opts), out.ctypes.data))
        return out

    # ------------------------------------------------------------------ the three hot-path calls
    def rnea(self, q, qd, qdd, gravity=(0.0, 0.0, -9.81), f_ext=None, layout=_lib.LAYOUT_AOS, consider_coriolis=True,
             consider_accelerations=True):
        return self._run("rnea", q, qd, qdd, gravity, f_ext, layout, consider_coriolis, consider_accelerations)

    def aba(self, q, qd, tau, gravity=(0.0, 0.0, -9.81), f_ext=None, layout=_lib.LAYOUT_AOS):
        return self._run("aba", q, qd, tau, gravity, f_ext, layout, True, True)

    def set_joint_source_modes(self, modes: Optional[Sequence[int]]):
        """One mode per joint of the description (0 = effort source, 1 = acceleration source); None resets all of them
        (ForwardDynamicsCalculator.java:400-444)."""
        lib = _lib.load()
        if modes is None:
            _lib.check(lib.mh_model_set_joint_source_modes(self._h, None))
            return
        m = _np(modes, np.int32)
        if m.shape != (self.n_joints,):
            raise _lib.MecanoHipError(2, f"expected {self.n_joints} joint source modes, got {m.shape}")
        _lib.check(lib.mh_model_set_joint_source_modes(self._h, m.ctypes.data))

    @property
    def n_acceleration_sources(self) -> int:
        return int(_lib.load().mh_model_n_acceleration_sources(self._h))

    def aba_locked(self, q, qd, tau, qdd_in, gravity=(0.0, 0.0, -9.81), f_ext=None, layout=_lib.LAYOUT_AOS):
        """Forward dynamics with acceleration-source joints: returns (qdd, tau) of all DoFs (fp64).  numpy inputs are moved to
        the current HIP device and the results back.  (The C call takes qdd_out == qdd_in and tau_out == tau, no other overlap.)"""
        import torch
        lib = _lib.load()
        host = not self._is_torch(q)
        if host:
            dev = torch.device("cuda", torch.cuda.current_device())
            q, qd, tau, qdd_in = [torch.from_numpy(_np(x, np.float64)).to(dev) for x in (q, qd, tau, qdd_in)]
            f_ext = None if f_ext is None else torch.from_numpy(_np(f_ext, np.float64)).to(dev)
        dt = q.dtype
        if dt not in (torch.float64, torch.float32):
            raise TypeError("state tensors must be float64 or float32")
        for t in (q, qd, tau, qdd_in) + ((f_ext,) if f_ext is not None else ()):
            if not t.is_cuda or t.dtype != dt or not t.is_contiguous():
                raise ValueError("aba_locked needs contiguous tensors of one dtype on the HIP device")
        B = self._batch(q, self.nq, layout)
        if any(self._batch(x, self.nv, layout) != B for x in (qd, tau, qdd_in)):
            raise _lib.MecanoHipError(2, "batch sizes of the state matrices differ")
        self._check_f_ext(f_ext, B, layout)
        g, ra = self._root(gravity)
        opts = self._options(layout, True, True, torch.cuda.current_stream(q.device).cuda_stream, root_acceleration=ra)
        qdd_out, tau_out = torch.empty_like(qd), torch.empty_like(qd)
        fn = lib.mh_aba_locked_f64 if dt == torch.float64 else lib.mh_aba_locked_f32
        _lib.check(fn(self._h, B, q.data_ptr(), qd.data_ptr(), tau.data_ptr(), qdd_in.data_ptr(), g,
                                         f_ext.data_ptr() if f_ext is not None else None, ctypes.byref(opts), qdd_out.data_ptr(),
                                         tau_out.data_ptr()))
        if host:
            return qdd_out.cpu().numpy(), tau_out.cpu().numpy()
        return qdd_out, tau_out

    def _bodies(self, kind, q, qd, x3, gravity, f_ext, layout, consider_coriolis=True, consider_accelerations=True):
        import torch
        lib = _lib.load()
        dt = q.dtype
        if dt not in (torch.float64, torch.float32) or (dt == torch.float32 and kind not in ("rnea", "aba")):
            raise TypeError("per-body outputs take float64 or float32 tensors, joint wrenches float64")
        for t in (q, qd, x3) + ((f_ext,) if f_ext is not None else ()):
            if not t.is_cuda or t.dtype != dt or not t.is_contiguous():
                raise ValueError("per-body outputs need contiguous tensors of one dtype on the HIP device")
        B = self._batch(q, self.nq, layout)
        if self._batch(qd, self.nv, layout) != B or self._batch(x3, self.nv, layout) != B:
            raise _lib.MecanoHipError(2, "batch sizes of the state matrices differ")
        self._check_f_ext(f_ext, B, layout)
        g, ra = self._root(gravity)
        opts = self._options(layout, consider_coriolis, consider_accelerations, torch.cuda.current_stream(q.device).cuda_stream, root_acceleration=ra)
        out = torch.empty_like(qd)
        shape = (B, self.n_joints, 6) if layout == _lib.LAYOUT_AOS else (self.n_joints * 6, B)
        if kind in ("rnea_wrenches", "aba_wrenches"):
            w = torch.empty(shape, dtype=dt, device=q.device)
            fn = lib.mh_rnea_joint_wrenches_f64 if kind == "rnea_wrenches" else lib.mh_aba_joint_wrenches_f64
            _lib.check(fn(self._h, B, q.data_ptr(), qd.data_ptr(), x3.data_ptr(), g, f_ext.data_ptr() if f_ext is not None else None,
                          ctypes.byref(opts), out.data_ptr(), w.data_ptr()))
            return out, w
        acc, tw = torch.empty(shape, dtype=dt, device=q.device), torch.empty(shape, dtype=dt, device=q.device)
        sfx = "f64" if dt == torch.float64 else "f32"
        fn = getattr(lib, f"mh_rnea_bodies_{sfx}" if kind == "rnea" else f"mh_aba_bodies_{sfx}")
        _lib.check(fn(self._h, B, q.data_ptr(), qd.data_ptr(), x3.data_ptr(), g, f_ext.data_ptr() if f_ext is not None else None, ctypes.byref(opts),
                      out.data_ptr(), acc.data_ptr(), tw.data_ptr()))
        return out, acc, tw

    def rnea_bodies(self, q, qd, qdd, gravity=(0.0, 0.0, -9.81), f_ext=None, layout=_lib.LAYOUT_AOS, consider_coriolis=True,
                    consider_accelerations=True):
        """RNEA plus per-body outputs: (tau, body_acc, body_twist), the latter [B, n_joints, 6] in the body-fixed frames."""
        return self._bodies("rnea", q, qd, qdd, gravity, f_ext, layout, consider_coriolis, consider_accelerations)

    def aba_bodies(self, q, qd, tau, gravity=(0.0, 0.0, -9.81), f_ext=None, layout=_lib.LAYOUT_AOS):
        """ABA plus per-body outputs: (qdd, body_acc, body_twist)."""
        return self._bodies("aba", q, qd, tau, gravity, f_ext, layout)

    def rnea_joint_wrenches(self, q, qd, qdd, gravity=(0.0, 0.0, -9.81), f_ext=None, layout=_lib.LAYOUT_AOS, consider_coriolis=True,
                            consider_accelerations=True):
        """RNEA plus InverseDynamicsCalculator.getComputedJointWrench of every joint: (tau, joint_wrench [B, n_joints, 6]), the
        wrenches (moment, force) in the frames after the joints."""
        return self._bodies("rnea_wrenches", q, qd, qdd, gravity, f_ext, layout, consider_coriolis, consider_accelerations)

    def aba_joint_wrenches(self, q, qd, tau, gravity=(0.0, 0.0, -9.81), f_ext=None, layout=_lib.LAYOUT_AOS):
        """ABA plus ForwardDynamicsCalculator.getJointWrench of every joint: (qdd, joint_wrench)."""
        return self._bodies("aba_wrenches", q, qd, tau, gravity, f_ext, layout)

    def relative_acceleration(self, q, body_acc, body_twist, base_joints, body_joints, gravity=(0.0, 0.0, -9.81), layout=_lib.LAYOUT_AOS,
                              consider_velocities=True):
        """RigidBodyAccelerationProvider.getRelativeAcceleration for pairs of bodies (indices of listed joints, -1 = the root body) from
        the per-body outputs of rnea_bodies / aba_bodies on the same configurations: [B, n_pairs, 6] in the body's body-fixed frame."""
        import torch
        lib = _lib.load()
        tensors = (q, body_acc) + ((body_twist,) if body_twist is not None else ())
        for t in tensors:
            if not t.is_cuda or t.dtype != torch.float64 or not t.is_contiguous():
                raise ValueError("relative_acceleration needs contiguous float64 tensors on the HIP device")
        B = self._batch(q, self.nq, layout)
        for t in tensors[1:]:
            self._check_f_ext(t, B, layout)
        base, body = _np(base_joints, np.int32).reshape(-1), _np(body_joints, np.int32).reshape(-1)
        if base.shape != body.shape:
            raise _lib.MecanoHipError(2, "base and body index lists differ in length")
        n_pairs = int(base.shape[0])
        g, ra = self._root(gravity)
        opts = self._options(layout, consider_velocities, True, torch.cuda.current_stream(q.device).cuda_stream, root_acceleration=ra)
        out = torch.empty((B, n_pairs, 6) if layout == _lib.LAYOUT_AOS else (n_pairs * 6, B), dtype=torch.float64, device=q.device)
        _lib.check(lib.mh_relative_acceleration_f64(self._h, B, q.data_ptr(), body_acc.data_ptr(),
                                                    body_twist.data_ptr() if body_twist is not None else None, g, n_pairs, base.ctypes.data,
                                                    body.ctypes.data, ctypes.byref(opts), out.data_ptr()))
        return out

    def integrate(self, dt, q, qd, qdd, layout=_lib.LAYOUT_AOS, out=None, return_acceleration=False):
        """One step of MultiBodySystemStateIntegrator.doubleIntegrateFromAcceleration on device tensors (fp64 / fp32).  ``out`` =
        (q_out, qd_out[, qdd_out]) may name the inputs themselves for an in-place step (each output its own input; any other overlap is
        refused); by default new tensors are returned."""
        import torch
        lib = _lib.load()
        dt_ = q.dtype
        if dt_ not in (torch.float64, torch.float32):
            raise TypeError("state tensors must be float64 or float32")
        for t in (q, qd, qdd):
            if not t.is_cuda or t.dtype != dt_ or not t.is_contiguous():
                raise ValueError("integrate needs contiguous tensors of one dtype on the HIP device")
        B = self._batch(q, self.nq, layout)
        if self._batch(qd, self.nv, layout) != B or self._batch(qdd, self.nv, layout) != B:
            raise _lib.MecanoHipError(2, "batch sizes of the state matrices differ")
        if out is None:
            # entries no joint owns are passed through unchanged
            out = (q.clone(), qd.clone()) + ((qdd.clone(),) if return_acceleration else ())
        q_out, qd_out = out[0], out[1]
        qdd_out = out[2] if len(out) > 2 else None
        opts = self._options(layout, True, True, torch.cuda.current_stream(q.device).cuda_stream)
        fn = lib.mh_integrate_f64 if dt_ == torch.float64 else lib.mh_integrate_f32
        _lib.check(fn(self._h, B, float(dt), q.data_ptr(), qd.data_ptr(), qdd.data_ptr(), ctypes.byref(opts), q_out.data_ptr(), qd_out.data_ptr(),
                      qdd_out.data_ptr() if qdd_out is not None else None))
        return out

    def step(self, dt, q, qd, tau, gravity=(0.0, 0.0, -9.81), f_ext=None, inplace=False):
        """One simulation step (forward dynamics + state integration, mh_aba_integrate_f64): returns (q_next, qd_next, qdd).  AoS fp64
        device tensors; ``inplace=True`` overwrites q and qd (q_next == q, qd_next == qd; qdd is always a tensor of its own)."""
        import torch
        lib = _lib.load()
        for t in (q, qd, tau) + ((f_ext,) if f_ext is not None else ()):
            if not t.is_cuda or t.dtype != torch.float64 or not t.is_contiguous():
                raise ValueError("step needs contiguous float64 tensors on the HIP device")
        B = self._batch(q, self.nq, _lib.LAYOUT_AOS)
        if self._batch(qd, self.nv, _lib.LAYOUT_AOS) != B or self._batch(tau, self.nv, _lib.LAYOUT_AOS) != B:
            raise _lib.MecanoHipError(2, "batch sizes of the state matrices differ")
        self._check_f_ext(f_ext, B, _lib.LAYOUT_AOS)
        g, ra = self._root(gravity)
        opts = self._options(_lib.LAYOUT_AOS, True, True, torch.cuda.current_stream(q.device).cuda_stream, root_acceleration=ra)
        qn, vn = (q, qd) if inplace else (q.clone(), qd.clone())
        qdd = torch.empty_like(qd)
        _lib.check(lib.mh_aba_integrate_f64(self._h, B, float(dt), q.data_ptr(), qd.data_ptr(), tau.data_ptr(), g,
                                            f_ext.data_ptr() if f_ext is not None else None, ctypes.byref(opts), qdd.data_ptr(), qn.data_ptr(),
                                            vn.data_ptr()))
        return qn, vn, qdd

    def rnea_aba(self, q, qd, qdd, tau, gravity=(0.0, 0.0, -9.81), f_ext=None, out=None, layout=_lib.LAYOUT_AOS):
        """tau_out = RNEA(q, qd, qdd) and qdd_out = ABA(q, qd, tau) in one call.  Device tensors: mh_rnea_aba_f64 / mh_rnea_aba_f32 (``layout``:
        AoS [B, n] or SoA [n, B]); numpy arrays (fp64, AoS): the pipelined host-pointer entry point mh_rnea_aba_f64_host (``out`` = (tau_out,
        qdd_out) arrays to write into, e.g. pinned ones)."""
        lib = _lib.load()
        if not self._is_torch(q):
            q, qd, qdd, tau = (_np(x, np.float64) for x in (q, qd, qdd, tau))
            B = self._batch(q, self.nq, _lib.LAYOUT_AOS)
            if any(self._batch(x, self.nv, _lib.LAYOUT_AOS) != B for x in (qd, qdd, tau)):
                raise _lib.MecanoHipError(2, "batch sizes of the state matrices differ")
            f = None if f_ext is None else _np(f_ext, np.float64)
            self._check_f_ext(f, B, _lib.LAYOUT_AOS)
            tau_out, qdd_out = out if out is not None else (np.empty_like(qd), np.empty_like(qd))
            g, ra = self._root(gravity)
            opts = self._options(_lib.LAYOUT_AOS, root_acceleration=ra)
            _lib.check(lib.mh_rnea_aba_f64_host(self._h, B, q.ctypes.data, qd.ctypes.data, qdd.ctypes.data, tau.ctypes.data, g,
                                                None if f is None else f.ctypes.data, ctypes.byref(opts), tau_out.ctypes.data, qdd_out.ctypes.data))
            return tau_out, qdd_out
        import torch
        for t in (q, qd, qdd, tau) + ((f_ext,) if f_ext is not None else ()):
            if not t.is_cuda or t.dtype not in (torch.float64, torch.float32) or t.dtype != q.dtype or not t.is_contiguous():
                raise ValueError("rnea_aba needs contiguous float64 (or float32) tensors of one dtype on the HIP device")
        B = self._batch(q, self.nq, layout)
        if any(self._batch(x, self.nv, layout) != B for x in (qd, qdd, tau)):
            raise _lib.MecanoHipError(2, "batch sizes of the state matrices differ")
        g, ra = self._root(gravity)
        opts = self._options(layout, True, True, torch.cuda.current_stream(q.device).cuda_stream, root_acceleration=ra)
        tau_out, qdd_out = torch.empty_like(qd), torch.empty_like(qd)
        fn = lib.mh_rnea_aba_f64 if q.dtype == torch.float64 else lib.mh_rnea_aba_f32
        _lib.check(fn(self._h, B, q.data_ptr(), qd.data_ptr(), qdd.data_ptr(), tau.data_ptr(), g,
                      f_ext.data_ptr() if f_ext is not None else None, ctypes.byref(opts), tau_out.data_ptr(), qdd_out.data_ptr()))
        return tau_out, qdd_out

    def rnea_crba(self, q, qd, qdd, gravity=(0.0, 0.0, -9.81), f_ext=None):
        """tau = RNEA(q, qd, qdd) and H = CRBA(q) in one call (mh_rnea_crba_f64; fp64, AoS, device tensors): (tau [B, nv], H [B, nv, nv])."""
        import torch
        lib = _lib.load()
        for t in (q, qd, qdd) + ((f_ext,) if f_ext is not None else ()):
            if not t.is_cuda or t.dtype != torch.float64 or not t.is_contiguous():
                raise ValueError("rnea_crba needs contiguous float64 tensors on the HIP device")
        B = self._batch(q, self.nq, _lib.LAYOUT_AOS)
        if any(self._batch(x, self.nv, _lib.LAYOUT_AOS) != B for x in (qd, qdd)):
            raise _lib.MecanoHipError(2, "batch sizes of the state matrices differ")
        self._check_f_ext(f_ext, B, _lib.LAYOUT_AOS)
        g, ra = self._root(gravity)
        opts = self._options(_lib.LAYOUT_AOS, True, True, torch.cuda.current_stream(q.device).cuda_stream, root_acceleration=ra)
        tau_out = torch.empty_like(qd)
        H = torch.empty((B, self.nv, self.nv), dtype=torch.float64, device=q.device)
        _lib.check(lib.mh_rnea_crba_f64(self._h, B, q.data_ptr(), qd.data_ptr(), qdd.data_ptr(), g, f_ext.data_ptr() if f_ext is not None else None,
                                        ctypes.byref(opts), tau_out.data_ptr(), H.data_ptr()))
        return tau_out, H

    def bind_rnea_aba(self, q, qd, qdd, tau, tau_out, qdd_out, gravity=(0.0, 0.0, -9.81), f_ext=None):
        """Returns a zero-argument callable that issues mh_rnea_aba_f64 (float32 tensors: mh_rnea_aba_f32) on the given (caller-owned,
        device-resident) buffers.
        All argument marshalling is done once here: a steady-state caller (a simulation loop, bench.py) pays one C call per step."""
        import torch
        lib = _lib.load()
        tensors = (q, qd, qdd, tau, tau_out, qdd_out) + ((f_ext,) if f_ext is not None else ())
        for t in tensors:
            if not t.is_cuda or t.dtype not in (torch.float64, torch.float32) or t.dtype != q.dtype or not t.is_contiguous():
                raise ValueError("bind_rnea_aba needs contiguous float64 (or float32) tensors of one dtype on the HIP device")
        B = self._batch(q, self.nq, _lib.LAYOUT_AOS)
        if any(self._batch(x, self.nv, _lib.LAYOUT_AOS) != B for x in (qd, qdd, tau, tau_out, qdd_out)):
            raise _lib.MecanoHipError(2, "batch sizes of the state matrices differ")
        g, ra = self._root(gravity)
        opts = self._options(_lib.LAYOUT_AOS, True, True, torch.cuda.current_stream(q.device).cuda_stream, root_acceleration=ra)
        args = (self._h, ctypes.c_int64(B), ctypes.c_void_p(q.data_ptr()), ctypes.c_void_p(qd.data_ptr()), ctypes.c_void_p(qdd.data_ptr()),
                ctypes.c_void_p(tau.data_ptr()), g, ctypes.c_void_p(f_ext.data_ptr()) if f_ext is not None else None, ctypes.byref(opts),
                ctypes.c_void_p(tau_out.data_ptr()), ctypes.c_void_p(qdd_out.data_ptr()))
        fn = lib.mh_rnea_aba_f64 if q.dtype == torch.float64 else lib.mh_rnea_aba_f32
        keep = (tensors, g, opts)

        def call(_fn=fn, _args=args, _keep=keep):
            st = _fn(*_args)
            if st:
                _lib.check(st)

        return call

    def bind_rnea_crba(self, q, qd, qdd, tau_out, H_out, gravity=(0.0, 0.0, -9.81), f_ext=None):
        """bind_rnea_aba's counterpart for mh_rnea_crba_f64: a zero-argument callable on caller-owned device buffers (H_out is [B, nv, nv])."""
        import torch
        lib = _lib.load()
        tensors = (q, qd, qdd, tau_out, H_out) + ((f_ext,) if f_ext is not None else ())
        for t in tensors:
            if not t.is_cuda or t.dtype != torch.float64 or not t.is_contiguous():
                raise ValueError("bind_rnea_crba needs contiguous float64 tensors on the HIP device")
        B = self._batch(q, self.nq, _lib.LAYOUT_AOS)
        if any(self._batch(x, self.nv, _lib.LAYOUT_AOS) != B for x in (qd, qdd, tau_out)) or tuple(H_out.shape) != (B, self.nv, self.nv):
            raise _lib.MecanoHipError(2, "batch sizes of the state matrices differ")
        self._check_f_ext(f_ext, B, _lib.LAYOUT_AOS)
        g, ra = self._root(gravity)
        opts = self._options(_lib.LAYOUT_AOS, True, True, torch.cuda.current_stream(q.device).cuda_stream, root_acceleration=ra)
        args = (self._h, ctypes.c_int64(B), ctypes.c_void_p(q.data_ptr()), ctypes.c_void_p(qd.data_ptr()), ctypes.c_void_p(qdd.data_ptr()), g,
                ctypes.c_void_p(f_ext.data_ptr()) if f_ext is not None else None, ctypes.byref(opts), ctypes.c_void_p(tau_out.data_ptr()),
                ctypes.c_void_p(H_out.data_ptr()))
        fn = lib.mh_rnea_crba_f64
        keep = (tensors, g, opts)

        def call(_fn=fn, _args=args, _keep=keep):
            st = _fn(*_args)
            if st:
                _lib.check(st)

        return call

    def crba(self, q, layout=_lib.LAYOUT_AOS):
        return self._run("crba", q, None, None, (0.0, 0.0, 0.0), None, layout, True, True)


    # ------------------------------------------------------------------ Coriolis matrix, centroidal momentum
    def _device_inputs(self, tensors, layout):
        import torch
        dt = tensors[0].dtype
        if dt not in (torch.float64, torch.float32):
            raise TypeError("state tensors must be float64 or float32")
        for t in tensors:
            if not t.is_cuda or t.dtype != dt or not t.is_contiguous():
                raise ValueError("device tensors must be contiguous, on the HIP device and of one dtype")
        B = self._batch(tensors[0], self.nq, layout)
        for t in tensors[1:]:
            if self._batch(t, self.nv, layout) != B:
                raise _lib.MecanoHipError(2, "batch sizes of the state matrices differ")
        return B, dt, ("f64" if dt == torch.float64 else "f32"), torch.cuda.current_stream(tensors[0].device).cuda_stream

    def crba_coriolis(self, q, qd, layout=_lib.LAYOUT_AOS):
        """Mass matrix and Coriolis matrix (CompositeRigidBodyMassMatrixCalculator with the Coriolis calculation enabled,
        CompositeRigidBodyMassMatrixCalculator.java:271-274, 344-365): (H, C), device tensors [B, nv, nv]."""
        if not self._is_torch(q):  # numpy: host-pointer entry point (fp64)
            q, qd = _np(q, np.float64), _np(qd, np.float64)
            B = self._batch(q, self.nq, layout)
            if self._batch(qd, self.nv, layout) != B:
                raise _lib.MecanoHipError(2, "batch sizes of the state matrices differ")
            shape = (B, self.nv, self.nv) if layout == _lib.LAYOUT_AOS else (self.nv * self.nv, B)
            H, C = np.empty(shape), np.empty(shape)
            opts = self._options(layout)
            _lib.check(_lib.load().mh_crba_coriolis_f64_host(self._h, B, q.ctypes.data, qd.ctypes.data, ctypes.byref(opts), H.ctypes.data,
                                                             C.ctypes.data))
            return H, C
        import torch
        B, dt, sfx, stream = self._device_inputs([q, qd], layout)
        shape = (B, self.nv, self.nv) if layout == _lib.LAYOUT_AOS else (self.nv * self.nv, B)
        H, C = torch.empty(shape, dtype=dt, device=q.device), torch.empty(shape, dtype=dt, device=q.device)
        opts = self._options(layout, stream=stream)
        _lib.check(getattr(_lib.load(), f"mh_crba_coriolis_{sfx}")(self._h, B, q.data_ptr(), qd.data_ptr(), ctypes.byref(opts), H.data_ptr(),
                                                                  C.data_ptr()))
        return H, C

    def gravity_gradient(self, q, gravity=(0.0, 0.0, -9.81), f_ext=None, layout=_lib.LAYOUT_AOS, out=None):
        """Joint efforts that hold the system against gravity and the external wrenches, and their gradient with respect to the
        configuration (MultiBodyGravityGradientCalculator.getTauMatrix / getTauGradientMatrix, MultiBodyGravityGradientCalculator.java:
        319-351): (tau [B, nv], grad [B, nv, nv]) with tau(q + dq) = tau(q) + grad(q) dq, dq in velocity space, the wrenches held constant
        in the world.  Device tensors (fp64 / fp32); SoA: tau [nv, B], grad [nv * nv, B].  ``gravity`` is the 3-vector g.  ``out``: a
        (tau, grad) pair of tensors to write into; either may be None (that output is then not computed), not both."""
        B, dt, sfx, stream = self._device_inputs([q], layout)
        a = [float(v) for v in np.asarray(gravity, dtype=np.float64).reshape(-1)]
        if len(a) != 3:
            raise _lib.MecanoHipError(2, f"gravity must have 3 entries, got {len(a)}")
        if f_ext is not None:
            self._device_tensor(f_ext, dt)
        self._check_f_ext(f_ext, B, layout)
        aos = layout == _lib.LAYOUT_AOS
        shapes = ((B, self.nv) if aos else (self.nv, B), (B, self.nv, self.nv) if aos else (self.nv * self.nv, B))
        if out is not None:
            tau, grad = out  # (a pair: anything else fails to unpack, here)
            if tau is None and grad is None:
                raise _lib.MecanoHipError(1, "both outputs are None")
        tau, grad = self._outputs(out, shapes, ("tau", "grad"), dt, q.device)
        opts = self._options(layout, stream=stream)
        _lib.check(getattr(_lib.load(), f"mh_gravity_gradient_{sfx}")(self._h, B, q.data_ptr(), (ctypes.c_double * 3)(*a),
                                                                     None if f_ext is None else f_ext.data_ptr(), ctypes.byref(opts),
                                                                     None if tau is None else tau.data_ptr(),
                                                                     None if grad is None else grad.data_ptr()))
        return tau, grad

    def apparent_inertia_inverse(self, q, targets, poses=None, coupled=False, layout=_lib.LAYOUT_AOS, out=None):
        """Inverse apparent inertia of the successor bodies of the joints ``targets`` (positions in the joint list, 1 to 16, duplicates
        allowed): how target b accelerates per unit wrench on target a (MultiBodyResponseCalculator.
        computeRigidBodyApparentSpatialInertiaInverse, applyRigidBodyWrench + getAccelerationChangeProvider,
        MultiBodyResponseCalculator.java:288-440, 608-627, 859-862), one launch.  ``poses`` [K, 12] (R row-major, p) or None: the frame of
        every target relative to its body-fixed frame, in which the wrench acts and the response is expressed.  ``coupled=False``:
        [B, K, 6, 6], the targets' own blocks; ``coupled=True``: [B, 6K, 6K], block (b, a) = response of b to a wrench on a.  SoA:
        [K * 36, B] / [(6K)^2, B].  The model's joint source modes hold.  numpy in -> numpy out (fp64); device tensors (fp64 / fp32)
        stay on the device, and ``out`` is a device tensor to write into."""
        import torch
        if not self._is_torch(q):
            W = self.apparent_inertia_inverse(torch.tensor(_np(q, np.float64), device="cuda"), targets, poses, coupled, layout)
            return W.cpu().numpy()
        B, dt, sfx, stream = self._device_inputs([q], layout)
        tgt = np.ascontiguousarray(np.asarray(targets, dtype=np.int32).reshape(-1))
        K = int(tgt.shape[0])
        if poses is not None:
            poses = np.ascontiguousarray(np.asarray(poses, dtype=np.float64).reshape(-1))
            if poses.shape[0] != 12 * K:
                raise _lib.MecanoHipError(2, f"poses must hold 12 numbers per target ({12 * K}), got {poses.shape[0]}")
        size = 36 * K * K if coupled else 36 * K
        aos_shape = (B, 6 * K, 6 * K) if coupled else (B, K, 6, 6)
        shape = aos_shape if layout == _lib.LAYOUT_AOS else (size, B)
        out = self._output(out, shape, dt, q.device, "W")
        opts = self._options(layout, stream=stream)
        _lib.check(getattr(_lib.load(), f"mh_apparent_inertia_inverse_{sfx}")(
            self._h, B, q.data_ptr(), K, tgt.ctypes.data, None if poses is None else poses.ctypes.data,
            _lib.APPARENT_BLOCKS_COUPLED if coupled else _lib.APPARENT_BLOCKS_DIAGONAL,
            ctypes.byref(opts), out.data_ptr()))
        return out

    # ------------------------------------------------------------------ kinematics: where the bodies are, how they move with the joints
    @staticmethod
    def _kinematic_targets(targets, bases, poses):
        tgt = np.ascontiguousarray(np.asarray(targets, dtype=np.int32).reshape(-1))
        K = int(tgt.shape[0])
        if bases is not None:
            bases = np.ascontiguousarray(np.asarray(bases, dtype=np.int32).reshape(-1))
            if bases.shape[0] != K:
                raise _lib.MecanoHipError(2, f"bases must name one body per target ({K}), got {bases.shape[0]}")
        if poses is not None:
            poses = np.ascontiguousarray(np.asarray(poses, dtype=np.float64).reshape(-1))
            if poses.shape[0] != 12 * K:
                raise _lib.MecanoHipError(2, f"poses must hold 12 numbers per target ({12 * K}), got {poses.shape[0]}")
        return tgt, K, bases, poses

    def body_poses(self, q, targets=None, poses=None, layout=_lib.LAYOUT_AOS, out=None):
        """Poses of frames fixed in bodies, in the root body frame (the frame ``gravity`` is expressed in): [B, K, 12], R row-major then p,
        x_root = R x + p; SoA: [12 K, B].  ``targets``: 1 to 16 positions in the joint list (the joint's successor body; -1 = the root
        body; duplicates allowed), each with a constant pose ``poses`` [K, 12] relative to its body-fixed frame (None: identity).
        ``targets=None``: the body-fixed frame of every body, in joint order (K = n_joints).  numpy in -> numpy out (fp64); device
        tensors (fp64 / fp32) stay on the device, and ``out`` is a device tensor to write into."""
        import torch
        if not self._is_torch(q):
            return self.body_poses(torch.tensor(_np(q, np.float64), device="cuda"), targets, poses, layout).cpu().numpy()
        B, dt, sfx, stream = self._device_inputs([q], layout)
        if targets is None:
            if poses is not None:
                raise _lib.MecanoHipError(1, "poses need targets: every body comes with the identity pose")
            tgt, K = None, self.n_joints
        else:
            tgt, K, _, poses = self._kinematic_targets(targets, None, poses)
        out = self._output(out, (B, K, 12) if layout == _lib.LAYOUT_AOS else (12 * K, B), dt, q.device, "pose")
        opts = self._options(layout, stream=stream)
        _lib.check(getattr(_lib.load(), f"mh_body_poses_{sfx}")(
            self._h, B, q.data_ptr(), K, None if tgt is None else tgt.ctypes.data, None if poses is None else poses.ctypes.data,
            ctypes.byref(opts), out.data_ptr()))
        return out

    def geometric_jacobian(self, q, targets, bases=None, poses=None, qd=None, convective=False, layout=_lib.LAYOUT_AOS, out=None):
        """Geometric Jacobians of K target frames (GeometricJacobianCalculator.getJacobianMatrix, GeometricJacobianCalculator.java:249-279,
        for K kinematic chains in one launch): [B, 6 K, nv], block k = the 6 x nv Jacobian (angular rows, then linear) of target k, with
        J qd the twist of the target frame relative to the body ``bases[k]`` (None: the root body) expressed in the target frame; columns
        indexed like tau, zero off the chain.  ``targets`` / ``bases``: positions in the joint list (-1 = the root body), ``poses``
        [K, 12] the target frames relative to the body-fixed frames (None: identity).  ``convective=True`` (needs ``qd``): returns
        (J, c) with c [B, K, 6] the convective term Jdot qd (getConvectiveTerm, :316-377).  SoA: [6 K nv, B] and [6 K, B].  numpy in ->
        numpy out (fp64); device tensors (fp64 / fp32) stay on the device; ``out``: the tensor J, or the pair (J, c), to write into."""
        import torch
        if not self._is_torch(q):
            r = self.geometric_jacobian(torch.tensor(_np(q, np.float64), device="cuda"), targets, bases, poses,
                                        None if qd is None else torch.tensor(_np(qd, np.float64), device="cuda"), convective, layout)
            return tuple(t.cpu().numpy() for t in r) if convective else r.cpu().numpy()
        if convective and qd is None:
            raise _lib.MecanoHipError(1, "the convective term needs qd")
        B, dt, sfx, stream = self._device_inputs([q] if qd is None else [q, qd], layout)
        tgt, K, bases, poses = self._kinematic_targets(targets, bases, poses)
        aos = layout == _lib.LAYOUT_AOS
        J_out, c_out = (out if convective else (out, None)) if out is not None else (None, None)
        J = self._output(J_out, (B, 6 * K, self.nv) if aos else (6 * K * self.nv, B), dt, q.device, "J")
        c = self._output(c_out, (B, K, 6) if aos else (6 * K, B), dt, q.device, "convective term") if convective else None
        opts = self._options(layout, stream=stream)
        _lib.check(getattr(_lib.load(), f"mh_geometric_jacobian_{sfx}")(
            self._h, B, q.data_ptr(), None if qd is None else qd.data_ptr(), K, None if bases is None else bases.ctypes.data, tgt.ctypes.data,
            None if poses is None else poses.ctypes.data, ctypes.byref(opts), J.data_ptr(), None if c is None else c.data_ptr()))
        return (J, c) if convective else J

    def _kinematic_cotangent(self, g, B, K, per_target, layout, dt, name):
        """``g`` checked as [B, K, per_target] (SoA: [per_target K, B]) beside q."""
        self._device_tensor(g, dt)
        shape = (B, K, per_target) if layout == _lib.LAYOUT_AOS else (per_target * K, B)
        if tuple(g.shape) != shape:
            raise _lib.MecanoHipError(2, f"{name} has shape {tuple(g.shape)}, expected {shape}")

    def body_poses_vjp(self, q, g_pose, targets=None, poses=None, layout=_lib.LAYOUT_AOS, out=None):
        """Reverse mode of ``body_poses``, one launch that writes nv numbers per configuration: for a cotangent ``g_pose`` [B, K, 12] of
        the poses (entry for entry: 9 for R row-major, 3 for p; the nine need not be tangent to the rotations) of the same ``targets`` /
        ``poses``, gq [B, nv] = sum g_pose d pose / d q, a step of q being the velocity-space step of ``configuration_add`` (the chart of
        ``rnea_vjp`` / ``aba_vjp``; ``chart_pullback`` brings it to the raw coordinates).  ``targets=None``: the cotangents of every
        body-fixed frame, in joint order.  SoA: [12 K, B] in, [nv, B] out.  numpy in -> numpy out (fp64); device tensors (fp64 / fp32)
        stay on the device, and ``out`` is a device tensor to write into."""
        import torch
        if not self._is_torch(q):
            dev = [torch.tensor(_np(x, np.float64), device="cuda") for x in (q, g_pose)]
            return self.body_poses_vjp(dev[0], dev[1], targets, poses, layout).cpu().numpy()
        B, dt, sfx, stream = self._device_inputs([q], layout)
        if targets is None:
            if poses is not None:
                raise _lib.MecanoHipError(1, "poses need targets: every body comes with the identity pose")
            tgt, K = None, self.n_joints
        else:
            tgt, K, _, poses = self._kinematic_targets(targets, None, poses)
        self._kinematic_cotangent(g_pose, B, K, 12, layout, dt, "g_pose")
        out = self._output(out, (B, self.nv) if layout == _lib.LAYOUT_AOS else (self.nv, B), dt, q.device, "gq")
        opts = self._options(layout, stream=stream)
        _lib.check(getattr(_lib.load(), f"mh_body_poses_vjp_{sfx}")(
            self._h, B, q.data_ptr(), K, None if tgt is None else tgt.ctypes.data, None if poses is None else poses.ctypes.data,
            g_pose.data_ptr(), ctypes.byref(opts), out.data_ptr()))
        return out

    def jacobian_transpose(self, q, wrench, targets, bases=None, poses=None, layout=_lib.LAYOUT_AOS, out=None):
        """sum_k J_k^T w_k without forming J (GeometricJacobianCalculator.getJointTorques, GeometricJacobianCalculator.java:477-484, summed
        over K chains), one launch: ``wrench`` [B, K, 6] (moment, then force) in the target frames at their origins, J_k exactly the block
        ``geometric_jacobian`` returns for (``bases[k]``, ``targets[k]``, ``poses[k]``); tau [B, nv], indexed like tau.  With a moving
        base the wrench acts on the target body and its opposite on the base body.  SoA: [6 K, B] in, [nv, B] out.  numpy in -> numpy
        out (fp64); device tensors (fp64 / fp32) stay on the device, and ``out`` is a device tensor to write into."""
        import torch
        if targets is None:
            raise _lib.MecanoHipError(1, "jacobian_transpose needs targets: there is no all-bodies form")
        if not self._is_torch(q):
            dev = [torch.tensor(_np(x, np.float64), device="cuda") for x in (q, wrench)]
            return self.jacobian_transpose(dev[0], dev[1], targets, bases, poses, layout).cpu().numpy()
        B, dt, sfx, stream = self._device_inputs([q], layout)
        tgt, K, bases, poses = self._kinematic_targets(targets, bases, poses)
        self._kinematic_cotangent(wrench, B, K, 6, layout, dt, "wrench")
        out = self._output(out, (B, self.nv) if layout == _lib.LAYOUT_AOS else (self.nv, B), dt, q.device, "tau")
        opts = self._options(layout, stream=stream)
        _lib.check(getattr(_lib.load(), f"mh_jacobian_transpose_{sfx}")(
            self._h, B, q.data_ptr(), K, None if bases is None else bases.ctypes.data, tgt.ctypes.data,
            None if poses is None else poses.ctypes.data, wrench.data_ptr(), ctypes.byref(opts), out.data_ptr()))
        return out

    def mass_matrix_inverse(self, q, columns=None, layout=_lib.LAYOUT_AOS, out=None):
        """Inverse of the joint-space inertia matrix, H^-1 = d qdd / d tau, from the articulated-body recursion in one launch
        (MultiBodyResponseCalculator.applyJointWrench and its recursion, MultiBodyResponseCalculator.java:685-735, 1206-1338; H is not
        formed).  ``columns=None``: [B, nv, nv], indexed like ``crba``'s H.  ``columns``: 1 to 64 DoF indices of that index space,
        duplicates allowed: [B, nv, K], column k = H^-1 e_columns[k], with the bits of that column of the full call.  SoA: [nv * nv, B] /
        [nv * K, B].  The model's joint source modes hold: rows and columns of acceleration-source joints are zero.  numpy in -> numpy
        out (fp64); device tensors (fp64 / fp32) stay on the device, and ``out`` is a device tensor to write into."""
        import torch
        if not self._is_torch(q):
            return self.mass_matrix_inverse(torch.tensor(_np(q, np.float64), device="cuda"), columns, layout).cpu().numpy()
        B, dt, sfx, stream = self._device_inputs([q], layout)
        cols = None if columns is None else np.ascontiguousarray(np.asarray(columns, dtype=np.int32).reshape(-1))
        K = self.nv if cols is None else int(cols.shape[0])
        shape = (B, self.nv, K) if layout == _lib.LAYOUT_AOS else (self.nv * K, B)
        out = self._output(out, shape, dt, q.device, "Hinv")
        opts = self._options(layout, stream=stream)
        _lib.check(getattr(_lib.load(), f"mh_mass_matrix_inverse_{sfx}")(
            self._h, B, q.data_ptr(), K, None if cols is None else cols.ctypes.data, ctypes.byref(opts), out.data_ptr()))
        return out

    # ------------------------------------------------------------------ dynamics under bilateral constraints on body frames
    def _constraint_call(self, name, states, targets, rows, poses, active, des, compliance, layout, out, out_names, bases=None):
        """What ``aba_constrained`` and ``constraint_impulse`` share: the target lists as host arrays, the device arguments checked, the
        outputs made.  Returns (B, entry-point suffix, stream, host arrays to keep alive, pointers of the target arguments, outputs);
        with ``bases`` the suffix and the pointers are those of the ``_between_`` entry points."""
        import torch
        B, dt, sfx, stream = self._device_inputs(states, layout)
        tgt, K, bases, poses = self._kinematic_targets(targets, bases, poses)
        row_masks = np.ascontiguousarray(np.asarray(rows, dtype=np.int32).reshape(-1))
        if row_masks.shape[0] != K:
            raise _lib.MecanoHipError(2, f"rows must hold one mask per target ({K}), got {row_masks.shape[0]}")
        aos = layout == _lib.LAYOUT_AOS
        if active is not None:
            self._device_tensor(active, torch.int32)
            if tuple(active.shape) != ((B, K) if aos else (K, B)):
                raise _lib.MecanoHipError(2, f"active has shape {tuple(active.shape)}, expected {(B, K) if aos else (K, B)}")
        wrench_shape = (B, K, 6) if aos else (6 * K, B)
        if des is not None:
            self._device_tensor(des, dt)
            if tuple(des.shape) != wrench_shape:
                raise _lib.MecanoHipError(2, f"{name} has shape {tuple(des.shape)}, expected {wrench_shape}")
        first, lam = self._outputs(out, ((B, self.nv) if aos else (self.nv, B), wrench_shape), out_names, dt, states[0].device)
        if first is None:
            raise _lib.MecanoHipError(1, f"the {out_names[0]} output is None")
        if not float(compliance) >= 0.0:
            raise _lib.MecanoHipError(1, "compliance must be >= 0")
        ptr = lambda t: None if t is None else t.data_ptr()
        args = (None if poses is None else poses.ctypes.data, row_masks.ctypes.data, ptr(active), ptr(des), float(compliance))
        if bases is None:
            return B, sfx, stream, (tgt, poses, row_masks), (K, tgt.ctypes.data) + args, first, lam
        return B, "between_" + sfx, stream, (tgt, bases, poses, row_masks), (K, tgt.ctypes.data, bases.ctypes.data) + args, first, lam

    def aba_constrained(self, q, qd, tau, targets, rows, poses=None, active=None, a_des=None, compliance=0.0, gravity=(0.0, 0.0, -9.81),
                        f_ext=None, layout=_lib.LAYOUT_AOS, out=None, bases=None):
        """Forward dynamics while frames fixed in bodies are held: (qdd [B, nv], lam [B, K, 6]) with
        H qdd + h = tau + J_c^T lam and J_c qdd + c + compliance lam = a_des, J_c the constrained rows of ``geometric_jacobian`` with every
        base at the root and c those of its convective term.  ``targets``: 1 to 8 positions in the joint list (the joint's successor
        body, duplicates allowed), ``poses`` [K, 12] their frames relative to the body-fixed frames (None: identity), ``rows`` one 6-bit
        mask per target (bit i: row i of the target frame, rows 0-2 angular, 3-5 linear; 0b111000 a point contact, 0b111111 a weld).
        ``active`` (int32 device tensor [B, K], None = all): the same mask per configuration; a row takes part where both have its bit.
        ``a_des`` [B, K, 6] (None: zeros).  lam is the wrench (moment, force) the constraint applies to the target's body, at and in the
        target frame; rows that take no part hold 0.  SoA: [nv, B], [6 K, B], active [K, B].  ``gravity`` as for ``aba``.  A singular
        system (compliance = 0 and dependent rows) gives NaN in that configuration only.  ``out``: a (qdd, lam) pair to write into; lam
        may be None.  ``bases`` (None: every frame is held relative to the root body): one position in the joint list per target, -1 =
        the root body; target k is then held relative to that body -- J_c and c those of ``geometric_jacobian`` with these bases -- and
        the base body receives the opposite of lam[k] at the same point (a hand on the other hand, the closing joint of a four-bar)."""
        B, sfx, stream, keep, args, qdd, lam = self._constraint_call("a_des", [q, qd, tau], targets, rows, poses, active, a_des, compliance, layout,
                                                                     out, ("qdd", "lambda"), bases)
        if f_ext is not None:
            self._device_tensor(f_ext, q.dtype)
        self._check_f_ext(f_ext, B, layout)
        g, ra = self._root(gravity)
        opts = self._options(layout, True, True, stream, root_acceleration=ra)
        _lib.check(getattr(_lib.load(), f"mh_aba_constrained_{sfx}")(
            self._h, B, q.data_ptr(), qd.data_ptr(), tau.data_ptr(), g, None if f_ext is None else f_ext.data_ptr(), *args, ctypes.byref(opts),
            qdd.data_ptr(), None if lam is None else lam.data_ptr()))
        return qdd, lam

    def constraint_impulse(self, q, qd, targets, rows, poses=None, active=None, v_des=None, compliance=0.0, layout=_lib.LAYOUT_AOS, out=None,
                           bases=None):
        """The velocity after frames fixed in bodies are stopped: (qd_next [B, nv], impulse [B, K, 6]) with qd_next = qd + H^-1 J_c^T impulse
        and J_c qd_next + compliance impulse = v_des (None: zeros; restitution is the caller's choice of v_des).  Arguments as for
        ``aba_constrained``."""
        B, sfx, stream, keep, args, qd_next, imp = self._constraint_call("v_des", [q, qd], targets, rows, poses, active, v_des, compliance, layout,
                                                                         out, ("qd_next", "impulse"), bases)
        opts = self._options(layout, stream=stream)
        _lib.check(getattr(_lib.load(), f"mh_constraint_impulse_{sfx}")(
            self._h, B, q.data_ptr(), qd.data_ptr(), *args, ctypes.byref(opts), qd_next.data_ptr(), None if imp is None else imp.data_ptr()))
        return qd_next, imp

    def contact_impulse(self, q, qd, targets, mu, poses=None, normals=None, active=None, v_normal=None, compliance=0.0, iterations=50, init=None,
                        layout=_lib.LAYOUT_AOS, out=None):
        """The velocity after frictional point contacts have acted: (qd_next [B, nv], impulse [B, K, 6], residual [B]).  The contact points
        are the origins of the target frames (``targets``, ``poses`` as for ``constraint_impulse``, 1 to 8 of them); ``mu`` one friction
        coefficient per target; ``normals`` [B, K, 3] the contact normals in the root body frame, pointing from the obstacle into the robot
        (None: (0, 0, 1)); ``active`` (int32 [B, K], None = all) which contacts are closed; ``v_normal`` [B, K] the least normal velocity
        after the impulse (None: zeros).  The impulses minimise 1/2 lam^T (S + compliance I) lam + lam^T b over the friction cones
        (include/mecano_hip.h, mh_contact_impulse_*) by ``iterations`` projected Gauss-Seidel sweeps from ``init`` (an impulse of an earlier
        call, None: zeros; it may be the impulse output itself); residual is the largest change of an impulse component in the last sweep.
        impulse[:, k] is the wrench on the target's body at and in the target frame: rows 0-2 and open contacts hold 0.  SoA: [nv, B],
        [6 K, B], [B]; normals [3 K, B], active and v_normal [K, B].  ``out``: a (qd_next, impulse, residual) triple to write into; the
        last two may be None."""
        return self._contact_call(q, qd, targets, None, mu, poses, normals, active, v_normal, compliance, iterations, init, layout, out)

    def contact_impulse_between(self, q, qd, targets, bases, mu, poses=None, normals=None, active=None, v_normal=None, compliance=0.0,
                                iterations=50, init=None, layout=_lib.LAYOUT_AOS, out=None):
        """``contact_impulse`` between two moving bodies: (qd_next [B, nv], impulse [B, K, 6], residual [B]).  ``bases``: one position in
        the joint list per contact, -1 = the root body (None: the root for every contact, the bits of ``contact_impulse``).  Contact k acts
        between the body of ``targets[k]`` and that of ``bases[k]``: its velocity is that of the contact point on the target body relative
        to the base body (the linear rows of ``geometric_jacobian`` with these bases), ``normals`` -- still in the root body frame -- point
        from the base body into the target body, impulse[:, k] acts on the target body and the base body receives its opposite at the
        same point, so that the momentum two bodies of the tree exchange is conserved.  Everything else as for ``contact_impulse``
        (include/mecano_hip.h, mh_contact_impulse_between_*)."""
        return self._contact_call(q, qd, targets, bases, mu, poses, normals, active, v_normal, compliance, iterations, init, layout, out, True)

    def _contact_call(self, q, qd, targets, bases, mu, poses, normals, active, v_normal, compliance, iterations, init, layout, out, between=False):
        """What ``contact_impulse`` and ``contact_impulse_between`` share."""
        import torch
        B, dt, sfx, stream = self._device_inputs([q, qd], layout)
        tgt, K, bases, poses = self._kinematic_targets(targets, bases, poses)
        mus = np.ascontiguousarray(np.asarray(mu, dtype=np.float64).reshape(-1))
        if mus.shape[0] != K:
            raise _lib.MecanoHipError(2, f"mu must hold one coefficient per target ({K}), got {mus.shape[0]}")
        aos = layout == _lib.LAYOUT_AOS
        wrench_shape = (B, K, 6) if aos else (6 * K, B)
        for name, t, tdt, shape in (("normals", normals, dt, (B, K, 3) if aos else (3 * K, B)), ("active", active, torch.int32, (B, K) if aos else (K, B)),
                                    ("v_normal", v_normal, dt, (B, K) if aos else (K, B)), ("init", init, dt, wrench_shape)):
            if t is not None:
                self._device_tensor(t, tdt)
                if tuple(t.shape) != shape:
                    raise _lib.MecanoHipError(2, f"{name} has shape {tuple(t.shape)}, expected {shape}")
        qd_next, imp, res = self._outputs(out, ((B, self.nv) if aos else (self.nv, B), wrench_shape, (B,)), ("qd_next", "impulse", "residual"), dt, q.device)
        if qd_next is None:
            raise _lib.MecanoHipError(1, "the qd_next output is None")
        ptr = lambda t: None if t is None else t.data_ptr()
        opts = self._options(layout, stream=stream)
        head = (K, tgt.ctypes.data) + ((None if bases is None else bases.ctypes.data,) if between else ())
        _lib.check(getattr(_lib.load(), f"mh_contact_impulse_{'between_' if between else ''}{sfx}")(
            self._h, B, q.data_ptr(), qd.data_ptr(), *head, None if poses is None else poses.ctypes.data, mus.ctypes.data, ptr(normals),
            ptr(active), ptr(v_normal), ptr(init), float(compliance), int(iterations), ctypes.byref(opts), qd_next.data_ptr(), ptr(imp), ptr(res)))
        return qd_next, imp, res

    def joint_limit_impulse(self, q, qd, joints, lower, upper, margin=0.0, erp=0.0, compliance=0.0, iterations=50, init=None,
                            layout=_lib.LAYOUT_AOS, out=None):
        """The velocity after joint limits have acted: (qd_next [B, nv], impulse [B, L], residual [B]).  ``joints``: 1 to 64 positions in
        the joint list, revolute or prismatic, each once; ``lower`` / ``upper`` one range per listed joint (-inf / +inf allowed).  A row is
        closed where its joint is within ``margin`` of the nearer limit (or beyond it); closed rows get impulses lam >= 0 towards the
        inside of the range that solve 0 <= lam  _|_  s qd_next + compliance lam + erp gap >= 0 (include/mecano_hip.h,
        mh_joint_limit_impulse_*) by ``iterations`` projected Gauss-Seidel sweeps from ``init`` (an impulse of an earlier call, None:
        zeros; it may be the impulse output itself).  impulse[:, i] is the generalised impulse on joint i, positive pushing q up; open
        rows hold 0.  residual: the largest change of an impulse in the last sweep.  SoA: [nv, B], [L, B], [B].  ``out``: a
        (qd_next, impulse, residual) triple to write into; the last two may be None."""
        B, dt, sfx, stream = self._device_inputs([q, qd], layout)
        jnt = np.ascontiguousarray(np.asarray(joints, dtype=np.int32).reshape(-1))
        lo = np.ascontiguousarray(np.asarray(lower, dtype=np.float64).reshape(-1))
        hi = np.ascontiguousarray(np.asarray(upper, dtype=np.float64).reshape(-1))
        L = int(jnt.shape[0])
        if lo.shape[0] != L or hi.shape[0] != L:
            raise _lib.MecanoHipError(2, f"lower and upper must hold one limit per listed joint ({L}), got {lo.shape[0]} and {hi.shape[0]}")
        aos = layout == _lib.LAYOUT_AOS
        row_shape = (B, L) if aos else (L, B)
        if init is not None:
            self._device_tensor(init, dt)
            if tuple(init.shape) != row_shape:
                raise _lib.MecanoHipError(2, f"init has shape {tuple(init.shape)}, expected {row_shape}")
        qd_next, imp, res = self._outputs(out, ((B, self.nv) if aos else (self.nv, B), row_shape, (B,)), ("qd_next", "impulse", "residual"), dt, q.device)
        if qd_next is None:
            raise _lib.MecanoHipError(1, "the qd_next output is None")
        ptr = lambda t: None if t is None else t.data_ptr()
        opts = self._options(layout, stream=stream)
        _lib.check(getattr(_lib.load(), f"mh_joint_limit_impulse_{sfx}")(
            self._h, B, q.data_ptr(), qd.data_ptr(), L, jnt.ctypes.data, lo.ctypes.data, hi.ctypes.data, float(margin), float(erp), ptr(init),
            float(compliance), int(iterations), ctypes.byref(opts), qd_next.data_ptr(), ptr(imp), ptr(res)))
        return qd_next, imp, res

    def rnea_derivatives(self, q, qd, qdd, gravity=(0.0, 0.0, -9.81), f_ext=None, layout=_lib.LAYOUT_AOS, consider_coriolis=True,
                         consider_accelerations=True, out=None):
        """Inverse dynamics and its first-order derivatives at a moving state, one analytic launch: (tau [B, nv], dtau_dq [B, nv, nv],
        dtau_dqd [B, nv, nv]), entry [i][j] = d tau_i / d q_j resp. d tau_i / d qd_j.  dq is a velocity-space step (what ``integrate``
        applies), the components of qd and qdd are held fixed, the wrenches are held constant in the world.  Device tensors (fp64 /
        fp32); SoA: [nv, B] and [nv * nv, B].  ``gravity``: the 3-vector g or a 6-D root acceleration, as for ``rnea``.  ``qdd`` may be
        None with ``consider_accelerations=False``, ``qd`` with ``consider_coriolis=False``.  ``out``: a (tau, dtau_dq, dtau_dqd) tuple to
        write into; any may be None (not computed), not both matrices."""
        given = [t for t in (q, qd if consider_coriolis else None, qdd if consider_accelerations else None) if t is not None]
        B, dt, sfx, stream = self._device_inputs(given, layout)
        if (consider_coriolis and qd is None) or (consider_accelerations and qdd is None):
            raise _lib.MecanoHipError(1, "qd / qdd may be None only with their switch off")
        if f_ext is not None:
            self._device_tensor(f_ext, dt)
        self._check_f_ext(f_ext, B, layout)
        aos = layout == _lib.LAYOUT_AOS
        vec, mat = (B, self.nv) if aos else (self.nv, B), (B, self.nv, self.nv) if aos else (self.nv * self.nv, B)
        tau, dq, dqd = self._outputs(out, (vec, mat, mat), ("tau", "dtau_dq", "dtau_dqd"), dt, q.device)
        if dq is None and dqd is None:
            raise _lib.MecanoHipError(1, "both matrices are None")
        g, ra = self._root(gravity)
        opts = self._options(layout, consider_coriolis, consider_accelerations, stream, root_acceleration=ra)
        ptr = lambda t: None if t is None else t.data_ptr()
        _lib.check(getattr(_lib.load(), f"mh_rnea_derivatives_{sfx}")(
            self._h, B, q.data_ptr(), ptr(qd) if consider_coriolis else None, ptr(qdd) if consider_accelerations else None, g, ptr(f_ext),
            ctypes.byref(opts), ptr(tau), ptr(dq), ptr(dqd)))
        return tau, dq, dqd

    def aba_derivatives(self, q, qd, tau, gravity=(0.0, 0.0, -9.81), f_ext=None, layout=_lib.LAYOUT_AOS, out=None):
        """Forward dynamics and its first-order derivatives: (qdd [B, nv], dqdd_dq, dqdd_dqd, Hinv [B, nv, nv]) with dqdd_dq = -H^-1
        d tau / d q and dqdd_dqd = -H^-1 d tau / d qd at qdd = aba(q, qd, tau), and d qdd / d tau = H^-1.  Steps, layouts and ``gravity`` as
        for ``rnea_derivatives``.  ``out``: a (qdd, dqdd_dq, dqdd_dqd, Hinv) tuple to write into; any may be None (qdd and Hinv then go to
        scratch of the model), not both derivative matrices.  A model with acceleration-source joints is refused."""
        B, dt, sfx, stream = self._device_inputs([q, qd, tau], layout)
        if f_ext is not None:
            self._device_tensor(f_ext, dt)
        self._check_f_ext(f_ext, B, layout)
        aos = layout == _lib.LAYOUT_AOS
        vec, mat = (B, self.nv) if aos else (self.nv, B), (B, self.nv, self.nv) if aos else (self.nv * self.nv, B)
        qdd, dq, dqd, Hinv = self._outputs(out, (vec, mat, mat, mat), ("qdd", "dqdd_dq", "dqdd_dqd", "Hinv"), dt, q.device)
        if dq is None and dqd is None:
            raise _lib.MecanoHipError(1, "both derivative matrices are None")
        g, ra = self._root(gravity)
        opts = self._options(layout, True, True, stream, root_acceleration=ra)
        ptr = lambda t: None if t is None else t.data_ptr()
        _lib.check(getattr(_lib.load(), f"mh_aba_derivatives_{sfx}")(
            self._h, B, q.data_ptr(), qd.data_ptr(), tau.data_ptr(), g, ptr(f_ext), ctypes.byref(opts), ptr(qdd), ptr(dq), ptr(dqd), ptr(Hinv)))
        return qdd, dq, dqd, Hinv

    def rnea_vjp(self, q, qd, qdd, u, gravity=(0.0, 0.0, -9.81), f_ext=None, layout=_lib.LAYOUT_AOS, consider_coriolis=True,
                 consider_accelerations=True, out=None):
        """Reverse-mode gradients of the inverse dynamics, one O(n) launch and no matrix: for a cotangent ``u`` [B, nv] of the efforts,
        (gq, gqd, gqdd) [B, nv] each with gq = u^T d tau / d q, gqd = u^T d tau / d qd (the matrices of ``rnea_derivatives``: velocity-space
        steps, wrenches held in the world) and gqdd = H(q) u.  ``chart_pullback`` turns gq into the gradient with respect to the raw
        coordinates.  SoA: [nv, B].  ``qdd`` may be None with ``consider_accelerations=False``, ``qd`` with ``consider_coriolis=False``
        (gqd is then zeros).  ``out``: a (gq, gqd, gqdd) tuple to write into; any may be None (not computed), not all three."""
        given = [t for t in (q, qd if consider_coriolis else None, qdd if consider_accelerations else None, u) if t is not None]
        B, dt, sfx, stream = self._device_inputs(given, layout)
        if u is None or (consider_coriolis and qd is None) or (consider_accelerations and qdd is None):
            raise _lib.MecanoHipError(1, "u is needed; qd / qdd may be None only with their switch off")
        if f_ext is not None:
            self._device_tensor(f_ext, dt)
        self._check_f_ext(f_ext, B, layout)
        vec = (B, self.nv) if layout == _lib.LAYOUT_AOS else (self.nv, B)
        gq, gqd, gqdd = self._outputs(out, (vec, vec, vec), ("gq", "gqd", "gqdd"), dt, q.device)
        if gq is None and gqd is None and gqdd is None:
            raise _lib.MecanoHipError(1, "all three outputs are None")
        g, ra = self._root(gravity)
        opts = self._options(layout, consider_coriolis, consider_accelerations, stream, root_acceleration=ra)
        ptr = lambda t: None if t is None else t.data_ptr()
        _lib.check(getattr(_lib.load(), f"mh_rnea_vjp_{sfx}")(
            self._h, B, q.data_ptr(), ptr(qd) if consider_coriolis else None, ptr(qdd) if consider_accelerations else None, g, ptr(f_ext),
            u.data_ptr(), ctypes.byref(opts), ptr(gq), ptr(gqd), ptr(gqdd)))
        return gq, gqd, gqdd

    def aba_vjp(self, q, qd, tau, w, gravity=(0.0, 0.0, -9.81), f_ext=None, layout=_lib.LAYOUT_AOS, out=None):
        """Reverse-mode gradients of the forward dynamics, no matrix: for a cotangent ``w`` [B, nv] of qdd = aba(q, qd, tau),
        (qdd, gq, gqd, gtau) [B, nv] each with gtau = H^-1 w, gq = w^T d qdd / d q and gqd = w^T d qdd / d qd (the matrices of
        ``aba_derivatives``).  Two forward-dynamics launches and the kernel of ``rnea_vjp``.  ``out``: a (qdd, gq, gqd, gtau) tuple to write
        into; any may be None, not all three gradients.  A model with acceleration-source joints is refused."""
        B, dt, sfx, stream = self._device_inputs([q, qd, tau, w], layout)
        if f_ext is not None:
            self._device_tensor(f_ext, dt)
        self._check_f_ext(f_ext, B, layout)
        vec = (B, self.nv) if layout == _lib.LAYOUT_AOS else (self.nv, B)
        qdd, gq, gqd, gtau = self._outputs(out, (vec, vec, vec, vec), ("qdd", "gq", "gqd", "gtau"), dt, q.device)
        if gq is None and gqd is None and gtau is None:
            raise _lib.MecanoHipError(1, "all three gradients are None")
        g, ra = self._root(gravity)
        opts = self._options(layout, True, True, stream, root_acceleration=ra)
        ptr = lambda t: None if t is None else t.data_ptr()
        _lib.check(getattr(_lib.load(), f"mh_aba_vjp_{sfx}")(
            self._h, B, q.data_ptr(), qd.data_ptr(), tau.data_ptr(), g, ptr(f_ext), w.data_ptr(), ctypes.byref(opts), ptr(qdd), ptr(gq), ptr(gqd),
            ptr(gtau)))
        return qdd, gq, gqd, gtau

    def chart_pullback(self, q, g):
        """The gradient with respect to the raw coordinates q [B, nq] from a velocity-space gradient g [B, nv] (gq of ``rnea_vjp`` /
        ``aba_vjp``): ``mecano_amd.autograd.chart_pullback`` on this model's index maps.  Plain torch operations, AoS, any device."""
        from . import autograd
        if getattr(self, "_chart_index", None) is None:
            self._chart_index = autograd.chart_maps(self.desc)
        return autograd.chart_pullback(self.desc, q, g, self._chart_index)

    def chart_cotangent(self, q, g_raw):
        """The velocity-space cotangent [B, nv] at q from a gradient with respect to the raw coordinates g_raw [B, nq]:
        ``mecano_amd.autograd.chart_cotangent`` on this model's index maps.  Plain torch operations, AoS, any device."""
        from . import autograd
        if getattr(self, "_chart_index", None) is None:
            self._chart_index = autograd.chart_maps(self.desc)
        return autograd.chart_cotangent(self.desc, q, g_raw, self._chart_index)

    def _cotangents(self, gq_next, gqd_next, vec, dt):
        """The two cotangents of a step: either may be None (zero), not both; shapes and dtype as the state vectors."""
        if gq_next is None and gqd_next is None:
            raise _lib.MecanoHipError(1, "gq_next and gqd_next are both None")
        for t in (gq_next, gqd_next):
            if t is not None:
                self._device_tensor(t, dt)
                if tuple(t.shape) != vec:
                    raise _lib.MecanoHipError(2, f"cotangent has shape {tuple(t.shape)}, expected {vec}")

    def integrate_vjp(self, dt, qd, qdd, gq_next, gqd_next, layout=_lib.LAYOUT_AOS, out=None):
        """Reverse-mode gradients of ``integrate``, one elementwise launch: for cotangents ``gq_next``, ``gqd_next`` [B, nv] of the new
        state (q_next as a velocity-space step, qd_next by components; either may be None for zero), (gq, gqd, gqdd) [B, nv] each: the
        transpose of the integrator's tangent map in the conventions of ``step_derivatives``.  The configuration does not appear.
        SoA: [nv, B].  fp64 / fp32.  ``out``: a (gq, gqd, gqdd) tuple to write into; any may be None (not computed), not all three."""
        import torch
        dtp = qd.dtype
        if dtp not in (torch.float64, torch.float32):
            raise TypeError("state tensors must be float64 or float32")
        for t in (qd, qdd):
            self._device_tensor(t, dtp)
        B = self._batch(qd, self.nv, layout)
        if self._batch(qdd, self.nv, layout) != B:
            raise _lib.MecanoHipError(2, "batch sizes of the state matrices differ")
        vec = (B, self.nv) if layout == _lib.LAYOUT_AOS else (self.nv, B)
        self._cotangents(gq_next, gqd_next, vec, dtp)
        gq, gqd, gqdd = self._outputs(out, (vec, vec, vec), ("gq", "gqd", "gqdd"), dtp, qd.device)
        if gq is None and gqd is None and gqdd is None:
            raise _lib.MecanoHipError(1, "all three outputs are None")
        opts = self._options(layout, True, True, torch.cuda.current_stream(qd.device).cuda_stream)
        ptr = lambda t: None if t is None else t.data_ptr()
        sfx = "f64" if dtp == torch.float64 else "f32"
        _lib.check(getattr(_lib.load(), f"mh_integrate_vjp_{sfx}")(
            self._h, B, float(dt), qd.data_ptr(), qdd.data_ptr(), ptr(gq_next), ptr(gqd_next), ctypes.byref(opts), ptr(gq), ptr(gqd), ptr(gqdd)))
        return gq, gqd, gqdd

    def step_vjp(self, dt, q, qd, tau, gq_next, gqd_next, gravity=(0.0, 0.0, -9.81), f_ext=None, layout=_lib.LAYOUT_AOS, out=None):
        """Reverse-mode gradients of the simulation step ``aba`` then ``integrate`` with step ``dt``, no matrix: for cotangents
        ``gq_next``, ``gqd_next`` [B, nv] of the new state (either may be None for zero), (qdd, gq, gqd, gtau) [B, nv] each with
        (gq, gqd) = A^T g' and gtau = B^T g' for the (A, B) of ``step_derivatives``.  ``chart_cotangent`` makes gq_next from a gradient
        with respect to raw coordinates, ``chart_pullback`` turns gq into one.  Two forward-dynamics launches, the kernel of
        ``integrate_vjp`` and that of ``rnea_vjp``.  SoA: [nv, B].  fp64 / fp32.  ``out``: a (qdd, gq, gqd, gtau) tuple to write into; any
        may be None, not all three gradients.  A model with acceleration-source joints is refused."""
        B, dtp, sfx, stream = self._device_inputs([q, qd, tau], layout)
        if f_ext is not None:
            self._device_tensor(f_ext, dtp)
        self._check_f_ext(f_ext, B, layout)
        vec = (B, self.nv) if layout == _lib.LAYOUT_AOS else (self.nv, B)
        self._cotangents(gq_next, gqd_next, vec, dtp)
        qdd, gq, gqd, gtau = self._outputs(out, (vec, vec, vec, vec), ("qdd", "gq", "gqd", "gtau"), dtp, q.device)
        if gq is None and gqd is None and gtau is None:
            raise _lib.MecanoHipError(1, "all three gradients are None")
        g, ra = self._root(gravity)
        opts = self._options(layout, True, True, stream, root_acceleration=ra)
        ptr = lambda t: None if t is None else t.data_ptr()
        _lib.check(getattr(_lib.load(), f"mh_aba_integrate_vjp_{sfx}")(
            self._h, B, float(dt), q.data_ptr(), qd.data_ptr(), tau.data_ptr(), g, ptr(f_ext), ptr(gq_next), ptr(gqd_next), ctypes.byref(opts),
            ptr(qdd), ptr(gq), ptr(gqd), ptr(gtau)))
        return qdd, gq, gqd, gtau

    def _directions(self, directions, names, vec, dt):
        """The directions of a forward-mode call: any may be None (zero), not all; shapes and dtype as the state vectors."""
        if all(t is None for t in directions):
            raise _lib.MecanoHipError(1, f"{', '.join(names)} are all None")
        for t, name in zip(directions, names):
            if t is not None:
                self._device_tensor(t, dt)
                if tuple(t.shape) != vec:
                    raise _lib.MecanoHipError(2, f"direction {name} has shape {tuple(t.shape)}, expected {vec}")

    def rnea_jvp(self, q, qd, qdd, dq, dqd, dqdd, gravity=(0.0, 0.0, -9.81), f_ext=None, layout=_lib.LAYOUT_AOS, consider_coriolis=True,
                 consider_accelerations=True, out=None):
        """Forward-mode derivative of the inverse dynamics, one O(n) launch and no matrix: for directions ``dq`` (a velocity-space step
        of ``configuration_add``), ``dqd``, ``dqdd`` [B, nv] (any may be None for zero, not all), dtau [B, nv] =
        (d tau / d q) dq + (d tau / d qd) dqd + H dqdd with the matrices of ``rnea_derivatives`` (wrenches held in the world).  SoA:
        [nv, B].  ``qdd`` may be None with ``consider_accelerations=False``, ``qd`` with ``consider_coriolis=False`` (dqd then contributes
        nothing and may be None too).  ``out``: the tensor to write into."""
        given = [t for t in (q, qd if consider_coriolis else None, qdd if consider_accelerations else None) if t is not None]
        B, dt, sfx, stream = self._device_inputs(given, layout)
        if (consider_coriolis and qd is None) or (consider_accelerations and qdd is None):
            raise _lib.MecanoHipError(1, "qd / qdd may be None only with their switch off")
        if f_ext is not None:
            self._device_tensor(f_ext, dt)
        self._check_f_ext(f_ext, B, layout)
        vec = (B, self.nv) if layout == _lib.LAYOUT_AOS else (self.nv, B)
        self._directions((dq, dqd, dqdd), ("dq", "dqd", "dqdd"), vec, dt)
        dtau = self._output(out, vec, dt, q.device, "dtau")
        g, ra = self._root(gravity)
        opts = self._options(layout, consider_coriolis, consider_accelerations, stream, root_acceleration=ra)
        ptr = lambda t: None if t is None else t.data_ptr()
        _lib.check(getattr(_lib.load(), f"mh_rnea_jvp_{sfx}")(
            self._h, B, q.data_ptr(), ptr(qd) if consider_coriolis else None, ptr(qdd) if consider_accelerations else None, g, ptr(f_ext),
            ptr(dq), ptr(dqd), ptr(dqdd), ctypes.byref(opts), dtau.data_ptr()))
        return dtau

    def aba_jvp(self, q, qd, tau, dq, dqd, dtau, gravity=(0.0, 0.0, -9.81), f_ext=None, layout=_lib.LAYOUT_AOS, out=None):
        """Forward-mode derivative of the forward dynamics, no matrix: for directions ``dq``, ``dqd``, ``dtau`` [B, nv] (any may be None
        for zero, not all), (qdd, dqdd) [B, nv] each with dqdd = (d qdd / d q) dq + (d qdd / d qd) dqd + H^-1 dtau (the matrices of
        ``aba_derivatives``) at qdd = aba(q, qd, tau).  Two forward-dynamics launches and the kernel of ``rnea_jvp`` between them.
        ``out``: a (qdd, dqdd) tuple to write into; qdd may be None.  A model with acceleration-source joints is refused."""
        B, dt, sfx, stream = self._device_inputs([q, qd, tau], layout)
        if f_ext is not None:
            self._device_tensor(f_ext, dt)
        self._check_f_ext(f_ext, B, layout)
        vec = (B, self.nv) if layout == _lib.LAYOUT_AOS else (self.nv, B)
        self._directions((dq, dqd, dtau), ("dq", "dqd", "dtau"), vec, dt)
        qdd, dqdd = self._outputs(out, (vec, vec), ("qdd", "dqdd"), dt, q.device)
        if dqdd is None:
            raise _lib.MecanoHipError(1, "dqdd is None")
        g, ra = self._root(gravity)
        opts = self._options(layout, True, True, stream, root_acceleration=ra)
        ptr = lambda t: None if t is None else t.data_ptr()
        _lib.check(getattr(_lib.load(), f"mh_aba_jvp_{sfx}")(
            self._h, B, q.data_ptr(), qd.data_ptr(), tau.data_ptr(), g, ptr(f_ext), ptr(dq), ptr(dqd), ptr(dtau), ctypes.byref(opts), ptr(qdd),
            ptr(dqdd)))
        return qdd, dqdd

    def integrate_jvp(self, dt, qd, qdd, dq, dqd, dqdd, layout=_lib.LAYOUT_AOS, out=None):
        """Forward-mode derivative of ``integrate``, one elementwise launch: for directions ``dq``, ``dqd``, ``dqdd`` [B, nv] (any may be
        None for zero, not all), (dq_next, dqd_next) [B, nv]: the integrator's tangent map in the conventions of ``step_derivatives``
        (dq_next the velocity-space step of q_next); ``integrate_vjp`` is its transpose.  The configuration does not appear.  SoA:
        [nv, B].  fp64 / fp32.  ``out``: a (dq_next, dqd_next) tuple to write into; either may be None (not computed), not both."""
        import torch
        dtp = qd.dtype
        if dtp not in (torch.float64, torch.float32):
            raise TypeError("state tensors must be float64 or float32")
        for t in (qd, qdd):
            self._device_tensor(t, dtp)
        B = self._batch(qd, self.nv, layout)
        if self._batch(qdd, self.nv, layout) != B:
            raise _lib.MecanoHipError(2, "batch sizes of the state matrices differ")
        vec = (B, self.nv) if layout == _lib.LAYOUT_AOS else (self.nv, B)
        self._directions((dq, dqd, dqdd), ("dq", "dqd", "dqdd"), vec, dtp)
        dqn, dqdn = self._outputs(out, (vec, vec), ("dq_next", "dqd_next"), dtp, qd.device)
        if dqn is None and dqdn is None:
            raise _lib.MecanoHipError(1, "both outputs are None")
        opts = self._options(layout, True, True, torch.cuda.current_stream(qd.device).cuda_stream)
        ptr = lambda t: None if t is None else t.data_ptr()
        sfx = "f64" if dtp == torch.float64 else "f32"
        _lib.check(getattr(_lib.load(), f"mh_integrate_jvp_{sfx}")(
            self._h, B, float(dt), qd.data_ptr(), qdd.data_ptr(), ptr(dq), ptr(dqd), ptr(dqdd), ctypes.byref(opts), ptr(dqn), ptr(dqdn)))
        return dqn, dqdn

    def step_jvp(self, dt, q, qd, tau, dq, dqd, dtau, gravity=(0.0, 0.0, -9.81), f_ext=None, layout=_lib.LAYOUT_AOS, out=None):
        """Forward-mode derivative of the simulation step ``aba`` then ``integrate`` with step ``dt``, no matrix: for directions ``dq``,
        ``dqd``, ``dtau`` [B, nv] (any may be None for zero, not all), (qdd, dqdd, dq_next, dqd_next) [B, nv] each with
        (dq_next, dqd_next) = A (dq, dqd) + B dtau for the (A, B) of ``step_derivatives``: ``aba_jvp`` followed by ``integrate_jvp``, bit
        for bit.  SoA: [nv, B].  fp64 / fp32.  ``out``: a (qdd, dqdd, dq_next, dqd_next) tuple to write into; any may be None, not all
        three tangents.  A model with acceleration-source joints is refused."""
        B, dtp, sfx, stream = self._device_inputs([q, qd, tau], layout)
        if f_ext is not None:
            self._device_tensor(f_ext, dtp)
        self._check_f_ext(f_ext, B, layout)
        vec = (B, self.nv) if layout == _lib.LAYOUT_AOS else (self.nv, B)
        self._directions((dq, dqd, dtau), ("dq", "dqd", "dtau"), vec, dtp)
        qdd, dqdd, dqn, dqdn = self._outputs(out, (vec, vec, vec, vec), ("qdd", "dqdd", "dq_next", "dqd_next"), dtp, q.device)
        if dqdd is None and dqn is None and dqdn is None:
            raise _lib.MecanoHipError(1, "all three tangents are None")
        g, ra = self._root(gravity)
        opts = self._options(layout, True, True, stream, root_acceleration=ra)
        ptr = lambda t: None if t is None else t.data_ptr()
        _lib.check(getattr(_lib.load(), f"mh_aba_integrate_jvp_{sfx}")(
            self._h, B, float(dt), q.data_ptr(), qd.data_ptr(), tau.data_ptr(), g, ptr(f_ext), ptr(dq), ptr(dqd), ptr(dtau), ctypes.byref(opts),
            ptr(qdd), ptr(dqdd), ptr(dqn), ptr(dqdn)))
        return qdd, dqdd, dqn, dqdn

    def _chart_call(self, name, a, b, b_cols, out_cols, layout, out):
        B, dt, sfx, stream = self._device_inputs([a], layout)
        aos = layout == _lib.LAYOUT_AOS
        shape_of = lambda n: (B, n) if aos else (n, B)
        self._device_tensor(b, dt)
        if tuple(b.shape) != shape_of(b_cols):
            raise _lib.MecanoHipError(2, f"second input has shape {tuple(b.shape)}, expected {shape_of(b_cols)}")
        out = self._output(out, shape_of(out_cols), dt, a.device)
        opts = self._options(layout, stream=stream)
        _lib.check(getattr(_lib.load(), f"{name}_{sfx}")(self._h, B, a.data_ptr(), b.data_ptr(), ctypes.byref(opts), out.data_ptr()))
        return out

    def configuration_add(self, q, dq, layout=_lib.LAYOUT_AOS, out=None):
        """q (+) dq, the pure configuration step the velocity-space derivatives are defined in: ``integrateFromVelocity`` with dt = 1 and
        twist dq [B, nv] (SixDoF: Q exp(dth), p + R(Q) dp).  Not ``integrate`` with qd = dq, whose double integrator adds a w x v term.
        Device tensors (fp64 / fp32); ``out`` may be q itself.  Entries of q no joint owns are copied only when ``out`` is None."""
        if out is None:
            out = q.clone()
        return self._chart_call("mh_configuration_add", q, dq, self.nv, self.nq, layout, out)

    def configuration_difference(self, q0, q1, layout=_lib.LAYOUT_AOS, out=None):
        """The dq [B, nv] with q0 (+) dq = q1: rotation vectors in their shortest form, dp = R(Q0)^T (p1 - p0)."""
        return self._chart_call("mh_configuration_difference", q0, q1, self.nq, self.nv, layout, out)

    def step_derivatives(self, dt, q, qd, tau, gravity=(0.0, 0.0, -9.81), f_ext=None, layout=_lib.LAYOUT_AOS, out=None):
        """Linearisation of the simulation step ``aba`` then ``integrate`` with step ``dt``: (qdd [B, nv], q_next [B, nq], qd_next [B, nv],
        A [B, 2nv, 2nv], B [B, 2nv, nv]) with dx' = A dx + B dtau, x = (q, qd); dq and dq' are velocity-space steps in the chart of
        ``configuration_add`` / ``configuration_difference``, dqd and dqd' component increments, the wrenches held in the world.  SoA:
        [nv, B], [nq, B], [nv, B], [(2nv)^2, B], [2nv nv, B].  ``out``: a (qdd, q_next, qd_next, A, B) tuple to write into; any may be None
        (not returned), not both matrices, q_next and qd_next only together.  A model with acceleration-source joints is refused."""
        import torch
        B, dtp, sfx, stream = self._device_inputs([q, qd, tau], layout)
        if f_ext is not None:
            self._device_tensor(f_ext, dtp)
        self._check_f_ext(f_ext, B, layout)
        aos, nv = layout == _lib.LAYOUT_AOS, self.nv
        shapes = ((B, nv), (B, self.nq), (B, nv), (B, 2 * nv, 2 * nv), (B, 2 * nv, nv)) if aos else \
                 ((nv, B), (self.nq, B), (nv, B), (4 * nv * nv, B), (2 * nv * nv, B))
        names = ("qdd", "q_next", "qd_next", "A", "B")
        if out is None:
            out = tuple(torch.empty(s, dtype=dtp, device=q.device) for s in shapes)
            out = (out[0], q.clone(), qd.clone()) + out[3:]  # entries no joint owns are passed through unchanged
        else:
            out = self._outputs(out, shapes, names, dtp, q.device)
        g, ra = self._root(gravity)
        opts = self._options(layout, True, True, stream, root_acceleration=ra)
        ptr = lambda t: None if t is None else t.data_ptr()
        _lib.check(getattr(_lib.load(), f"mh_aba_integrate_derivatives_{sfx}")(
            self._h, B, float(dt), q.data_ptr(), qd.data_ptr(), tau.data_ptr(), g, ptr(f_ext), ctypes.byref(opts), *[ptr(t) for t in out]))
        return tuple(out)

    def inertial_parameters(self) -> np.ndarray:
        """The model's own inertial parameters, [n_joints, 10]: (mass, com_x, com_y, com_z, Jxx, Jxy, Jxz, Jyy, Jyz, Jzz) of joint j's
        successor body in the description's order -- ``inertia_mass``, ``inertia_com`` and the symmetric part of ``inertia_J``, the order
        of ``regressor`` and of ``OracleModel.parameter_vector``.  A row of ``pi`` for ``rnea_parameters`` / ``aba_parameters`` is this
        array flattened: perturb it instead of reconstructing it."""
        out = np.empty((self.n_joints, 10), dtype=np.float64)
        _lib.check(_lib.load().mh_model_inertial_parameters(self._h, out.ctypes.data))
        return out

    def _parameters_call(self, kind, q, qd, x3, pi, gravity, f_ext, layout, consider_coriolis, consider_accelerations, out):
        import torch
        if not self._is_torch(q):  # numpy in -> numpy out (float32 arrays go to the fp32 kernels)
            ndt = np.float32 if getattr(q, "dtype", None) == np.float32 else np.float64
            dev = lambda x: None if x is None else torch.tensor(_np(x, ndt), device="cuda")
            res = self._parameters_call(kind, dev(q), dev(qd), dev(x3), dev(pi), gravity, dev(f_ext), layout, consider_coriolis,
                                        consider_accelerations, None).cpu().numpy()
            if out is not None:
                out[...] = res
                return out
            return res
        B, dt, sfx, stream = self._device_inputs([q, qd, x3], layout)
        aos = layout == _lib.LAYOUT_AOS
        for t in (pi, f_ext):
            if t is not None:
                self._device_tensor(t, dt)
        if pi is None:
            raise _lib.MecanoHipError(1, "pi is None")
        want = ((B, self.n_joints, 10), (B, self.n_joints * 10)) if aos else ((self.n_joints * 10, B),)
        if tuple(pi.shape) not in want:
            raise _lib.MecanoHipError(2, f"inertial parameters have shape {tuple(pi.shape)}, expected {want[0]}")
        self._check_f_ext(f_ext, B, layout)
        out = self._output(out, tuple(qd.shape), dt, qd.device)
        g, ra = self._root(gravity)
        opts = self._options(layout, consider_coriolis, consider_accelerations, stream, root_acceleration=ra)
        _lib.check(getattr(_lib.load(), f"mh_{kind}_parameters_{sfx}")(
            self._h, B, q.data_ptr(), qd.data_ptr(), x3.data_ptr(), pi.data_ptr(), g, None if f_ext is None else f_ext.data_ptr(),
            ctypes.byref(opts), out.data_ptr()))
        return out

    def rnea_parameters(self, q, qd, qdd, pi, gravity=(0.0, 0.0, -9.81), f_ext=None, layout=_lib.LAYOUT_AOS, consider_coriolis=True,
                        consider_accelerations=True, out=None):
        """Inverse dynamics of B different robots of this model's topology and geometry: row r is evaluated with the inertial parameters
        ``pi[r]`` ([B, n_joints, 10]; SoA: [10 n_joints, B]; the ten numbers and their order as in ``inertial_parameters``).  Everything
        else as for ``rnea``.  Device tensors (fp64 / fp32) stay on the device, ``out`` is a device tensor to write into -- it may be qd or
        qdd themselves (include/mecano_hip.h, "Aliasing"), any other overlap with an input is refused; numpy in -> numpy out."""
        return self._parameters_call("rnea", q, qd, qdd, pi, gravity, f_ext, layout, consider_coriolis, consider_accelerations, out)

    def aba_parameters(self, q, qd, tau, pi, gravity=(0.0, 0.0, -9.81), f_ext=None, layout=_lib.LAYOUT_AOS, out=None):
        """Forward dynamics of B different robots: row r with the inertial parameters ``pi[r]``, laid out as for ``rnea_parameters``;
        everything else as for ``aba`` (``out`` may be qd or tau themselves, no other overlap).  A ``pi`` that is no physical inertia is not diagnosed: it shows as inf / nan in that row only.
        A model with acceleration-source joints is refused."""
        return self._parameters_call("aba", q, qd, tau, pi, gravity, f_ext, layout, True, True, out)

    def _parameter_tensor(self, pi, B, dt, layout, name="pi"):
        """``pi`` checked as a device tensor of the parameters' shape; returns that shape as given."""
        if pi is None:
            raise _lib.MecanoHipError(1, f"{name} is None")
        self._device_tensor(pi, dt)
        want = ((B, self.n_joints, 10), (B, self.n_joints * 10)) if layout == _lib.LAYOUT_AOS else ((self.n_joints * 10, B),)
        if tuple(pi.shape) not in want:
            raise _lib.MecanoHipError(2, f"{name} has shape {tuple(pi.shape)}, expected {want[0]}")
        return tuple(pi.shape)

    def rnea_parameters_vjp(self, q, qd, qdd, pi, u, gravity=(0.0, 0.0, -9.81), layout=_lib.LAYOUT_AOS, consider_coriolis=True,
                            consider_accelerations=True, out=None):
        """Reverse-mode gradient of ``rnea_parameters`` with respect to the inertial parameters, one O(n) launch and no regressor: for a
        cotangent ``u`` [B, nv] of the efforts, gpi = u^T d tau / d pi in the shape of ``pi`` ([B, n_joints, 10]; SoA: [10 n_joints, B]),
        with respect to the ten numbers (mass, com, J) themselves.  ``qdd`` may be None with ``consider_accelerations=False``, ``qd`` with
        ``consider_coriolis=False``.  External wrenches do not enter (the efforts are affine in them).  Device tensors, fp64 / fp32;
        ``out``: a device tensor of pi's shape to write into."""
        given = [t for t in (q, qd if consider_coriolis else None, qdd if consider_accelerations else None, u) if t is not None]
        B, dt, sfx, stream = self._device_inputs(given, layout)
        if u is None or (consider_coriolis and qd is None) or (consider_accelerations and qdd is None):
            raise _lib.MecanoHipError(1, "u is needed; qd / qdd may be None only with their switch off")
        gpi = self._output(out, self._parameter_tensor(pi, B, dt, layout), dt, q.device, "gpi")
        g, ra = self._root(gravity)
        opts = self._options(layout, consider_coriolis, consider_accelerations, stream, root_acceleration=ra)
        ptr = lambda t: None if t is None else t.data_ptr()
        _lib.check(getattr(_lib.load(), f"mh_rnea_parameters_vjp_{sfx}")(
            self._h, B, q.data_ptr(), ptr(qd) if consider_coriolis else None, ptr(qdd) if consider_accelerations else None, pi.data_ptr(), g,
            u.data_ptr(), ctypes.byref(opts), gpi.data_ptr()))
        return gpi

    def aba_parameters_vjp(self, q, qd, tau, pi, w, gravity=(0.0, 0.0, -9.81), f_ext=None, layout=_lib.LAYOUT_AOS, out=None):
        """Reverse-mode gradient of ``aba_parameters`` with respect to the inertial parameters: for a cotangent ``w`` [B, nv] of
        qdd = aba_parameters(q, qd, tau, pi), (qdd, gtau, gpi) with gtau = H(pi)^-1 w [B, nv] and gpi = w^T d qdd / d pi in the shape of
        ``pi``.  Two forward-dynamics launches and the kernel of ``rnea_parameters_vjp``.  ``out``: a (qdd, gtau, gpi) tuple to write into;
        qdd and gtau may be None (they then go to scratch of the model and None is returned in their place), gpi not.  A model with
        acceleration-source joints is refused."""
        B, dt, sfx, stream = self._device_inputs([q, qd, tau, w], layout)
        if f_ext is not None:
            self._device_tensor(f_ext, dt)
        self._check_f_ext(f_ext, B, layout)
        vec = (B, self.nv) if layout == _lib.LAYOUT_AOS else (self.nv, B)
        qdd, gtau, gpi = self._outputs(out, (vec, vec, self._parameter_tensor(pi, B, dt, layout)), ("qdd", "gtau", "gpi"), dt, q.device)
        if gpi is None:
            raise _lib.MecanoHipError(1, "the gpi output is None")
        g, ra = self._root(gravity)
        opts = self._options(layout, True, True, stream, root_acceleration=ra)
        ptr = lambda t: None if t is None else t.data_ptr()
        _lib.check(getattr(_lib.load(), f"mh_aba_parameters_vjp_{sfx}")(
            self._h, B, q.data_ptr(), qd.data_ptr(), tau.data_ptr(), pi.data_ptr(), g, ptr(f_ext), w.data_ptr(), ctypes.byref(opts), ptr(qdd),
            ptr(gtau), gpi.data_ptr()))
        return qdd, gtau, gpi

    def rnea_parameters_state_vjp(self, q, qd, qdd, pi, u, gravity=(0.0, 0.0, -9.81), f_ext=None, layout=_lib.LAYOUT_AOS, consider_coriolis=True,
                                  consider_accelerations=True, out=None):
        """Reverse-mode gradients of ``rnea_parameters`` with respect to the state AND the inertial parameters, one O(n) launch: for a
        cotangent ``u`` [B, nv] of the efforts, (gq, gqd, gqdd, gpi) -- what ``rnea_vjp`` gives, with the inertias of row r taken from
        ``pi[r]`` (gqdd = H(pi) u), and what ``rnea_parameters_vjp`` gives, from one pair of sweeps.  Shapes, layouts, ``chart_pullback``
        and the two switches as in those two.  ``out``: a (gq, gqd, gqdd, gpi) tuple to write into; any may be None (not computed), not all
        four.  A model with acceleration-source joints is refused."""
        given = [t for t in (q, qd if consider_coriolis else None, qdd if consider_accelerations else None, u) if t is not None]
        B, dt, sfx, stream = self._device_inputs(given, layout)
        if u is None or (consider_coriolis and qd is None) or (consider_accelerations and qdd is None):
            raise _lib.MecanoHipError(1, "u is needed; qd / qdd may be None only with their switch off")
        if f_ext is not None:
            self._device_tensor(f_ext, dt)
        self._check_f_ext(f_ext, B, layout)
        vec = (B, self.nv) if layout == _lib.LAYOUT_AOS else (self.nv, B)
        gq, gqd, gqdd, gpi = self._outputs(out, (vec, vec, vec, self._parameter_tensor(pi, B, dt, layout)), ("gq", "gqd", "gqdd", "gpi"), dt, q.device)
        if gq is None and gqd is None and gqdd is None and gpi is None:
            raise _lib.MecanoHipError(1, "all four outputs are None")
        g, ra = self._root(gravity)
        opts = self._options(layout, consider_coriolis, consider_accelerations, stream, root_acceleration=ra)
        ptr = lambda t: None if t is None else t.data_ptr()
        _lib.check(getattr(_lib.load(), f"mh_rnea_parameters_state_vjp_{sfx}")(
            self._h, B, q.data_ptr(), ptr(qd) if consider_coriolis else None, ptr(qdd) if consider_accelerations else None, pi.data_ptr(), g,
            ptr(f_ext), u.data_ptr(), ctypes.byref(opts), ptr(gq), ptr(gqd), ptr(gqdd), ptr(gpi)))
        return gq, gqd, gqdd, gpi

    def aba_parameters_state_vjp(self, q, qd, tau, pi, w, gravity=(0.0, 0.0, -9.81), f_ext=None, layout=_lib.LAYOUT_AOS, out=None):
        """Reverse-mode gradients of ``aba_parameters`` with respect to the state AND the inertial parameters: for a cotangent ``w``
        [B, nv] of qdd = aba_parameters(q, qd, tau, pi), (qdd, gq, gqd, gtau, gpi) -- what ``aba_vjp`` gives at H(pi_r) and the inertias of
        row r, and the gpi of ``aba_parameters_vjp``.  Two forward-dynamics launches and the kernel of ``rnea_parameters_state_vjp``.
        ``out``: a (qdd, gq, gqd, gtau, gpi) tuple to write into; any may be None, not all four gradients.  A model with
        acceleration-source joints is refused."""
        B, dt, sfx, stream = self._device_inputs([q, qd, tau, w], layout)
        if f_ext is not None:
            self._device_tensor(f_ext, dt)
        self._check_f_ext(f_ext, B, layout)
        vec = (B, self.nv) if layout == _lib.LAYOUT_AOS else (self.nv, B)
        qdd, gq, gqd, gtau, gpi = self._outputs(out, (vec, vec, vec, vec, self._parameter_tensor(pi, B, dt, layout)),
                                                ("qdd", "gq", "gqd", "gtau", "gpi"), dt, q.device)
        if gq is None and gqd is None and gtau is None and gpi is None:
            raise _lib.MecanoHipError(1, "all four gradients are None")
        g, ra = self._root(gravity)
        opts = self._options(layout, True, True, stream, root_acceleration=ra)
        ptr = lambda t: None if t is None else t.data_ptr()
        _lib.check(getattr(_lib.load(), f"mh_aba_parameters_state_vjp_{sfx}")(
            self._h, B, q.data_ptr(), qd.data_ptr(), tau.data_ptr(), pi.data_ptr(), g, ptr(f_ext), w.data_ptr(), ctypes.byref(opts), ptr(qdd),
            ptr(gq), ptr(gqd), ptr(gtau), ptr(gpi)))
        return qdd, gq, gqd, gtau, gpi

    def regressor(self, q, qd, qdd, gravity=(0.0, 0.0, -9.81), layout=_lib.LAYOUT_AOS, consider_coriolis=True, consider_accelerations=True,
                  first_moment_columns=False):
        """Joint torque regressor (JointTorqueRegressorCalculator.compute, JointTorqueRegressorCalculator.java:173-190): Y [B, nv, 10 n_joints]
        with tau = Y pi; the ten columns of joint j's successor body start at column 10 j.  Device tensors (fp64 / fp32); ``layout`` is the
        layout of q, qd, qdd and Y (SoA: Y [nv, 10 n_joints, B]).  ``first_moment_columns``: d tau / d (m c) in columns 1..3 of every body instead of the reference's zeros."""
        import torch
        B, dt, sfx, stream = self._device_inputs([q, qd, qdd], layout)
        Y = torch.empty((B, self.nv, 10 * self.n_joints) if layout == _lib.LAYOUT_AOS else (self.nv, 10 * self.n_joints, B), dtype=dt, device=q.device)
        g, ra = self._root(gravity)
        opts = self._options(layout, consider_coriolis, consider_accelerations, stream, root_acceleration=ra)
        _lib.check(getattr(_lib.load(), f"mh_regressor_{sfx}")(self._h, B, q.data_ptr(), qd.data_ptr(), qdd.data_ptr(), g, ctypes.byref(opts),
                                                              1 if first_moment_columns else 0, Y.data_ptr()))
        return Y

    def centroidal(self, q, qd=None, frame=None, at_com=False, layout=_lib.LAYOUT_AOS):
        """Centroidal momentum matrix, convective term and frame origin (CompositeRigidBodyMassMatrixCalculator.java:375-420, 801-839):
        (A [B, 6, nv], b [B, 6] or None without qd, com [B, 3]).  ``frame``: 12 numbers (R row-major, p), pose of the centroidal momentum
        frame in the root body frame, None = the root body frame; ``at_com`` re-centres it on the centre of mass."""
        fr = None
        if frame is not None:
            fr = (ctypes.c_double * 12)(*[float(v) for v in np.asarray(frame, dtype=np.float64).reshape(12)])
        mode = _lib.CENTROIDAL_FRAME_AT_COM if at_com else _lib.CENTROIDAL_FRAME_FIXED
        if not self._is_torch(q):  # numpy: host-pointer entry point (fp64)
            q = _np(q, np.float64)
            qd = None if qd is None else _np(qd, np.float64)
            B = self._batch(q, self.nq, layout)
            aos = layout == _lib.LAYOUT_AOS
            A = np.empty((B, 6, self.nv) if aos else (6 * self.nv, B))
            b = None if qd is None else np.empty((B, 6) if aos else (6, B))
            com = np.empty((B, 3) if aos else (3, B))
            opts = self._options(layout)
            _lib.check(_lib.load().mh_centroidal_f64_host(self._h, B, q.ctypes.data, None if qd is None else qd.ctypes.data, fr, mode,
                                                          ctypes.byref(opts), A.ctypes.data, None if b is None else b.ctypes.data,
                                                          com.ctypes.data))
            return A, b, com
        import torch
        B, dt, sfx, stream = self._device_inputs([q] if qd is None else [q, qd], layout)
        aos = layout == _lib.LAYOUT_AOS
        A = torch.empty((B, 6, self.nv) if aos else (6 * self.nv, B), dtype=dt, device=q.device)
        b = None if qd is None else torch.empty((B, 6) if aos else (6, B), dtype=dt, device=q.device)
        com = torch.empty((B, 3) if aos else (3, B), dtype=dt, device=q.device)
        opts = self._options(layout, stream=stream)
        _lib.check(getattr(_lib.load(), f"mh_centroidal_{sfx}")(self._h, B, q.data_ptr(), None if qd is None else qd.data_ptr(), fr, mode,
                                                               ctypes.byref(opts), A.data_ptr(), None if b is None else b.data_ptr(),
                                                               com.data_ptr()))
        return A, b, com


def pinned_empty(shape, dtype=np.float64):
    """A numpy array in PINNED host memory (mh_host_alloc): the host-pointer entry points copy from / to it at PCIe rate, where pageable
    arrays go through the runtime's staging copies.  The memory is released when the array (and every view of it) is gone."""
    import weakref
    lib = _lib.load()
    dt = np.dtype(dtype)
    n = int(np.prod(shape)) if np.ndim(shape) else int(shape)
    ptr = ctypes.c_void_p()
    _lib.check(lib.mh_host_alloc(max(1, n * dt.itemsize), ctypes.byref(ptr)))
    buf = (ctypes.c_char * max(1, n * dt.itemsize)).from_address(ptr.value)
    arr = np.frombuffer(buf, dtype=dt, count=n).reshape(shape)
    weakref.finalize(buf, lib.mh_host_free, ctypes.c_void_p(ptr.value))
    return arr


class HipTimer:
    """HIP events recorded on the stream the kernels are launched on (bench.py, SURVEY.md section 8d timing protocol)."""

    def __init__(self):
        self._h = ctypes.c_void_p()
        _lib.check(_lib.load().mh_timer_create(ctypes.byref(self._h)))

    def start(self, stream=None):
        _lib.check(_lib.load().mh_timer_start(self._h, stream))

    def stop(self, stream=None):
        _lib.check(_lib.load().mh_timer_stop(self._h, stream))

    def elapsed_ms(self) -> float:
        ms = ctypes.c_float()
        _lib.check(_lib.load().mh_timer_elapsed_ms(self._h, ctypes.byref(ms)))
        return float(ms.value)

    def __del__(self):
        try:
            if self._h:
                _lib.load().mh_timer_destroy(self._h)
                self._h = None
        except Exception:
            pass


class HipCommunicator:
    """The C-ABI's RCCL communicator (mh_comm_*, include/mecano_hip.h): what a host without torch.distributed uses around the sharded
    compute calls -- shard_range, one broadcast of the robot description, one all-gather of the output rows.  mecano_amd/distributed.py
    does the same over torch.distributed; bench.py keeps that transport (the driver launches it under torch.distributed.run)."""

    ID_BYTES = 128

    @staticmethod
    def unique_id() -> bytes:
        buf = ctypes.create_string_buffer(HipCommunicator.ID_BYTES)
        _lib.check(_lib.load().mh_comm_unique_id(buf))
        return buf.raw

    @staticmethod
    def shard_range(B: int, rank: int, world: int):
        lo, hi = ctypes.c_int64(), ctypes.c_int64()
        _lib.check(_lib.load().mh_shard_range(B, rank, world, ctypes.byref(lo), ctypes.byref(hi)))
        return int(lo.value), int(hi.value)

    def __init__(self, unique_id: bytes, rank: int, world: int):
        if len(unique_id) != self.ID_BYTES:
            raise ValueError(f"a communicator id has {self.ID_BYTES} bytes")
        self._h = ctypes.c_void_p()
        _lib.check(_lib.load().mh_comm_create(ctypes.create_string_buffer(unique_id, self.ID_BYTES), rank, world, ctypes.byref(self._h)))
        r, w = ctypes.c_int32(), ctypes.c_int32()
        _lib.check(_lib.load().mh_comm_size(self._h, ctypes.byref(r), ctypes.byref(w)))
        self.rank, self.world = int(r.value), int(w.value)

    def broadcast_bytes(self, payload: Optional[bytes], nbytes: int, root: int = 0) -> bytes:
        """`root` passes the payload, the others None; everybody returns the same nbytes bytes."""
        buf = ctypes.create_string_buffer(payload if self.rank == root else b"", nbytes)
        _lib.check(_lib.load().mh_comm_broadcast_host(self._h, buf, nbytes, root))
        return buf.raw

    def broadcast_model_desc(self, desc, root: int = 0):
        """The robot description from `root` (the others pass None): header of two lengths, then the packed integer and real arrays."""
        from .distributed import pack_desc, unpack_desc
        if self.rank == root:
            ints, f64 = pack_desc(desc)
            head = np.array([len(ints), len(f64)], dtype=np.int64).tobytes()
        else:
            ints = f64 = None
            head = None
        ni, nf = (int(x) for x in np.frombuffer(self.broadcast_bytes(head, 16, root), dtype=np.int64))
        raw = self.broadcast_bytes(ints.tobytes() + f64.tobytes() if self.rank == root else None, 8 * (ni + nf), root)
        return unpack_desc(np.frombuffer(raw[:8 * ni], dtype=np.int64).copy(), np.frombuffer(raw[8 * ni:], dtype=np.float64).copy())

    def all_gather_rows(self, local, B_total: int, stream=None):
        """local: this rank's rows of shard_range(B_total, rank, world), a contiguous CUDA tensor [rows, ...]; returns [B_total, ...]."""
        import torch
        lo, hi = self.shard_range(B_total, self.rank, self.world)
        if local.shape[0] != hi - lo or not local.is_contiguous():
            raise ValueError(f"rank {self.rank} owns rows [{lo}, {hi}) of {B_total}: pass exactly those, contiguous")
        out = torch.empty((B_total,) + tuple(local.shape[1:]), dtype=local.dtype, device=local.device)
        row_bytes = local.element_size() * int(np.prod(local.shape[1:], dtype=np.int64))
        s = stream if stream is not None else torch.cuda.current_stream().cuda_stream
        _lib.check(_lib.load().mh_comm_all_gather_rows(self._h, local.data_ptr(), B_total, row_bytes, out.data_ptr(), s))
        return out

    def barrier(self, stream=None):
        _lib.check(_lib.load().mh_comm_barrier(self._h, stream))

    def close(self):
        if self._h:
            _lib.check(_lib.load().mh_comm_destroy(self._h))
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
