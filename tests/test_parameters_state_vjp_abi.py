"""The four state-and-parameter gradient exports in include/mecano_hip.h, mecano_amd/_lib.py, the library and the Java handles, with
the same argument lists (host only), and the refusals of their contract through the bare C-ABI (those need a model, hence a device)."""
import ctypes
import os
import re

import numpy as np
import pytest

from mecano_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "mecano_hip.h")).read()
NATIVE = open(os.path.join(ROOT, "java", "us", "ihmc", "mecano", "hip", "MecanoHipNative.java")).read()
RNEA_NAMES = ("mh_rnea_parameters_state_vjp_f64", "mh_rnea_parameters_state_vjp_f32")
ABA_NAMES = ("mh_aba_parameters_state_vjp_f64", "mh_aba_parameters_state_vjp_f32")
INVALID = 1  # MH_ERR_INVALID_ARGUMENT
GRAVITY = (0.3, -0.2, -9.81)


def header_args(name):
    text = re.sub(r"/\*.*?\*/", " ", HEADER, flags=re.S)
    m = re.search(r"mh_status\s+" + name + r"\s*\(([^;]*?)\)\s*;", text, flags=re.S)
    assert m, f"{name} is not declared"
    return [" ".join(a.split()) for a in m.group(1).split(",")]


def test_header_declares_the_exports_with_one_argument_list_per_pair():
    a64, a32 = header_args(RNEA_NAMES[0]), header_args(RNEA_NAMES[1])
    assert a64 == ["mh_model_t model", "int64_t B", "const double *q", "const double *qd", "const double *qdd", "const double *pi",
                   "const double gravity[3]", "const double *f_ext", "const double *u", "const mh_options *opts", "double *gq_out",
                   "double *gqd_out", "double *gqdd_out", "double *gpi_out"]
    assert a32 == [a if "gravity" in a else a.replace("double *", "float *") for a in a64]
    b64, b32 = header_args(ABA_NAMES[0]), header_args(ABA_NAMES[1])
    assert b64 == ["mh_model_t model", "int64_t B", "const double *q", "const double *qd", "const double *tau", "const double *pi",
                   "const double gravity[3]", "const double *f_ext", "const double *w", "const mh_options *opts", "double *qdd_out",
                   "double *gq_out", "double *gqd_out", "double *gtau_out", "double *gpi_out"]
    assert b32 == [a if "gravity" in a else a.replace("double *", "float *") for a in b64]
    assert re.search(r"MH_ABI_VERSION\s+5\b", HEADER)  # new exports only


def test_python_binding_lists_and_types_them(hip_lib):
    P, I64 = ctypes.c_void_p, ctypes.c_int64
    assert hip_lib.mh_abi_version() == 5
    for names, n, opt_at in ((RNEA_NAMES, 14, 9), (ABA_NAMES, 15, 9)):
        for name in names:
            assert name in _lib.ABI_SYMBOLS
            fn = getattr(hip_lib, name)  # (AttributeError: the library does not export it)
            assert len(fn.argtypes) == n and fn.argtypes[0] is P and fn.argtypes[1] is I64
            assert all(a is P for k, a in enumerate(fn.argtypes[2:], 2) if k != opt_at)
            assert fn.argtypes[opt_at] is not P  # the options pointer


def test_python_methods_and_autograd_functions_exist():
    from mecano_amd import autograd
    from mecano_amd.engine import HipModel
    assert callable(HipModel.rnea_parameters_state_vjp) and callable(HipModel.aba_parameters_state_vjp)
    assert callable(autograd.rnea_parameters_state) and callable(autograd.aba_parameters_state) and callable(autograd.step_parameters)


def test_null_model_is_refused_before_any_device_work(hip_lib):
    for name in RNEA_NAMES:
        assert getattr(hip_lib, name)(None, 4, *([None] * 12)) == INVALID
        assert b"model" in hip_lib.mh_last_error()
    for name in ABA_NAMES:
        assert getattr(hip_lib, name)(None, 4, *([None] * 13)) == INVALID
        assert b"model" in hip_lib.mh_last_error()


def test_java_handles_match():
    text = re.sub(r"/\*.*?\*/", " ", NATIVE, flags=re.S)
    for names, n in ((RNEA_NAMES, 14), (ABA_NAMES, 15)):
        for name in names:
            m = re.search(r'handle\(\s*"' + name + r'"\s*,\s*status\(([^)]*)\)\s*\)\s*;', text, flags=re.S)
            assert m, f"no Java handle for {name}"
            assert [k.strip() for k in m.group(1).split(",")] == ["ADDRESS", "JAVA_LONG"] + ["ADDRESS"] * (n - 2)


def test_the_kernel_header_is_built_and_hashed_with_the_library():
    from mecano_amd import build
    assert any(os.path.basename(p) == "mh_params_state_vjp_kernels.h" for p in build.LIB_HEADERS)
    assert all(os.path.exists(p) for p in build.LIB_HEADERS)


@pytest.mark.gpu
def test_argument_errors_come_back_before_any_launch(hip_lib):
    """NULL pi / cotangent, all outputs NULL, NULL states, overlapping buffers (pi with gpi_out, the cotangent with gq_out, two outputs),
    no gravity, a bad batch size, acceleration-source joints (both forms): refused, and the poisoned outputs stay untouched.  B = 0
    returns MH_OK and touches nothing."""
    import torch
    from mecano_amd import random_tools as rt
    from mecano_amd.engine import HipModel
    sys_ = rt.nextHumanoid(np.random.default_rng(11))
    desc = sys_.toModelDesc()
    hm, B, nv, n = HipModel(desc), 8, desc.nv, desc.n_joints
    q, qd, qdd, tau = (torch.tensor(x, device="cuda") for x in rt.nextState(np.random.default_rng(5), sys_, B))
    u = torch.ones_like(qd)
    pi = torch.tensor(np.broadcast_to(hm.inertial_parameters(), (B, n, 10)).copy(), device="cuda")
    g3 = (ctypes.c_double * 3)(*GRAVITY)
    opts = hm._options(0, stream=torch.cuda.current_stream().cuda_stream)
    o = ctypes.byref(opts)
    nan = lambda *s: torch.full(s, float("nan"), dtype=torch.float64, device="cuda")
    a, b, c, d, gp = nan(B, nv), nan(B, nv), nan(B, nv), nan(B, nv), nan(B, n, 10)
    p = lambda x: x.data_ptr()
    rnea, aba = hip_lib.mh_rnea_parameters_state_vjp_f64, hip_lib.mh_aba_parameters_state_vjp_f64
    for fn in (rnea, hip_lib.mh_rnea_parameters_state_vjp_f32):
        assert fn(hm._h, B, p(q), p(qd), p(qdd), None, g3, None, p(u), o, p(a), p(b), p(c), p(gp)) == INVALID      # NULL pi
        assert fn(hm._h, B, p(q), p(qd), p(qdd), p(pi), g3, None, None, o, p(a), p(b), p(c), p(gp)) == INVALID     # NULL u
        assert fn(hm._h, B, p(q), p(qd), p(qdd), p(pi), g3, None, p(u), o, None, None, None, None) == INVALID      # every output NULL
    assert rnea(hm._h, B, None, p(qd), p(qdd), p(pi), g3, None, p(u), o, p(a), p(b), p(c), p(gp)) == INVALID       # NULL states
    assert rnea(hm._h, B, p(q), None, p(qdd), p(pi), g3, None, p(u), o, p(a), p(b), p(c), p(gp)) == INVALID
    assert rnea(hm._h, B, p(q), p(qd), None, p(pi), g3, None, p(u), o, p(a), p(b), p(c), p(gp)) == INVALID
    assert rnea(hm._h, B, p(q), p(qd), p(qdd), p(pi), None, None, p(u), o, p(a), p(b), p(c), p(gp)) == INVALID     # no gravity, no root acceleration
    assert rnea(hm._h, B, p(q), p(qd), p(qdd), p(pi), g3, None, p(u), o, p(a), p(b), p(c), p(pi)) == INVALID       # pi with gpi_out
    assert rnea(hm._h, B, p(q), p(qd), p(qdd), p(pi), g3, None, p(u), o, p(u), p(b), p(c), p(gp)) == INVALID       # u with gq_out
    assert rnea(hm._h, B, p(q), p(qd), p(qdd), p(pi), g3, None, p(u), o, p(a), p(a), p(c), p(gp)) == INVALID       # two outputs
    assert rnea(hm._h, -1, p(q), p(qd), p(qdd), p(pi), g3, None, p(u), o, p(a), p(b), p(c), p(gp)) == 2            # MH_ERR_BAD_DIMENSION
    for fn in (aba, hip_lib.mh_aba_parameters_state_vjp_f32):
        assert fn(hm._h, B, p(q), p(qd), p(tau), None, g3, None, p(u), o, p(a), p(b), p(c), p(d), p(gp)) == INVALID
        assert fn(hm._h, B, p(q), p(qd), p(tau), p(pi), g3, None, None, o, p(a), p(b), p(c), p(d), p(gp)) == INVALID
        assert fn(hm._h, B, p(q), p(qd), p(tau), p(pi), g3, None, p(u), o, p(a), None, None, None, None) == INVALID  # qdd_out alone
    assert aba(hm._h, B, None, p(qd), p(tau), p(pi), g3, None, p(u), o, p(a), p(b), p(c), p(d), p(gp)) == INVALID
    assert aba(hm._h, B, p(q), p(qd), p(tau), p(pi), None, None, p(u), o, p(a), p(b), p(c), p(d), p(gp)) == INVALID
    assert aba(hm._h, B, p(q), p(qd), p(tau), p(pi), g3, None, p(u), o, p(a), p(a), p(c), p(d), p(gp)) == INVALID    # two outputs overlap
    assert aba(hm._h, B, p(q), p(qd), p(tau), p(pi), g3, None, p(u), o, p(tau), p(b), p(c), p(d), p(gp)) == INVALID  # an output on an input
    assert aba(hm._h, B, p(q), p(qd), p(tau), p(pi), g3, None, p(u), o, p(a), p(u), p(c), p(d), p(gp)) == INVALID    # w with gq_out
    assert aba(hm._h, B, p(q), p(qd), p(tau), p(pi), g3, None, p(u), o, p(a), p(b), p(c), p(d), p(pi)) == INVALID    # pi with gpi_out
    assert rnea(hm._h, 0, None, None, None, p(pi), g3, None, p(u), o, p(a), p(b), p(c), p(gp)) == 0                  # B = 0: MH_OK, nothing touched
    assert aba(hm._h, 0, None, None, None, p(pi), g3, None, p(u), o, p(a), p(b), p(c), p(d), p(gp)) == 0
    modes = [0] * n
    modes[3] = 1
    hm.set_joint_source_modes(modes)
    assert rnea(hm._h, B, p(q), p(qd), p(qdd), p(pi), g3, None, p(u), o, p(a), p(b), p(c), p(gp)) == INVALID         # acceleration sources
    assert aba(hm._h, B, p(q), p(qd), p(tau), p(pi), g3, None, p(u), o, p(a), p(b), p(c), p(d), p(gp)) == INVALID
    hm.set_joint_source_modes(None)
    torch.cuda.synchronize()
    for x in (a, b, c, d, gp):
        assert torch.isnan(x).all()
    assert rnea(hm._h, B, p(q), p(qd), p(qdd), p(pi), g3, None, p(u), o, p(a), p(b), p(c), p(gp)) == 0
    ref = hm.rnea_parameters_state_vjp(q, qd, qdd, pi, u, GRAVITY)
    torch.cuda.synchronize()
    assert all(torch.equal(x, y) and torch.isfinite(x).all() for x, y in zip((a, b, c, gp), ref))
