"""The four reverse-mode gradient exports in include/mecano_hip.h, mecano_amd/_lib.py, the library and the Java handles, with the same
argument lists (host only), and the argument errors of their contract through the bare C-ABI (those need a model, hence a device)."""
import ctypes
import os
import re

import numpy as np
import pytest

from mecano_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "mecano_hip.h")).read()
NATIVE = open(os.path.join(ROOT, "java", "us", "ihmc", "mecano", "hip", "MecanoHipNative.java")).read()
RNEA_NAMES = ("mh_rnea_vjp_f64", "mh_rnea_vjp_f32")
ABA_NAMES = ("mh_aba_vjp_f64", "mh_aba_vjp_f32")
INVALID = 1  # MH_ERR_INVALID_ARGUMENT
GRAVITY = (0.3, -0.2, -9.81)


def header_args(name):
    text = re.sub(r"/\*.*?\*/", " ", HEADER, flags=re.S)
    m = re.search(r"mh_status\s+" + name + r"\s*\(([^;]*?)\)\s*;", text, flags=re.S)
    assert m, f"{name} is not declared"
    return [" ".join(a.split()) for a in m.group(1).split(",")]


def test_header_declares_the_exports_with_one_argument_list_per_pair():
    a64, a32 = header_args(RNEA_NAMES[0]), header_args(RNEA_NAMES[1])
    assert a64 == ["mh_model_t model", "int64_t B", "const double *q", "const double *qd", "const double *qdd", "const double gravity[3]",
                   "const double *f_ext", "const double *u", "const mh_options *opts", "double *gq_out", "double *gqd_out", "double *gqdd_out"]
    assert a32 == [a if "gravity" in a else a.replace("double *", "float *") for a in a64]
    b64, b32 = header_args(ABA_NAMES[0]), header_args(ABA_NAMES[1])
    assert b64 == ["mh_model_t model", "int64_t B", "const double *q", "const double *qd", "const double *tau", "const double gravity[3]",
                   "const double *f_ext", "const double *w", "const mh_options *opts", "double *qdd_out", "double *gq_out", "double *gqd_out",
                   "double *gtau_out"]
    assert b32 == [a if "gravity" in a else a.replace("double *", "float *") for a in b64]
    assert re.search(r"MH_ABI_VERSION\s+5\b", HEADER)  # new exports only


def test_python_binding_lists_and_types_them(hip_lib):
    P, I64 = ctypes.c_void_p, ctypes.c_int64
    assert hip_lib.mh_abi_version() == 5
    for names, n in ((RNEA_NAMES, 12), (ABA_NAMES, 13)):
        for name in names:
            assert name in _lib.ABI_SYMBOLS
            fn = getattr(hip_lib, name)  # (AttributeError: the library does not export it)
            assert len(fn.argtypes) == n and fn.argtypes[0] is P and fn.argtypes[1] is I64 and all(a is P for a in fn.argtypes[2:8])
            assert all(a is P for a in fn.argtypes[9:])


def test_null_model_is_refused_before_any_device_work(hip_lib):
    for name in RNEA_NAMES:
        assert getattr(hip_lib, name)(None, 4, *([None] * 10)) == INVALID
        assert hip_lib.mh_last_error()
    for name in ABA_NAMES:
        assert getattr(hip_lib, name)(None, 4, *([None] * 11)) == INVALID


def test_java_handles_match():
    text = re.sub(r"/\*.*?\*/", " ", NATIVE, flags=re.S)
    for names, n in ((RNEA_NAMES, 12), (ABA_NAMES, 13)):
        for name in names:
            m = re.search(r'handle\(\s*"' + name + r'"\s*,\s*status\(([^)]*)\)\s*\)\s*;', text, flags=re.S)
            assert m, f"no Java handle for {name}"
            assert [k.strip() for k in m.group(1).split(",")] == ["ADDRESS", "JAVA_LONG"] + ["ADDRESS"] * (n - 2)


@pytest.mark.gpu
def test_argument_errors_come_back_before_any_launch(hip_lib):
    """Every output NULL, overlapping buffers, NULL states and cotangents, acceleration-source joints: MH_ERR_INVALID_ARGUMENT, and the
    poisoned outputs stay untouched.  B = 0 returns MH_OK and touches nothing."""
    import torch
    from mecano_amd import random_tools as rt
    from mecano_amd.engine import HipModel
    sys_ = rt.nextHumanoid(np.random.default_rng(11))
    desc = sys_.toModelDesc()
    hm, B, nv = HipModel(desc), 8, desc.nv
    q, qd, qdd, tau = (torch.tensor(x, device="cuda") for x in rt.nextState(np.random.default_rng(5), sys_, B))
    u = torch.ones_like(qd)
    g3 = (ctypes.c_double * 3)(*GRAVITY)
    opts = hm._options(0, stream=torch.cuda.current_stream().cuda_stream)
    o = ctypes.byref(opts)
    nan = lambda *s: torch.full(s, float("nan"), dtype=torch.float64, device="cuda")
    a, b, c, d = nan(B, nv), nan(B, nv), nan(B, nv), nan(B, nv)
    big = nan(2 * B * nv)
    p = lambda x: x.data_ptr()
    rnea, aba = hip_lib.mh_rnea_vjp_f64, hip_lib.mh_aba_vjp_f64
    assert rnea(hm._h, B, p(q), p(qd), p(qdd), g3, None, p(u), o, None, None, None) == INVALID      # every output NULL
    assert hip_lib.mh_rnea_vjp_f32(hm._h, B, p(q), p(qd), p(qdd), g3, None, p(u), o, None, None, None) == INVALID
    assert rnea(hm._h, B, p(q), p(qd), p(qdd), g3, None, p(u), o, p(a), p(a), p(c)) == INVALID      # outputs overlap
    assert rnea(hm._h, B, p(q), p(qd), p(qdd), g3, None, p(u), o, p(big), p(big) + 8 * nv, None) == INVALID
    assert rnea(hm._h, B, p(q), p(qd), p(qdd), g3, None, p(u), o, p(a), p(b), p(u)) == INVALID      # an output overlaps an input
    assert rnea(hm._h, B, p(q), p(qd), p(qdd), g3, None, p(u), o, p(qd), p(b), p(c)) == INVALID
    assert rnea(hm._h, B, None, p(qd), p(qdd), g3, None, p(u), o, p(a), p(b), p(c)) == INVALID      # NULL states / cotangent
    assert rnea(hm._h, B, p(q), None, p(qdd), g3, None, p(u), o, p(a), p(b), p(c)) == INVALID
    assert rnea(hm._h, B, p(q), p(qd), None, g3, None, p(u), o, p(a), p(b), p(c)) == INVALID
    assert rnea(hm._h, B, p(q), p(qd), p(qdd), g3, None, None, o, p(a), p(b), p(c)) == INVALID
    assert rnea(hm._h, B, p(q), p(qd), p(qdd), None, None, p(u), o, p(a), p(b), p(c)) == INVALID    # no gravity, no root acceleration
    assert aba(hm._h, B, p(q), p(qd), p(tau), g3, None, p(u), o, p(a), None, None, None) == INVALID
    assert aba(hm._h, B, p(q), p(qd), p(tau), g3, None, p(u), o, p(a), p(b), p(b), p(d)) == INVALID
    assert aba(hm._h, B, p(q), p(qd), p(tau), g3, None, p(u), o, p(tau), p(b), p(c), p(d)) == INVALID
    assert aba(hm._h, B, p(q), p(qd), p(tau), g3, None, p(u), o, p(a), p(b), p(c), p(u)) == INVALID
    assert aba(hm._h, B, p(q), p(qd), p(tau), g3, None, None, o, p(a), p(b), p(c), p(d)) == INVALID
    assert rnea(hm._h, 0, None, None, None, g3, None, None, o, p(a), p(b), p(c)) == 0                # B = 0: MH_OK, nothing touched
    assert aba(hm._h, 0, None, None, None, g3, None, None, o, p(a), p(b), p(c), p(d)) == 0
    modes = [0] * desc.n_joints
    modes[3] = 1
    hm.set_joint_source_modes(modes)
    assert rnea(hm._h, B, p(q), p(qd), p(qdd), g3, None, p(u), o, p(a), p(b), p(c)) == INVALID      # acceleration sources
    assert aba(hm._h, B, p(q), p(qd), p(tau), g3, None, p(u), o, p(a), p(b), p(c), p(d)) == INVALID
    with pytest.raises(_lib.MecanoHipError):
        hm.aba_vjp(q, qd, tau, u, GRAVITY)
    torch.cuda.synchronize()
    for x in (a, b, c, d, big):
        assert torch.isnan(x).all()
    hm.set_joint_source_modes(None)
    assert rnea(hm._h, B, p(q), p(qd), p(qdd), g3, None, p(u), o, p(a), p(b), p(c)) == 0
    ref = hm.rnea_vjp(q, qd, qdd, u, GRAVITY)
    torch.cuda.synchronize()
    assert all(torch.equal(x, y) for x, y in zip((a, b, c), ref))
