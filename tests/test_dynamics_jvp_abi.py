"""The eight forward-mode exports in include/mecano_hip.h, mecano_amd/_lib.py, the library and the Java handles, with the same argument
lists (host only), and the argument errors of their contract through the bare C-ABI (those need a model, hence a device)."""
import ctypes
import os
import re

import numpy as np
import pytest

from mecano_amd import _lib
from mecano_amd import build as mbuild

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "mecano_hip.h")).read()
NATIVE = open(os.path.join(ROOT, "java", "us", "ihmc", "mecano", "hip", "MecanoHipNative.java")).read()
INVALID = 1  # MH_ERR_INVALID_ARGUMENT
GRAVITY = (0.3, -0.2, -9.81)
STATE = ["const double *q", "const double *qd"]
HEAD = ["mh_model_t model", "int64_t B"]
WORLD = ["const double gravity[3]", "const double *f_ext"]
# name -> (fp64 argument list, index of dt or None)
EXPORTS = {
    "mh_rnea_jvp": (HEAD + STATE + ["const double *qdd"] + WORLD + ["const double *dq", "const double *dqd", "const double *dqdd", "const mh_options *opts",
                                                                     "double *dtau_out"], None),
    "mh_aba_jvp": (HEAD + STATE + ["const double *tau"] + WORLD + ["const double *dq", "const double *dqd", "const double *dtau", "const mh_options *opts",
                                                                    "double *qdd_out", "double *dqdd_out"], None),
    "mh_integrate_jvp": (HEAD + ["double dt", "const double *qd", "const double *qdd", "const double *dq", "const double *dqd", "const double *dqdd",
                                 "const mh_options *opts", "double *dq_next_out", "double *dqd_next_out"], 2),
    "mh_aba_integrate_jvp": (HEAD + ["double dt"] + STATE + ["const double *tau"] + WORLD + ["const double *dq", "const double *dqd", "const double *dtau",
                                                                                               "const mh_options *opts", "double *qdd_out", "double *dqdd_out",
                                                                                               "double *dq_next_out", "double *dqd_next_out"], 2),
}


def header_args(name):
    text = re.sub(r"/\*.*?\*/", " ", HEADER, flags=re.S)
    m = re.search(r"mh_status\s+" + name + r"\s*\(([^;]*?)\)\s*;", text, flags=re.S)
    assert m, f"{name} is not declared"
    return [" ".join(a.split()) for a in m.group(1).split(",")]


def test_header_declares_the_exports_with_one_argument_list_per_pair():
    for name, (want, _) in EXPORTS.items():
        a64, a32 = header_args(name + "_f64"), header_args(name + "_f32")
        assert a64 == want, name
        assert a32 == [a if "gravity" in a else a.replace("double *", "float *") for a in a64], name
    assert re.search(r"MH_ABI_VERSION\s+5\b", HEADER)  # new exports only


def test_python_binding_lists_and_types_them(hip_lib):
    P, I64 = ctypes.c_void_p, ctypes.c_int64
    assert hip_lib.mh_abi_version() == 5
    for name, (want, dt_at) in EXPORTS.items():
        for sfx in ("_f64", "_f32"):
            assert name + sfx in _lib.ABI_SYMBOLS
            fn = getattr(hip_lib, name + sfx)  # (AttributeError: the library does not export it)
            assert len(fn.argtypes) == len(want) and fn.argtypes[0] is P and fn.argtypes[1] is I64
            opt_at = want.index("const mh_options *opts")
            for k, a in enumerate(fn.argtypes[2:], start=2):
                assert (a is ctypes.c_double) if k == dt_at else (a is P or k == opt_at), (name, k)


def test_the_new_header_is_hashed_with_the_library():
    assert any(os.path.basename(h) == "mh_rnea_jvp_kernels.h" and os.path.exists(h) for h in mbuild.LIB_HEADERS)


def test_null_model_is_refused_before_any_device_work(hip_lib):
    for name, (want, dt_at) in EXPORTS.items():
        for sfx in ("_f64", "_f32"):
            args = [0.01 if k == dt_at else None for k in range(2, len(want))]
            assert getattr(hip_lib, name + sfx)(None, 4, *args) == INVALID
            assert hip_lib.mh_last_error()


def test_java_handles_match():
    text = re.sub(r"/\*.*?\*/", " ", NATIVE, flags=re.S)
    for name, (want, dt_at) in EXPORTS.items():
        for sfx in ("_f64", "_f32"):
            m = re.search(r'handle\(\s*"' + name + sfx + r'"\s*,\s*status\(([^)]*)\)\s*\)\s*;', text, flags=re.S)
            assert m, f"no Java handle for {name + sfx}"
            kinds = ["ADDRESS", "JAVA_LONG"] + ["JAVA_DOUBLE" if k == dt_at else "ADDRESS" for k in range(2, len(want))]
            assert [k.strip() for k in m.group(1).split(",")] == kinds


@pytest.mark.gpu
def test_argument_errors_come_back_before_any_launch(hip_lib):
    """No output, no direction, overlapping buffers, NULL states, no gravity, a dt that is not finite, acceleration-source joints:
    MH_ERR_INVALID_ARGUMENT, and the poisoned outputs stay untouched.  B = 0 returns MH_OK and touches nothing."""
    import torch
    from mecano_amd import random_tools as rt
    from mecano_amd.engine import HipModel
    sys_ = rt.nextHumanoid(np.random.default_rng(11))
    desc = sys_.toModelDesc()
    hm, B, nv = HipModel(desc), 8, desc.nv
    q, qd, qdd, tau = (torch.tensor(x, device="cuda") for x in rt.nextState(np.random.default_rng(5), sys_, B))
    d1, d2, d3 = (torch.full_like(qd, v) for v in (1.0, 0.5, -0.25))
    g3 = (ctypes.c_double * 3)(*GRAVITY)
    opts = hm._options(0, stream=torch.cuda.current_stream().cuda_stream)
    o = ctypes.byref(opts)
    nan = lambda *s: torch.full(s, float("nan"), dtype=torch.float64, device="cuda")
    a, b, c, d = nan(B, nv), nan(B, nv), nan(B, nv), nan(B, nv)
    big = nan(2 * B * nv)
    p = lambda x: x.data_ptr()
    rnea, aba, integ, step = hip_lib.mh_rnea_jvp_f64, hip_lib.mh_aba_jvp_f64, hip_lib.mh_integrate_jvp_f64, hip_lib.mh_aba_integrate_jvp_f64
    S, D = (p(q), p(qd)), (p(d1), p(d2), p(d3))
    assert rnea(hm._h, B, *S, p(qdd), g3, None, *D, o, None) == INVALID                       # no output
    assert hip_lib.mh_rnea_jvp_f32(hm._h, B, *S, p(qdd), g3, None, *D, o, None) == INVALID
    assert rnea(hm._h, B, *S, p(qdd), g3, None, None, None, None, o, p(a)) == INVALID         # no direction
    assert rnea(hm._h, B, *S, p(qdd), g3, None, *D, o, p(d2)) == INVALID                      # the output on a direction, on a state
    assert rnea(hm._h, B, *S, p(qdd), g3, None, *D, o, p(qd)) == INVALID
    assert rnea(hm._h, B, None, p(qd), p(qdd), g3, None, *D, o, p(a)) == INVALID              # NULL states
    assert rnea(hm._h, B, p(q), None, p(qdd), g3, None, *D, o, p(a)) == INVALID
    assert rnea(hm._h, B, p(q), p(qd), None, g3, None, *D, o, p(a)) == INVALID
    assert rnea(hm._h, B, *S, p(qdd), None, None, *D, o, p(a)) == INVALID                     # no gravity, no root acceleration
    assert aba(hm._h, B, *S, p(tau), g3, None, *D, o, p(a), None) == INVALID                  # dqdd_out is needed
    assert aba(hm._h, B, *S, p(tau), g3, None, None, None, None, o, p(a), p(b)) == INVALID
    assert aba(hm._h, B, *S, p(tau), g3, None, *D, o, p(a), p(a)) == INVALID                  # outputs overlap
    assert aba(hm._h, B, *S, p(tau), g3, None, *D, o, p(big), p(big) + 8 * nv) == INVALID
    assert aba(hm._h, B, *S, p(tau), g3, None, *D, o, p(a), p(d3)) == INVALID
    assert aba(hm._h, B, *S, p(tau), g3, None, *D, o, p(tau), p(b)) == INVALID
    assert aba(hm._h, B, *S, None, g3, None, *D, o, p(a), p(b)) == INVALID
    assert aba(hm._h, B, *S, p(tau), None, None, *D, o, p(a), p(b)) == INVALID
    assert integ(hm._h, B, 0.01, p(qd), p(qdd), *D, o, None, None) == INVALID
    assert integ(hm._h, B, 0.01, p(qd), p(qdd), None, None, None, o, p(a), p(b)) == INVALID
    assert integ(hm._h, B, float("inf"), p(qd), p(qdd), *D, o, p(a), p(b)) == INVALID
    assert integ(hm._h, B, float("nan"), p(qd), p(qdd), *D, o, p(a), p(b)) == INVALID
    assert integ(hm._h, B, 0.01, p(qd), p(qdd), *D, o, p(a), p(a)) == INVALID
    assert integ(hm._h, B, 0.01, p(qd), p(qdd), *D, o, p(a), p(d1)) == INVALID
    assert integ(hm._h, B, 0.01, None, p(qdd), *D, o, p(a), p(b)) == INVALID
    assert step(hm._h, B, 0.01, *S, p(tau), g3, None, *D, o, p(a), None, None, None) == INVALID   # qdd_out alone is no tangent
    assert step(hm._h, B, 0.01, *S, p(tau), g3, None, None, None, None, o, p(a), p(b), p(c), p(d)) == INVALID
    assert step(hm._h, B, float("-inf"), *S, p(tau), g3, None, *D, o, p(a), p(b), p(c), p(d)) == INVALID
    assert step(hm._h, B, 0.01, *S, p(tau), g3, None, *D, o, p(a), p(b), p(c), p(b)) == INVALID
    assert step(hm._h, B, 0.01, *S, p(tau), g3, None, *D, o, p(a), p(b), p(d2), p(d)) == INVALID
    assert step(hm._h, B, 0.01, *S, p(tau), None, None, *D, o, p(a), p(b), p(c), p(d)) == INVALID
    assert rnea(hm._h, 0, None, None, None, g3, None, *D, o, p(a)) == 0                       # B = 0: MH_OK, nothing touched
    assert aba(hm._h, 0, None, None, None, g3, None, *D, o, p(a), p(b)) == 0
    assert integ(hm._h, 0, 0.01, None, None, *D, o, p(a), p(b)) == 0
    assert step(hm._h, 0, 0.01, None, None, None, g3, None, *D, o, p(a), p(b), p(c), p(d)) == 0
    modes = [0] * desc.n_joints
    modes[3] = 1
    hm.set_joint_source_modes(modes)
    assert rnea(hm._h, B, *S, p(qdd), g3, None, *D, o, p(a)) == INVALID                       # acceleration sources
    assert aba(hm._h, B, *S, p(tau), g3, None, *D, o, p(a), p(b)) == INVALID
    assert step(hm._h, B, 0.01, *S, p(tau), g3, None, *D, o, p(a), p(b), p(c), p(d)) == INVALID
    with pytest.raises(_lib.MecanoHipError):
        hm.aba_jvp(q, qd, tau, d1, d2, d3, GRAVITY)
    torch.cuda.synchronize()
    for x in (a, b, c, d, big):
        assert torch.isnan(x).all()
    hm.set_joint_source_modes(None)
    assert rnea(hm._h, B, *S, p(qdd), g3, None, *D, o, p(a)) == 0
    ref = hm.rnea_jvp(q, qd, qdd, d1, d2, d3, GRAVITY)
    torch.cuda.synchronize()
    assert torch.equal(a, ref)
