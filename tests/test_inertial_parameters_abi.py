"""The five inertial-parameter exports in include/mecano_hip.h, mecano_amd/_lib.py, the library and the Java handles, with the same
argument lists (host only), and their refusals through the bare C-ABI.

mh_model_inertial_parameters itself touches no device, but it takes a model handle, and mh_model_create gives none without a device
(MH_ERR_NO_DEVICE: tests/test_abi.py pins that): its comparison with the description's fields is therefore marked gpu."""
import ctypes
import os
import re

import numpy as np
import pytest

from mecano_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "mecano_hip.h")).read()
NATIVE = open(os.path.join(ROOT, "java", "us", "ihmc", "mecano", "hip", "MecanoHipNative.java")).read()
RNEA_NAMES = ("mh_rnea_parameters_f64", "mh_rnea_parameters_f32")
ABA_NAMES = ("mh_aba_parameters_f64", "mh_aba_parameters_f32")
INVALID = 1  # MH_ERR_INVALID_ARGUMENT


def header_args(name):
    text = re.sub(r"/\*.*?\*/", " ", HEADER, flags=re.S)
    m = re.search(r"mh_status\s+" + name + r"\s*\(([^;]*?)\)\s*;", text, flags=re.S)
    assert m, f"{name} is not declared"
    return [" ".join(a.split()) for a in m.group(1).split(",")]


def test_header_declares_the_exports_with_one_argument_list_per_pair():
    assert header_args("mh_model_inertial_parameters") == ["mh_model_t model", "double *pi_out"]
    a64, a32 = header_args(RNEA_NAMES[0]), header_args(RNEA_NAMES[1])
    assert a64 == ["mh_model_t model", "int64_t B", "const double *q", "const double *qd", "const double *qdd", "const double *pi",
                   "const double gravity[3]", "const double *f_ext", "const mh_options *opts", "double *tau_out"]
    assert a32 == [a if "gravity" in a else a.replace("double *", "float *") for a in a64]
    b64, b32 = header_args(ABA_NAMES[0]), header_args(ABA_NAMES[1])
    assert b64 == [a.replace("*qdd", "*tau").replace("*tau_out", "*qdd_out") if a in ("const double *qdd", "double *tau_out") else a for a in a64]
    assert b32 == [a if "gravity" in a else a.replace("double *", "float *") for a in b64]
    assert re.search(r"MH_ABI_VERSION\s+5\b", HEADER)  # new exports only


def test_python_binding_lists_and_types_them(hip_lib):
    P, I64 = ctypes.c_void_p, ctypes.c_int64
    assert hip_lib.mh_abi_version() == 5
    assert "mh_model_inertial_parameters" in _lib.ABI_SYMBOLS and hip_lib.mh_model_inertial_parameters.argtypes == [P, P]
    for name in RNEA_NAMES + ABA_NAMES:
        assert name in _lib.ABI_SYMBOLS
        fn = getattr(hip_lib, name)  # (AttributeError: the library does not export it)
        assert len(fn.argtypes) == 10 and fn.argtypes[0] is P and fn.argtypes[1] is I64
        assert all(a is P for a in fn.argtypes[2:8]) and fn.argtypes[9] is P


def test_java_handles_match():
    text = re.sub(r"/\*.*?\*/", " ", NATIVE, flags=re.S)
    m = re.search(r'handle\(\s*"mh_model_inertial_parameters"\s*,\s*status\(([^)]*)\)\s*\)\s*;', text, flags=re.S)
    assert m and [k.strip() for k in m.group(1).split(",")] == ["ADDRESS", "ADDRESS"]
    for name in RNEA_NAMES + ABA_NAMES:
        m = re.search(r'handle\(\s*"' + name + r'"\s*,\s*status\(([^)]*)\)\s*\)\s*;', text, flags=re.S)
        assert m, f"no Java handle for {name}"
        assert [k.strip() for k in m.group(1).split(",")] == ["ADDRESS", "JAVA_LONG"] + ["ADDRESS"] * 8


def test_null_model_is_refused_before_any_device_work(hip_lib):
    buf = np.zeros(10)
    assert hip_lib.mh_model_inertial_parameters(None, buf.ctypes.data) == INVALID
    assert b"model" in hip_lib.mh_last_error()
    for name in RNEA_NAMES + ABA_NAMES:
        assert getattr(hip_lib, name)(None, 4, None, None, None, None, None, None, None, None) == INVALID
        assert b"model" in hip_lib.mh_last_error()


def committed_models():
    from mecano_amd.build import registered_models
    return registered_models()


@pytest.mark.gpu
def test_model_parameters_equal_the_descriptions_fields(hip_lib):
    """Every model the build registers: the ten numbers per joint are inertia_mass, inertia_com and the symmetric part of inertia_J, in
    the description's joint order (OracleModel.parameter_vector's); a NULL output is refused."""
    from mecano_amd.engine import HipModel
    from oracle.cpu_oracle import OracleModel
    for name, desc in committed_models().items():
        hm = HipModel(desc)
        pi = hm.inertial_parameters()
        n = desc.n_joints
        J = np.asarray(desc.inertia_J, dtype=np.float64).reshape(n, 3, 3)
        assert pi.shape == (n, 10), name
        assert np.array_equal(pi[:, 0], np.asarray(desc.inertia_mass, dtype=np.float64)), name
        assert np.array_equal(pi[:, 1:4], np.asarray(desc.inertia_com, dtype=np.float64).reshape(n, 3)), name
        for c, (a, b) in enumerate(((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))):
            assert np.array_equal(pi[:, 4 + c], 0.5 * (J[:, a, b] + J[:, b, a])), name
        if np.array_equal(J, J.transpose(0, 2, 1)):
            assert np.array_equal(pi.reshape(-1), OracleModel(desc).parameter_vector()), name
        assert hip_lib.mh_model_inertial_parameters(hm._h, None) == INVALID
        hm.close()
