"""The six exports of the step linearisation in include/mecano_hip.h, mecano_amd/_lib.py, the library and the Java handles, with the same
argument lists (host only), and what the bare C-ABI decides before it looks for a device.

A model handle exists only with a device (mh_model_create reports MH_ERR_NO_DEVICE without one: tests/test_abi.py pins that), so on a
host without one the only call that can be made is the one with a NULL model, which every export refuses as MH_ERR_INVALID_ARGUMENT
before any device work; the NULL, aliasing and dt refusals that need a handle's sizes are exercised by tests/test_gpu_step_derivatives.py
through the same entry points."""
import ctypes
import os
import re

from mecano_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "mecano_hip.h")).read()
NATIVE = open(os.path.join(ROOT, "java", "us", "ihmc", "mecano", "hip", "MecanoHipNative.java")).read()
ADD = ("mh_configuration_add_f64", "mh_configuration_add_f32")
DIFF = ("mh_configuration_difference_f64", "mh_configuration_difference_f32")
STEP = ("mh_aba_integrate_derivatives_f64", "mh_aba_integrate_derivatives_f32")
INVALID = 1  # MH_ERR_INVALID_ARGUMENT


def header_args(name):
    text = re.sub(r"/\*.*?\*/", " ", HEADER, flags=re.S)
    m = re.search(r"mh_status\s+" + name + r"\s*\(([^;]*?)\)\s*;", text, flags=re.S)
    assert m, f"{name} is not declared"
    return [" ".join(a.split()) for a in m.group(1).split(",")]


def as_f32(args):
    return [a if "gravity" in a or a == "double dt" else a.replace("double *", "float *") for a in args]


def test_header_declares_the_exports_with_one_argument_list_per_pair():
    a = header_args(ADD[0])
    assert a == ["mh_model_t model", "int64_t B", "const double *q", "const double *dq", "const mh_options *opts", "double *q_out"]
    assert header_args(ADD[1]) == as_f32(a)
    d = header_args(DIFF[0])
    assert d == ["mh_model_t model", "int64_t B", "const double *q0", "const double *q1", "const mh_options *opts", "double *dq_out"]
    assert header_args(DIFF[1]) == as_f32(d)
    s = header_args(STEP[0])
    assert s == ["mh_model_t model", "int64_t B", "double dt", "const double *q", "const double *qd", "const double *tau",
                 "const double gravity[3]", "const double *f_ext", "const mh_options *opts", "double *qdd_out", "double *q_next",
                 "double *qd_next", "double *A_out", "double *B_out"]
    assert header_args(STEP[1]) == as_f32(s)
    assert re.search(r"MH_ABI_VERSION\s+5\b", HEADER)  # new exports only


def test_python_binding_lists_and_types_them(hip_lib):
    P, I64 = ctypes.c_void_p, ctypes.c_int64
    assert hip_lib.mh_abi_version() == 5
    for name in ADD + DIFF:
        assert name in _lib.ABI_SYMBOLS
        fn = getattr(hip_lib, name)  # (AttributeError: the library does not export it)
        assert len(fn.argtypes) == len(header_args(name)) == 6
        assert fn.argtypes[0] is P and fn.argtypes[1] is I64 and fn.argtypes[2] is P and fn.argtypes[3] is P and fn.argtypes[5] is P
    for name in STEP:
        assert name in _lib.ABI_SYMBOLS
        fn = getattr(hip_lib, name)
        assert len(fn.argtypes) == len(header_args(name)) == 14
        assert fn.argtypes[0] is P and fn.argtypes[1] is I64 and fn.argtypes[2] is ctypes.c_double
        assert all(a is P for a in fn.argtypes[3:8]) and all(a is P for a in fn.argtypes[9:])


def test_java_handles_match():
    text = re.sub(r"/\*.*?\*/", " ", NATIVE, flags=re.S)
    for names, want in ((ADD + DIFF, ["ADDRESS", "JAVA_LONG"] + ["ADDRESS"] * 4), (STEP, ["ADDRESS", "JAVA_LONG", "JAVA_DOUBLE"] + ["ADDRESS"] * 11)):
        for name in names:
            m = re.search(r'handle\(\s*"' + name + r'"\s*,\s*status\(([^)]*)\)\s*\)\s*;', text, flags=re.S)
            assert m, f"no Java handle for {name}"
            assert [k.strip() for k in m.group(1).split(",")] == want


def test_null_model_is_refused_before_any_device_work(hip_lib):
    for name in ADD + DIFF:
        assert getattr(hip_lib, name)(None, 4, None, None, None, None) == INVALID
        assert b"model" in hip_lib.mh_last_error()
    for name in STEP:
        assert getattr(hip_lib, name)(None, 4, 0.01, None, None, None, None, None, None, None, None, None, None, None) == INVALID
        assert b"model" in hip_lib.mh_last_error()
