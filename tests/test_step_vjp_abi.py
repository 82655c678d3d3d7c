"""The four exports of the step's reverse mode in include/mecano_hip.h, mecano_amd/_lib.py, the library and the Java handles, with the
same argument lists (host only)."""
import ctypes
import os
import re

from mecano_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "mecano_hip.h")).read()
NATIVE = open(os.path.join(ROOT, "java", "us", "ihmc", "mecano", "hip", "MecanoHipNative.java")).read()
INT_NAMES = ("mh_integrate_vjp_f64", "mh_integrate_vjp_f32")
STEP_NAMES = ("mh_aba_integrate_vjp_f64", "mh_aba_integrate_vjp_f32")
INVALID = 1  # MH_ERR_INVALID_ARGUMENT


def header_args(name):
    text = re.sub(r"/\*.*?\*/", " ", HEADER, flags=re.S)
    m = re.search(r"mh_status\s+" + name + r"\s*\(([^;]*?)\)\s*;", text, flags=re.S)
    assert m, f"{name} is not declared"
    return [" ".join(a.split()) for a in m.group(1).split(",")]


def test_header_declares_the_exports_with_one_argument_list_per_pair():
    a64, a32 = header_args(INT_NAMES[0]), header_args(INT_NAMES[1])
    assert a64 == ["mh_model_t model", "int64_t B", "double dt", "const double *qd", "const double *qdd", "const double *gq_next",
                   "const double *gqd_next", "const mh_options *opts", "double *gq_out", "double *gqd_out", "double *gqdd_out"]
    assert a32 == [a.replace("double *", "float *") for a in a64]
    b64, b32 = header_args(STEP_NAMES[0]), header_args(STEP_NAMES[1])
    assert b64 == ["mh_model_t model", "int64_t B", "double dt", "const double *q", "const double *qd", "const double *tau",
                   "const double gravity[3]", "const double *f_ext", "const double *gq_next", "const double *gqd_next", "const mh_options *opts",
                   "double *qdd_out", "double *gq_out", "double *gqd_out", "double *gtau_out"]
    assert b32 == [a if "gravity" in a else a.replace("double *", "float *") for a in b64]
    assert re.search(r"MH_ABI_VERSION\s+5\b", HEADER)  # new exports only


def test_python_binding_lists_and_types_them(hip_lib):
    P, I64, D = ctypes.c_void_p, ctypes.c_int64, ctypes.c_double
    assert hip_lib.mh_abi_version() == 5
    for names, n, opts_at in ((INT_NAMES, 11, 7), (STEP_NAMES, 15, 10)):
        for name in names:
            assert name in _lib.ABI_SYMBOLS
            fn = getattr(hip_lib, name)  # (AttributeError: the library does not export it)
            assert len(fn.argtypes) == n and fn.argtypes[0] is P and fn.argtypes[1] is I64 and fn.argtypes[2] is D
            assert all(a is P for k, a in enumerate(fn.argtypes) if k > 2 and k != opts_at)
            assert fn.argtypes[opts_at] is not P


def test_null_model_is_refused_before_any_device_work(hip_lib):
    for names, n in ((INT_NAMES, 11), (STEP_NAMES, 15)):
        for name in names:
            assert getattr(hip_lib, name)(None, 4, 1.0e-3, *([None] * (n - 3))) == INVALID
            assert hip_lib.mh_last_error()


def test_java_handles_match():
    text = re.sub(r"/\*.*?\*/", " ", NATIVE, flags=re.S)
    for names, n in ((INT_NAMES, 11), (STEP_NAMES, 15)):
        for name in names:
            m = re.search(r'handle\(\s*"' + name + r'"\s*,\s*status\(([^)]*)\)\s*\)\s*;', text, flags=re.S)
            assert m, f"no Java handle for {name}"
            assert [k.strip() for k in m.group(1).split(",")] == ["ADDRESS", "JAVA_LONG", "JAVA_DOUBLE"] + ["ADDRESS"] * (n - 3)
