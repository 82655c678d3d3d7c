"""Host-only: the two apparent-inertia exports and their two constants exist in include/mecano_hip.h, mecano_amd/_lib.py and the Java
handles, with the same argument lists."""
import ctypes
import os
import re

from mecano_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "mecano_hip.h")).read()
NATIVE = open(os.path.join(ROOT, "java", "us", "ihmc", "mecano", "hip", "MecanoHipNative.java")).read()
NAMES = ("mh_apparent_inertia_inverse_f64", "mh_apparent_inertia_inverse_f32")
KINDS = ["ADDRESS", "JAVA_LONG", "ADDRESS", "JAVA_INT", "ADDRESS", "ADDRESS", "JAVA_INT", "ADDRESS", "ADDRESS"]


def header_args(name):
    text = re.sub(r"/\*.*?\*/", " ", HEADER, flags=re.S)
    m = re.search(r"mh_status\s+" + name + r"\s*\(([^;]*?)\)\s*;", text, flags=re.S)
    assert m, f"{name} is not declared"
    return [" ".join(a.split()) for a in m.group(1).split(",")]


def test_header_declares_both_exports_with_one_argument_list():
    a64, a32 = header_args(NAMES[0]), header_args(NAMES[1])
    assert a64 == ["mh_model_t model", "int64_t B", "const double *q", "int32_t n_targets", "const int32_t *target_joints",
                   "const double *target_poses", "int32_t blocks", "const mh_options *opts", "double *W_out"]
    assert a32 == [a.replace("double *q", "float *q").replace("double *W_out", "float *W_out") for a in a64]  # the poses stay double


def test_constants_agree():
    assert re.search(r"MH_APPARENT_BLOCKS_DIAGONAL\s*=\s*0\s*,\s*MH_APPARENT_BLOCKS_COUPLED\s*=\s*1", HEADER)
    assert re.search(r"#define\s+MH_MAX_APPARENT_TARGETS\s+16\b", HEADER)
    assert (_lib.APPARENT_BLOCKS_DIAGONAL, _lib.APPARENT_BLOCKS_COUPLED, _lib.MAX_APPARENT_TARGETS) == (0, 1, 16)
    assert re.search(r"APPARENT_BLOCKS_DIAGONAL\s*=\s*0\s*,\s*APPARENT_BLOCKS_COUPLED\s*=\s*1\s*;", NATIVE)
    assert re.search(r"MAX_APPARENT_TARGETS\s*=\s*16\s*;", NATIVE)
    assert re.search(r"MH_ABI_VERSION\s+5\b", HEADER)  # new exports only


def test_python_binding_lists_and_types_both(hip_lib):
    P, I64, I32 = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32
    for name in NAMES:
        assert name in _lib.ABI_SYMBOLS
        fn = getattr(hip_lib, name)
        assert [a for a in fn.argtypes[:7]] == [P, I64, P, I32, P, P, I32] and fn.argtypes[8] is P and len(fn.argtypes) == 9


def test_java_handles_match():
    text = re.sub(r"/\*.*?\*/", " ", NATIVE, flags=re.S)
    for name in NAMES:
        m = re.search(r'handle\(\s*"' + name + r'"\s*,\s*status\(([^)]*)\)\s*\)\s*;', text, flags=re.S)
        assert m, f"no Java handle for {name}"
        assert [k.strip() for k in m.group(1).split(",")] == KINDS
