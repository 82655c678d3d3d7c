"""Host-only: the two mass-matrix-inverse exports and their constant exist in include/mecano_hip.h, mecano_amd/_lib.py, the library and
the Java handles, with the same argument lists; the one argument error that is refused before the device is looked at comes back as
MH_ERR_INVALID_ARGUMENT (the others need a model, hence a device: tests/test_gpu_mass_matrix_inverse.py)."""
import ctypes
import os
import re

from mecano_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "mecano_hip.h")).read()
NATIVE = open(os.path.join(ROOT, "java", "us", "ihmc", "mecano", "hip", "MecanoHipNative.java")).read()
CALCULATOR = open(os.path.join(ROOT, "java", "us", "ihmc", "mecano", "hip", "HipMultiBodyResponseCalculator.java")).read()
NAMES = ("mh_mass_matrix_inverse_f64", "mh_mass_matrix_inverse_f32")
KINDS = ["ADDRESS", "JAVA_LONG", "ADDRESS", "JAVA_INT", "ADDRESS", "ADDRESS", "ADDRESS"]
INVALID = 1  # MH_ERR_INVALID_ARGUMENT


def header_args(name):
    text = re.sub(r"/\*.*?\*/", " ", HEADER, flags=re.S)
    m = re.search(r"mh_status\s+" + name + r"\s*\(([^;]*?)\)\s*;", text, flags=re.S)
    assert m, f"{name} is not declared"
    return [" ".join(a.split()) for a in m.group(1).split(",")]


def test_header_declares_both_exports_with_one_argument_list():
    a64, a32 = header_args(NAMES[0]), header_args(NAMES[1])
    assert a64 == ["mh_model_t model", "int64_t B", "const double *q", "int32_t n_columns", "const int32_t *columns", "const mh_options *opts",
                   "double *Hinv_out"]
    assert a32 == [a.replace("double *q", "float *q").replace("double *Hinv_out", "float *Hinv_out") for a in a64]


def test_constant_agrees():
    assert re.search(r"#define\s+MH_MAX_INVERSE_COLUMNS\s+64\b", HEADER)
    assert _lib.MAX_INVERSE_COLUMNS == 64
    assert re.search(r"MAX_INVERSE_COLUMNS\s*=\s*64\s*;", NATIVE)
    assert re.search(r"MH_ABI_VERSION\s+5\b", HEADER)  # new exports only


def test_python_binding_lists_and_types_both(hip_lib):
    P, I64, I32 = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32
    assert hip_lib.mh_abi_version() == 5
    for name in NAMES:
        assert name in _lib.ABI_SYMBOLS
        fn = getattr(hip_lib, name)  # (AttributeError: the library does not export it)
        assert [a for a in fn.argtypes[:5]] == [P, I64, P, I32, P] and fn.argtypes[6] is P and len(fn.argtypes) == 7


def test_null_model_is_refused_before_any_device_work(hip_lib):
    cols = (ctypes.c_int32 * 2)(0, 1)
    for name in NAMES:
        fn = getattr(hip_lib, name)
        assert fn(None, 4, None, 2, cols, None, None) == INVALID
        assert hip_lib.mh_last_error()
        assert fn(None, 0, None, 0, None, None, None) == INVALID


def test_java_handles_match_and_the_calculator_uses_them():
    text = re.sub(r"/\*.*?\*/", " ", NATIVE, flags=re.S)
    for name in NAMES:
        m = re.search(r'handle\(\s*"' + name + r'"\s*,\s*status\(([^)]*)\)\s*\)\s*;', text, flags=re.S)
        assert m, f"no Java handle for {name}"
        assert [k.strip() for k in m.group(1).split(",")] == KINDS
    assert "MecanoHipNative.MASS_MATRIX_INVERSE.invokeExact(" in CALCULATOR
    for method in ("computeJointApparentInertiaInverse(JointReadOnly target)", "computeJointSpaceInertiaInverse()"):
        assert "public DMatrixRMaj " + method in CALCULATOR
