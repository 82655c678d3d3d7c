"""The constrained-dynamics exports on the host side: declared in the header, carried by the ctypes binding with matching argument counts,
exported by the library, refusing a NULL model before anything touches a device, and kept out of the code objects' source hash.  No GPU:
a model handle needs a device, so the refusals that need one (target lists, masks, compliance, aliasing) are exercised through ctypes in
tests/test_gpu_constrained_dynamics.py::test_refusals_leave_the_outputs_untouched."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "mecano_hip.h")).read()
EXPORTS = ["mh_aba_constrained_f64", "mh_aba_constrained_f32", "mh_constraint_impulse_f64", "mh_constraint_impulse_f32"]
INVALID = 1  # MH_ERR_INVALID_ARGUMENT


def c_arguments(name):
    """The argument list of a prototype in the header, comments removed: [(type, name)]"""
    text = re.sub(r"/\*.*?\*/", "", HEADER, flags=re.S)
    m = re.search(r"\bmh_status\s+%s\s*\((.*?)\)\s*;" % name, text, flags=re.S)
    assert m, f"{name} is not declared"
    args = []
    for a in m.group(1).split(","):
        a = " ".join(a.split())
        mm = re.match(r"(.*?)(\w+)(\[\d+\])?$", a)
        args.append(((mm.group(1) + ("*" if mm.group(3) else "")).replace(" ", ""), mm.group(2)))
    return args


@pytest.mark.parametrize("name", EXPORTS)
def test_header_declares_the_export_with_the_issue_s_argument_order(name):
    names = [n for _, n in c_arguments(name)]
    targets = ["n_targets", "target_joints", "target_poses", "target_rows", "active"]
    if "aba_constrained" in name:
        assert names == ["model", "B", "q", "qd", "tau", "gravity", "f_ext"] + targets + ["a_des", "compliance", "opts", "qdd_out", "lambda_out"]
    else:
        assert names == ["model", "B", "q", "qd"] + targets + ["v_des", "compliance", "opts", "qd_out", "impulse_out"]


def test_header_states_the_limit_and_keeps_the_abi_version():
    assert re.search(r"#define\s+MH_MAX_CONSTRAINT_TARGETS\s+8\b", HEADER)
    assert re.search(r"#define\s+MH_ABI_VERSION\s+5\b", HEADER)
    from mecano_amd import _lib
    assert _lib.MAX_CONSTRAINT_TARGETS == 8


@pytest.mark.parametrize("name", EXPORTS)
def test_binding_matches_the_prototype(hip_lib, name):
    from mecano_amd import _lib
    assert name in _lib.ABI_SYMBOLS
    fn = getattr(hip_lib, name)
    kinds = {"int64_t": ctypes.c_int64, "int32_t": ctypes.c_int32, "double": ctypes.c_double, "mh_model_t": ctypes.c_void_p}
    want = [ctypes.POINTER(_lib.MhOptions) if t == "constmh_options*" else kinds.get(t, ctypes.c_void_p) for t, _ in c_arguments(name)]
    assert list(fn.argtypes) == want
    real = "double" if name.endswith("f64") else "float"
    assert all(t == f"const{real}*" for t, n in c_arguments(name) if n in ("q", "qd", "tau", "f_ext", "a_des", "v_des"))
    assert all(t == f"{real}*" for t, n in c_arguments(name) if n.endswith("_out"))


@pytest.mark.parametrize("name", EXPORTS)
def test_null_model_is_refused(hip_lib, name):
    tgt, rows = (ctypes.c_int32 * 1)(0), (ctypes.c_int32 * 1)(0x3F)
    if "aba_constrained" in name:
        st = getattr(hip_lib, name)(None, 1, None, None, None, None, None, 1, tgt, None, rows, None, None, 0.0, None, None, None)
    else:
        st = getattr(hip_lib, name)(None, 1, None, None, 1, tgt, None, rows, None, None, 0.0, None, None, None)
    assert st == INVALID
    assert b"model is NULL" in hip_lib.mh_last_error()


def test_engine_has_the_methods():
    from mecano_amd import engine
    assert callable(engine.HipModel.aba_constrained) and callable(engine.HipModel.constraint_impulse)


def test_the_kernel_header_is_the_library_s_alone():
    """mh_constraint_kernels.h is compiled into the library and hashed with it, and is no source of the topology-specialised code objects:
    their hash, and with it every code object built before, stays valid."""
    from mecano_amd import build
    names = [os.path.basename(p) for p in build.LIB_HEADERS]
    assert "mh_constraint_kernels.h" in names
    assert "mh_constraint_kernels.h" not in [os.path.basename(p) for p in build.SPEC_HASH_FILES + build.SPEC_HEADERS]
