"""The exports of the constraints between two moving bodies on the host side: declared in the header with base_joints behind
target_joints, carried by the ctypes binding with matching argument types, exported by the library, refusing a NULL model before anything
touches a device, and kept out of the code objects' source hash.  No GPU: a model handle needs a device, so the refusals that need one
(base = target, a base out of range, and those inherited from the rooted calls) are exercised through ctypes in
tests/test_gpu_relative_constraints.py::test_refusals_leave_the_outputs_untouched."""
import ctypes
import inspect
import os

import pytest

from test_constrained_dynamics_abi import HEADER, INVALID, c_arguments

EXPORTS = ["mh_aba_constrained_between_f64", "mh_aba_constrained_between_f32", "mh_constraint_impulse_between_f64",
           "mh_constraint_impulse_between_f32"]


@pytest.mark.parametrize("name", EXPORTS)
def test_header_declares_the_rooted_arguments_with_base_joints_behind_target_joints(name):
    rooted = c_arguments(name.replace("_between", ""))
    at = [n for _, n in rooted].index("target_joints") + 1
    assert c_arguments(name) == rooted[:at] + [("constint32_t*", "base_joints")] + rooted[at:]


def test_header_keeps_the_abi_version_and_states_the_scratch():
    import re
    assert re.search(r"#define\s+MH_ABI_VERSION\s+5\b", HEADER)
    assert "(6 n_app)^2 + 6 K + 18 n_joints + nv" in HEADER


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
    tgt, base, rows = (ctypes.c_int32 * 1)(0), (ctypes.c_int32 * 1)(-1), (ctypes.c_int32 * 1)(0x3F)
    if "aba_constrained" in name:
        st = getattr(hip_lib, name)(None, 1, None, None, None, None, None, 1, tgt, base, None, rows, None, None, 0.0, None, None, None)
    else:
        st = getattr(hip_lib, name)(None, 1, None, None, 1, tgt, base, None, rows, None, None, 0.0, None, None, None)
    assert st == INVALID
    assert b"model is NULL" in hip_lib.mh_last_error()


def test_engine_methods_take_bases():
    from mecano_amd import engine
    for fn in (engine.HipModel.aba_constrained, engine.HipModel.constraint_impulse):
        p = inspect.signature(fn).parameters
        assert "bases" in p and p["bases"].default is None


def test_the_kernel_header_stays_the_library_s_alone():
    from mecano_amd import build
    assert "mh_constraint_kernels.h" in [os.path.basename(p) for p in build.LIB_HEADERS]
    assert "mh_constraint_kernels.h" not in [os.path.basename(p) for p in build.SPEC_HASH_FILES + build.SPEC_HEADERS]
