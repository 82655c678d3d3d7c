"""The reverse-mode kinematics exports on the host side: declared in the header, carried by the ctypes binding and by the Java handle list
with matching descriptors, exported by the library, and refusing a NULL model before anything touches a device.  No GPU."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "mecano_hip.h")).read()
EXPORTS = ["mh_body_poses_vjp_f64", "mh_body_poses_vjp_f32", "mh_jacobian_transpose_f64", "mh_jacobian_transpose_f32"]
INVALID = 1  # MH_ERR_INVALID_ARGUMENT


@pytest.mark.parametrize("name", EXPORTS)
def test_header_declares_the_export(name):
    assert re.search(r"\bmh_status\s+%s\s*\(\s*mh_model_t\s+model\s*,\s*int64_t\s+B\s*," % name, HEADER), name


def test_header_keeps_the_abi_version():
    assert re.search(r"#define\s+MH_ABI_VERSION\s+5\b", HEADER)


@pytest.mark.parametrize("name", EXPORTS)
def test_binding_carries_the_export(hip_lib, name):
    from mecano_amd import _lib
    assert name in _lib.ABI_SYMBOLS
    fn = getattr(hip_lib, name)
    assert len(fn.argtypes) == (9 if "poses" in name else 10)


@pytest.mark.parametrize("name", EXPORTS)
def test_java_handle_list_names_the_export(name):
    from test_java_binding import c_prototypes, java_descriptors
    java = java_descriptors()
    assert name in java, f"{name}: no handle in MecanoHipNative.java"
    assert java[name] == c_prototypes()[name]


@pytest.mark.parametrize("name", EXPORTS)
def test_null_model_is_refused(hip_lib, name):
    tgt = (ctypes.c_int32 * 1)(0)
    if "poses" in name:
        st = getattr(hip_lib, name)(None, 1, None, 1, tgt, None, None, None, None)
    else:
        st = getattr(hip_lib, name)(None, 1, None, 1, None, tgt, None, None, None, None)
    assert st == INVALID
    assert b"model is NULL" in hip_lib.mh_last_error()


def test_engine_and_autograd_have_the_callables():
    from mecano_amd import autograd, engine
    assert callable(engine.HipModel.body_poses_vjp) and callable(engine.HipModel.jacobian_transpose)
    assert callable(autograd.body_poses)
    assert "body_poses" in autograd.__doc__
