"""The exports of the contact impulses between two moving bodies on the host side: declared in the header with the documented argument
order (base_joints directly behind target_joints), the limits and the ABI version unchanged, carried by the ctypes binding with matching
argument types, exported by the library, refusing a NULL model before anything touches a device; the engine method beside the rooted one,
whose signature stays; the Java natives; the kernel header still the library's alone.  No GPU: the refusals that need a model are exercised
through ctypes in tests/test_gpu_contact_between.py::test_refusals_leave_the_outputs_untouched."""
import ctypes
import os
import re

import pytest

from test_constrained_dynamics_abi import HEADER, INVALID, c_arguments

EXPORTS = ["mh_contact_impulse_between_f64", "mh_contact_impulse_between_f32"]
ARGUMENTS = ["model", "B", "q", "qd", "n_targets", "target_joints", "base_joints", "target_poses", "mu", "normals", "active", "v_normal", "impulse_init",
             "compliance", "n_iterations", "opts", "qd_out", "impulse_out", "residual_out"]


@pytest.mark.parametrize("name", EXPORTS)
def test_header_declares_the_export_with_the_issue_s_argument_order(name):
    assert [n for _, n in c_arguments(name)] == ARGUMENTS
    rooted = [n for _, n in c_arguments(name.replace("_between", ""))]
    assert [n for n in ARGUMENTS if n != "base_joints"] == rooted  # the rooted call's arguments, in its order


def test_limits_and_abi_version_are_unchanged():
    assert re.search(r"#define\s+MH_MAX_CONTACT_TARGETS\s+8\b", HEADER)
    assert re.search(r"#define\s+MH_MAX_CONTACT_ITERATIONS\s+4096\b", HEADER)
    assert re.search(r"#define\s+MH_MAX_APPARENT_TARGETS\s+16\b", HEADER)
    assert re.search(r"#define\s+MH_ABI_VERSION\s+5\b", HEADER)
    from mecano_amd import _lib
    assert (_lib.MAX_CONTACT_TARGETS, _lib.MAX_CONTACT_ITERATIONS) == (8, 4096)


@pytest.mark.parametrize("name", EXPORTS)
def test_binding_matches_the_prototype(hip_lib, name):
    from mecano_amd import _lib
    assert name in _lib.ABI_SYMBOLS
    fn = getattr(hip_lib, name)
    kinds = {"int64_t": ctypes.c_int64, "int32_t": ctypes.c_int32, "double": ctypes.c_double, "mh_model_t": ctypes.c_void_p}
    want = [ctypes.POINTER(_lib.MhOptions) if t == "constmh_options*" else kinds.get(t, ctypes.c_void_p) for t, _ in c_arguments(name)]
    assert list(fn.argtypes) == want
    real = "double" if name.endswith("f64") else "float"
    args = dict((n, t) for t, n in c_arguments(name))
    assert all(args[n] == f"const{real}*" for n in ("q", "qd", "normals", "v_normal", "impulse_init"))
    assert all(args[n] == f"{real}*" for n in ("qd_out", "impulse_out", "residual_out"))
    assert args["mu"] == "constdouble*" and args["target_poses"] == "constdouble*" and args["compliance"] == "double"  # whatever the precision
    assert args["target_joints"] == "constint32_t*" and args["base_joints"] == "constint32_t*"


@pytest.mark.parametrize("name", EXPORTS)
def test_null_model_is_refused(hip_lib, name):
    tgt, base, mu = (ctypes.c_int32 * 1)(0), (ctypes.c_int32 * 1)(-1), (ctypes.c_double * 1)(0.5)
    assert getattr(hip_lib, name)(None, 1, None, None, 1, tgt, base, None, mu, None, None, None, None, 0.0, 10, None, None, None, None) == INVALID
    assert b"model is NULL" in hip_lib.mh_last_error()


def test_engine_has_the_method_and_the_rooted_one_keeps_its_signature():
    import inspect
    from mecano_amd import engine
    names = list(inspect.signature(engine.HipModel.contact_impulse_between).parameters)
    assert names == ["self", "q", "qd", "targets", "bases", "mu", "poses", "normals", "active", "v_normal", "compliance", "iterations", "init", "layout",
                     "out"]
    defaults = {k: p.default for k, p in inspect.signature(engine.HipModel.contact_impulse_between).parameters.items()}
    assert (defaults["poses"], defaults["compliance"], defaults["iterations"], defaults["init"], defaults["out"]) == (None, 0.0, 50, None, None)
    assert defaults["bases"] is inspect.Parameter.empty and defaults["mu"] is inspect.Parameter.empty
    names = list(inspect.signature(engine.HipModel.contact_impulse).parameters)
    assert names == ["self", "q", "qd", "targets", "mu", "poses", "normals", "active", "v_normal", "compliance", "iterations", "init", "layout", "out"]


def test_java_declares_the_natives():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "java", "us", "ihmc", "mecano", "hip", "MecanoHipNative.java")).read()
    for name in EXPORTS:
        assert 'handle("%s"' % name in text, name
        decl = text[text.index('handle("%s"' % name):]
        decl = decl[:decl.index(";")]
        assert decl.count("ADDRESS") == 15 and decl.count("JAVA_INT") == 2 and decl.count("JAVA_LONG") == 1 and decl.count("JAVA_DOUBLE") == 1


def test_the_kernel_header_is_the_library_s_alone():
    from mecano_amd import build
    names = [os.path.basename(p) for p in build.LIB_HEADERS]
    assert "mh_contact_kernels.h" in names and "mh_constraint_kernels.h" in names
    assert "mh_contact_kernels.h" not in [os.path.basename(p) for p in build.SPEC_HASH_FILES + build.SPEC_HEADERS]
