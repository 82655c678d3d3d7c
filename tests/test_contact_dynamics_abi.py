"""The frictional-contact exports on the host side: declared in the header with the documented argument order and limits, carried by the
ctypes binding with matching argument types, exported by the library, refusing a NULL model before anything touches a device; the kernel
header compiled into the library and kept out of the code objects' source hash; and the host-only choice between the LDS-resident and the
streamed solve (mh_launch_plans.h: contact_plan).  No GPU: the refusals that need a model are exercised through ctypes in
tests/test_gpu_contact_dynamics.py::test_refusals_leave_the_outputs_untouched."""
import ctypes
import os
import re

import numpy as np
import pytest

from test_constrained_dynamics_abi import HEADER, INVALID, c_arguments
from test_launch_plans_cpu import Planner

EXPORTS = ["mh_contact_impulse_f64", "mh_contact_impulse_f32"]
ARGUMENTS = ["model", "B", "q", "qd", "n_targets", "target_joints", "target_poses", "mu", "normals", "active", "v_normal", "impulse_init", "compliance",
             "n_iterations", "opts", "qd_out", "impulse_out", "residual_out"]


@pytest.mark.parametrize("name", EXPORTS)
def test_header_declares_the_export_with_the_issue_s_argument_order(name):
    assert [n for _, n in c_arguments(name)] == ARGUMENTS


def test_header_states_the_limits_and_keeps_the_abi_version():
    assert re.search(r"#define\s+MH_MAX_CONTACT_TARGETS\s+8\b", HEADER)
    assert re.search(r"#define\s+MH_MAX_CONTACT_ITERATIONS\s+4096\b", HEADER)
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


@pytest.mark.parametrize("name", EXPORTS)
def test_null_model_is_refused(hip_lib, name):
    tgt, mu = (ctypes.c_int32 * 1)(0), (ctypes.c_double * 1)(0.5)
    assert getattr(hip_lib, name)(None, 1, None, None, 1, tgt, None, mu, None, None, None, None, 0.0, 10, None, None, None, None) == INVALID
    assert b"model is NULL" in hip_lib.mh_last_error()
    assert hip_lib.mh_internal_contact_path(None, 0) == INVALID


def test_engine_has_the_method():
    import inspect
    from mecano_amd import engine
    names = list(inspect.signature(engine.HipModel.contact_impulse).parameters)
    assert names == ["self", "q", "qd", "targets", "mu", "poses", "normals", "active", "v_normal", "compliance", "iterations", "init", "layout", "out"]


def test_java_declares_the_natives():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "java", "us", "ihmc", "mecano", "hip", "MecanoHipNative.java")).read()
    for name in EXPORTS:
        assert 'handle("%s"' % name in text, name


def test_the_kernel_header_is_the_library_s_alone():
    from mecano_amd import build
    names = [os.path.basename(p) for p in build.LIB_HEADERS]
    assert "mh_contact_kernels.h" in names
    assert "mh_contact_kernels.h" not in [os.path.basename(p) for p in build.SPEC_HASH_FILES + build.SPEC_HEADERS]


def lds_bytes(K, elem):
    return 9 * K * (K + 1) // 2 * 64 * elem


def test_the_plan_keeps_S_in_lds_while_it_fits(hip_lib):
    """contact_plan(K, element size, force, CUs, batch) -> (resident, LDS bytes, waves per CU, grid, unrolled contacts): the lower block
    triangle of S stays in LDS while it fits the 160 KB of a CU; K = 8 in fp64 (166 KB) streams; forcing streams anything and makes
    nothing resident that does not fit."""
    P = Planner(hip_lib, "arm7")
    cus, B = 256, 1 << 20
    for elem in (4, 8):
        for K in range(1, 9):
            resident, lds, per_cu, grid, kmax = (int(x) for x in P.plan("contact_solve", K, elem, -1, cus, B))
            fits = lds_bytes(K, elem) <= 160 * 1024
            assert resident == fits, (K, elem)
            assert lds == (lds_bytes(K, elem) if fits else 0)
            assert per_cu == (max(1, min(8, 160 * 1024 // lds_bytes(K, elem))) if fits else 8)
            assert per_cu * lds <= 160 * 1024 and grid == cus * per_cu
            assert kmax == (4 if K <= 4 else 8) and kmax >= K
            assert [int(x) for x in P.plan("contact_solve", K, elem, 1, cus, B)] == [resident, lds, per_cu, grid, kmax]  # forcing LDS makes nothing fit
            assert [int(x) for x in P.plan("contact_solve", K, elem, 0, cus, B)] == [0, 0, 8, cus * 8, kmax]
    assert int(P.plan("contact_solve", 8, 8, -1, cus, B)[0]) == 0 and lds_bytes(8, 8) == 165888
    assert all(int(P.plan("contact_solve", K, 8, -1, cus, B)[0]) == 1 for K in (1, 2, 3, 4))
    assert int(P.plan("contact_solve", 8, 4, -1, cus, B)[0]) == 1 and int(P.plan("contact_solve", 8, 4, -1, cus, B)[1]) == 82944
    assert int(P.plan("contact_solve", 4, 8, -1, cus, B)[1]) == 46080
    # small batches: one wave per group of 64 configurations
    for B_small, groups in ((1, 1), (64, 1), (65, 2), (257, 5)):
        assert int(P.plan("contact_solve", 4, 8, -1, cus, B_small)[3]) == groups
    for bad in ((0, 8, -1, cus, 1), (9, 8, -1, cus, 1), (4, 2, -1, cus, 1), (4, 8, 2, cus, 1), (4, 8, -1, 0, 1), (4, 8, -1, cus, -1), (4, 8, -1)):
        assert P.status("contact_solve", *bad)[0] == INVALID, bad
