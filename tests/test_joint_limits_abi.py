"""The joint-limit exports on the host side: declared in the header with the documented argument order and limits, carried by the ctypes
binding with matching argument types, exported by the library, refusing a NULL model before anything touches a device; the kernel header
compiled into the library and kept out of the code objects' source hash; and the host-only choice between the LDS-resident and the streamed
solve (mh_launch_plans.h: limit_plan).  No GPU: the refusals that need a model are exercised through ctypes in
tests/test_gpu_joint_limits.py::test_refusals_leave_the_outputs_untouched."""
import ctypes
import os
import re

import pytest

from test_constrained_dynamics_abi import HEADER, INVALID, c_arguments
from test_launch_plans_cpu import Planner

EXPORTS = ["mh_joint_limit_impulse_f64", "mh_joint_limit_impulse_f32"]
ARGUMENTS = ["model", "B", "q", "qd", "n_limits", "limit_joints", "lower", "upper", "margin", "erp", "impulse_init", "compliance", "n_iterations", "opts",
             "qd_out", "impulse_out", "residual_out"]
KB160 = 160 * 1024


@pytest.mark.parametrize("name", EXPORTS)
def test_header_declares_the_export_with_the_issue_s_argument_order(name):
    assert [n for _, n in c_arguments(name)] == ARGUMENTS


def test_header_states_the_limits_and_keeps_the_abi_version():
    assert re.search(r"#define\s+MH_MAX_LIMIT_JOINTS\s+64\b", HEADER)
    assert re.search(r"#define\s+MH_MAX_INVERSE_COLUMNS\s+64\b", HEADER)  # the listed-column launch carries the rows
    assert re.search(r"#define\s+MH_MAX_LIMIT_ITERATIONS\s+4096\b", HEADER)
    assert re.search(r"#define\s+MH_ABI_VERSION\s+5\b", HEADER)
    from mecano_amd import _lib
    assert (_lib.MAX_LIMIT_JOINTS, _lib.MAX_LIMIT_ITERATIONS) == (64, 4096)


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
    assert all(args[n] == f"const{real}*" for n in ("q", "qd", "impulse_init"))
    assert all(args[n] == f"{real}*" for n in ("qd_out", "impulse_out", "residual_out"))
    assert args["lower"] == args["upper"] == "constdouble*" and args["limit_joints"] == "constint32_t*"
    assert args["margin"] == args["erp"] == args["compliance"] == "double"  # whatever the precision


@pytest.mark.parametrize("name", EXPORTS)
def test_null_model_is_refused(hip_lib, name):
    jnt, lo, hi = (ctypes.c_int32 * 1)(0), (ctypes.c_double * 1)(-1.0), (ctypes.c_double * 1)(1.0)
    assert getattr(hip_lib, name)(None, 1, None, None, 1, jnt, lo, hi, 0.0, 0.0, None, 0.0, 10, None, None, None, None) == INVALID
    assert b"model is NULL" in hip_lib.mh_last_error()
    assert hip_lib.mh_internal_limit_path(None, 0) == INVALID


def test_engine_has_the_method():
    import inspect
    from mecano_amd import engine
    sig = inspect.signature(engine.HipModel.joint_limit_impulse)
    assert list(sig.parameters) == ["self", "q", "qd", "joints", "lower", "upper", "margin", "erp", "compliance", "iterations", "init", "layout", "out"]
    defaults = {k: p.default for k, p in sig.parameters.items() if p.default is not inspect.Parameter.empty}
    assert defaults == dict(margin=0.0, erp=0.0, compliance=0.0, iterations=50, init=None, layout=0, out=None)


def test_java_declares_the_natives():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "java", "us", "ihmc", "mecano", "hip", "MecanoHipNative.java")).read()
    for name in EXPORTS:
        assert 'handle("%s"' % name in text, name
    assert re.search(r"MAX_LIMIT_JOINTS\s*=\s*64\s*,\s*MAX_LIMIT_ITERATIONS\s*=\s*4096", text)


def test_the_kernel_header_is_the_library_s_alone():
    from mecano_amd import build
    names = [os.path.basename(p) for p in build.LIB_HEADERS]
    assert "mh_limit_kernels.h" in names
    assert "mh_limit_kernels.h" not in [os.path.basename(p) for p in build.SPEC_HASH_FILES + build.SPEC_HEADERS]


def state_bytes(L, elem):
    return 3 * L * 64 * elem


def full_bytes(L, elem):
    return (L * (L + 1) // 2 + 3 * L) * 64 * elem


def test_the_plan_keeps_S_in_lds_while_it_fits(hip_lib):
    """limit_plan(L, element size, force, CUs, batch) -> (resident, LDS bytes, waves per CU, grid): the triangle of S stays in LDS beside
    the 3 L state entries while both fit the 160 KB of a CU; above that the state alone; forcing streams anything and makes nothing
    resident that does not fit."""
    P = Planner(hip_lib, "arm7")
    cus, B = 256, 1 << 20
    for elem in (4, 8):
        for L in range(1, 65):
            resident, lds, per_cu, grid = (int(x) for x in P.plan("limit_solve", L, elem, -1, cus, B))
            fits = full_bytes(L, elem) <= KB160
            assert resident == fits, (L, elem)
            assert lds == (full_bytes(L, elem) if fits else state_bytes(L, elem))
            assert per_cu == max(1, min(8, KB160 // lds)) and per_cu * lds <= KB160 and grid == cus * per_cu
            assert [int(x) for x in P.plan("limit_solve", L, elem, 1, cus, B)] == [resident, lds, per_cu, grid]  # forcing LDS makes nothing fit
            streamed = state_bytes(L, elem)
            assert [int(x) for x in P.plan("limit_solve", L, elem, 0, cus, B)] == [0, streamed, max(1, min(8, KB160 // streamed)), cus * max(1, min(8, KB160 // streamed))]
    first = lambda L, elem: int(P.plan("limit_solve", L, elem, -1, cus, B)[0])
    assert (first(22, 8), first(23, 8), first(32, 4), first(33, 4)) == (1, 0, 1, 0)
    assert (full_bytes(22, 8), full_bytes(23, 8), full_bytes(32, 4), full_bytes(33, 4)) == (163328, 176640, 159744, 168960)
    assert [int(x) for x in P.plan("limit_solve", 22, 8, -1, cus, B)] == [1, 163328, 1, cus]
    assert [int(x) for x in P.plan("limit_solve", 64, 8, -1, cus, B)] == [0, 98304, 1, cus]
    assert [int(x) for x in P.plan("limit_solve", 64, 4, -1, cus, B)] == [0, 49152, 3, 3 * cus]
    assert [int(x) for x in P.plan("limit_solve", 7, 8, -1, cus, B)] == [1, 25088, 6, 6 * cus]
    # small batches: one wave per group of 64 configurations
    for B_small, groups in ((0, 1), (1, 1), (64, 1), (65, 2), (257, 5)):
        assert int(P.plan("limit_solve", 7, 8, -1, cus, B_small)[3]) == groups
    for bad in ((0, 8, -1, cus, 1), (65, 8, -1, cus, 1), (4, 2, -1, cus, 1), (4, 8, 2, cus, 1), (4, 8, -1, 0, 1), (4, 8, -1, cus, -1), (4, 8, -1)):
        assert P.status("limit_solve", *bad)[0] == INVALID, bad
