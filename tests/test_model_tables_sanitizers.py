"""The host-side model compiler (mecano_amd/csrc/mh_model_tables.h: plan_model, compile_model) under AddressSanitizer +
UndefinedBehaviorSanitizer: index arithmetic over caller-supplied maps.  A small stand-alone program includes the header, holds the
descriptions of tests/golden/model_tables_models.json as plain C++ arrays of exactly the sizes the description states, compiles each and
the bad descriptions of tests/test_abi.py, and prints one line per model (hipcc builds it here for the host; nothing touches a device and
nothing is preloaded).  Exit status 0 and an empty stderr is the assertion."""
import json
import os
import shutil
import subprocess

import pytest

from mecano_amd import build as mbuild

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODELS = ("one_revolute", "one_fixed", "star", "every_kind_permuted", "forest2")
FIELDS = (("parent", "int32_t"), ("joint_type", "int32_t"), ("axis", "double"), ("X_before", "double"), ("X_com", "double"), ("inertia_J", "double"),
          ("inertia_mass", "double"), ("inertia_com", "double"), ("dof_indices", "int32_t"), ("cfg_indices", "int32_t"))

MAIN = r"""
// compiles a description and reads every table once, end to end
static long touch(const ModelTables &t)
{
   long sum = 0;
   for (const std::vector<int> *v : {&t.meta, &t.dof_map, &t.cfg_map, &t.engine_of, &t.prog, &t.prog_seq, &t.grav_zero_ofs, &t.grav_zero_cols, &t.resp_info,
                                     &t.minv_owner, &t.deriv_slot})
      for (int x : *v)
         sum += x;
   double fsum = 0.0;
   for (const std::vector<double> *v : {&t.consts, &t.sub_mass, &t.inertial_parameters})
      for (double x : *v)
         fsum += x;
   return sum + (fsum != 0.0);
}
static int run(const char *name, const mh_model_desc &d, mh_status want)
{
   Plan P;
   ModelTables t;
   mh_status st = plan_model(&d, P);
   if (st == MH_OK)
      st = compile_model(&d, P, t);
   printf("%s: status %d n_slots %d events %d checksum %ld%s%s\n", name, (int)st, t.n_slots, (int)t.prog.size(), st == MH_OK ? touch(t) : 0L,
          st == MH_OK ? "" : " -- ", st == MH_OK ? "" : g_err);
   return st == want ? 0 : 1;
}
int main()
{
   int bad = 0;
   MODEL_RUNS
   // the bad descriptions: a cycle, a repeated index, an index out of range, an axis that is no unit vector (on copies of the star)
   {
      int32_t parent[5];
      std::memcpy(parent, star_parent, sizeof parent);
      mh_model_desc d = star();
      d.parent = parent;
      parent[2] = 4; // 2 <-> 4
      bad += run("cycle", d, MH_ERR_LOOP_CLOSURE);
   }
   {
      int32_t dof[5];
      std::memcpy(dof, star_dof_indices, sizeof dof);
      mh_model_desc d = star();
      d.dof_indices = dof;
      dof[3] = dof[1];
      bad += run("repeated index", d, MH_ERR_BAD_TOPOLOGY);
      dof[3] = 5;
      bad += run("index out of range", d, MH_ERR_BAD_TOPOLOGY);
      dof[3] = -1;
      bad += run("negative index", d, MH_ERR_BAD_TOPOLOGY);
   }
   {
      double axis[15];
      std::memcpy(axis, star_axis, sizeof axis);
      mh_model_desc d = star();
      d.axis = axis;
      axis[6] *= 1.5, axis[7] *= 1.5, axis[8] *= 1.5;
      bad += run("non-unit axis", d, MH_ERR_BAD_AXIS);
   }
   return bad;
}
"""


def _program():
    with open(os.path.join(ROOT, "tests", "golden", "model_tables_models.json")) as f:
        models = json.load(f)
    src = ['#include "mh_model_tables.h"', "#include <cstdio>"]
    runs = []
    for name in MODELS:
        m = models[name]
        for field, ctype in FIELDS:
            values = m[field]
            # an array of no entries (the fixed joint's index maps) is one the compiler must never read: a pointer one past an object
            body = ", ".join(repr(v) for v in values)
            src.append(f"static const {ctype} {name}_{field}[{max(1, len(values))}] = {{{body}}};" if values else f"static const {ctype} {name}_{field}_none = 0;")
        ptr = {field: (f"{name}_{field}" if m[field] else f"&{name}_{field}_none + 1") for field, _ in FIELDS}
        src.append(f"static mh_model_desc {name}()\n{{\n   mh_model_desc d;\n   std::memset(&d, 0, sizeof d);\n"
                   f"   d.n_joints = {m['n_joints']}, d.nq = {m['nq']}, d.nv = {m['nv']};\n"
                   + "".join(f"   d.{field} = {ptr[field]};\n" for field, _ in FIELDS) + "   return d;\n}")
        runs.append(f'bad += run("{name}", {name}(), MH_OK);')
    return "\n".join(src) + MAIN.replace("MODEL_RUNS", "\n   ".join(runs))


@pytest.mark.timeout(300)
def test_model_compiler_is_clean_under_asan_and_ubsan(tmp_path):
    hipcc = mbuild.hipcc() if (shutil.which("hipcc") or os.path.exists("/opt/rocm/bin/hipcc")) else None
    if hipcc is None:
        pytest.skip("no hipcc")
    src, exe = tmp_path / "tables.hip", tmp_path / "tables"
    src.write_text(_program())
    subprocess.check_call([hipcc, "--offload-arch=gfx950", "-O1", "-std=c++17", "-w", "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host",
                           "-fno-sanitize-recover=undefined", "-I", os.path.join(ROOT, "mecano_amd", "csrc"), str(src), "-o", str(exe)])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    run = subprocess.run([str(exe)], env=env, capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    assert run.stderr == "", run.stderr
    lines = run.stdout.splitlines()
    assert len(lines) == len(MODELS) + 5 and all(": status " in line for line in lines), run.stdout
    for name in MODELS:
        assert any(line.startswith(name + ": status 0 ") for line in lines), run.stdout
