"""bench.py's own contract: a plain run times exactly --steps steps and prints the headline line, nothing else; --dump-outputs writes what
the timed call returned in its last step, whole or as one fixed seeded sample of rows within the size budget."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def test_dump_outputs_writes_whole_arrays_in_their_dtype_within_the_budget(tmp_path):
    import torch
    import bench
    tau = torch.arange(12, dtype=torch.float64).reshape(4, 3)
    H = torch.arange(36, dtype=torch.float32).reshape(4, 3, 3)
    assert bench.dump_outputs(str(tmp_path), {"rnea_tau": tau, "crba_H": H}) is None
    got_tau, got_H = np.load(tmp_path / "rnea_tau.npy"), np.load(tmp_path / "crba_H.npy")
    assert got_tau.dtype == np.float64 and np.array_equal(got_tau, tau.numpy())
    assert got_H.dtype == np.float32 and np.array_equal(got_H, H.numpy())


def test_dump_outputs_samples_the_same_rows_of_every_output_beyond_the_budget(tmp_path):
    import torch
    import bench
    B, nv = 1000, 5
    tau = torch.arange(B * nv, dtype=torch.float64).reshape(B, nv)
    qdd = -tau.to(torch.float32)
    budget = 100 * nv * (8 + 4) + 7  # room for 100 rows of both
    rows = bench.dump_outputs(str(tmp_path / "a"), {"rnea_tau": tau, "aba_qdd": qdd}, budget=budget)
    assert len(rows) == 100 and np.all(np.diff(rows) > 0) and rows[-1] < B
    a_tau, a_qdd = np.load(tmp_path / "a" / "rnea_tau.npy"), np.load(tmp_path / "a" / "aba_qdd.npy")
    assert a_tau.nbytes + a_qdd.nbytes <= budget and a_qdd.dtype == np.float32
    assert np.array_equal(a_tau, tau.numpy()[rows]) and np.array_equal(a_qdd, qdd.numpy()[rows])
    # the same arguments, the same rows
    assert np.array_equal(bench.dump_outputs(str(tmp_path / "b"), {"rnea_tau": tau, "aba_qdd": qdd}, budget=budget), rows)
    assert np.array_equal(np.load(tmp_path / "b" / "rnea_tau.npy"), a_tau)


def test_regions_are_refused_without_full():
    """A plain run times one region of exactly --steps steps: asking it for more regions is an error, not a silent change of the count."""
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "2", "--regions", "3"], capture_output=True, text=True,
                       timeout=120)
    assert p.returncode == 2 and "--regions needs --full" in p.stderr


@pytest.mark.gpu
def test_plain_run_times_exactly_its_steps_and_dumps_what_the_call_returned(hip_lib, tmp_path):
    """The metric's plain run: ONE timed region of exactly --steps steps, a line without the --full parts (no oracle check, roofline,
    kernel times or CPU baseline), and the dumped tau / qdd of mh_rnea_aba_f64 on the benchmark's seeded inputs, every row checked here
    against the CPU oracle."""
    import bench
    from mecano_amd import random_tools as rt
    from oracle.cpu_oracle import OracleModel
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "7", "--warmup", "2", "--dump-outputs",
                        str(tmp_path)], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, p.stdout
    line = json.loads(lines[0])
    assert line["steps"] == 7 and line["regions"] == 1 and len(line["region_ms"]) == 1 and line["full"] is False
    assert line["ms_per_step"] == pytest.approx(line["region_ms"][0] / 7)
    assert line["value"] == pytest.approx(bench.BATCH * 7 / (line["region_ms"][0] * 1e-3))
    assert (line["unit"], line["higher_is_better"], line["dtype"]) == ("configs/s", True, "f64")
    assert not {"check", "roofline", "kernels_ms", "cpu_baseline"} & set(line)
    assert sorted(os.listdir(tmp_path)) == ["aba_qdd.npy", "rnea_tau.npy"]
    sys_ = rt.nextHumanoid(np.random.default_rng(bench.MODEL_SEED))
    q, qd, qdd, tau_in = rt.nextState(np.random.default_rng(bench.STATE_SEED), sys_, bench.BATCH)
    om, g = OracleModel(rt.humanoid30Desc()), (0.0, 0.0, -9.81)
    for name, ref in (("rnea_tau", om.rnea(q, qd, qdd, g)), ("aba_qdd", om.aba(q, qd, tau_in, g))):
        got = np.load(tmp_path / f"{name}.npy")
        assert got.dtype == np.float64 and got.shape == ref.shape == (bench.BATCH, line["config"]["nv"])
        err, bound = float(np.abs(got - ref).max()), 1e-10 * max(1.0, float(np.abs(ref).max()))
        assert err <= bound, (name, err, bound)
