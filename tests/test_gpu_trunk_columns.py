"""The trunk's columns of the two-stage hand-off signal themselves (mh_zv_kernels.h, "The hand-off without flags"): the bias job stores them
and is done, every wave of the inertia job requests them in front of its early limbs' fold, looks at them behind it (polling while a lane
that holds a configuration still reads the sentinel) and one wave writes the sentinel back behind the barrier that closes the outward sweep.

Shapes: the smallest at which that can go wrong -- humanoid, centaur (two sub-trunks), torso (revolute root, a one-body late limb),
quadruped (the root is the whole trunk, un-staged fold) at B = 1, 63, 64, 65, 197 (one lane, a ragged single group, a full group, a second
group with one active lane, four groups).

1. Row-for-row parity of mh_aba_f64, mh_rnea_aba_f64 and mh_aba_integrate_f64 with the tree-split kernels of the same code object
   (tools/measure_trunk_cols_parity.py).  The change moves values and rounds nothing: the bound is 4 x the worst scaled difference the
   commit BEFORE it reaches in this very comparison (profiles/trunk_cols_parity.txt), the factor of tests/test_gpu_tail_parity.py; the
   pair call's efforts, which the inverse-dynamics job forms, bit for bit.
2. Stale columns: three launches on one stream without a synchronisation in between, each with other efforts and other velocities (so
   that the trunk's tau - h differs in every configuration), each bit for bit what the same call gives alone.  A consumer that takes the
   previous launch's trunk columns, or a sentinel that did not go back, fails here.
3. A captured launch replayed three times with the inputs overwritten in place: every replay bit for bit the eager result.
4. Behind 2 and 3 the model reports no give-up and no output holds a NaN.
5. Without a GPU: every registered code object keeps the protocol (tools/isa_handoff.py) and no two-stage kernel drains and flags a run
   of column stores any more.
"""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

gpu = pytest.mark.gpu

# profiles/trunk_cols_parity.txt: worst scaled difference of the parent commit per shape, over B = 1, 63, 64, 65, 197 and the three calls
PARENT_WORST = {"humanoid": 8.216e-16, "centaur": 1.116e-15, "torso": 6.460e-16, "quadruped": 5.338e-16}
FACTOR = 4.0
G = (0.3, -0.2, -9.81)
DT = 1e-3


@gpu
@pytest.mark.parametrize("shape", ["humanoid", "centaur", "torso", "quadruped"])
def test_bias_split_matches_tree_split_row_for_row(hip_lib, shape):
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    import measure_trunk_cols_parity as m
    rows = m.cases((shape,))
    assert {(r[1], r[2]) for r in rows} == {(b, c) for b in (1, 63, 64, 65, 197) for c in ("aba", "rnea_aba", "step")}
    bound = FACTOR * PARENT_WORST[shape]
    for name, B, call, err, same in rows:
        print(f"{name} B={B} {call}: worst scaled difference {err:.3e} (bound {bound:.3e})" + (f", efforts bit for bit: {same}" if call == "rnea_aba" else ""))
    for name, B, call, err, same in rows:
        assert err <= bound, (name, B, call, err)
        assert same, (name, B, call, "the pair call's efforts differ from the tree-split kernels'")


_MODELS = {}


def _zv_model(shape):
    """(system, bias-split model at every batch size), one per shape for the module"""
    import measure_trunk_cols_parity as m
    if shape not in _MODELS:
        sys_ = m.system_of(shape)
        _MODELS[shape] = (sys_, m.models_of(sys_.toModelDesc())[1])
    return _MODELS[shape]


def _states(sys_, B, n, seed):
    """n states of one batch whose efforts and velocities all differ (the velocities by a factor per state on top: other bias forces everywhere)"""
    import torch
    from mecano_amd import random_tools as rt
    out = []
    for i in range(n):
        q, qd, qdd, tau = rt.nextState(np.random.default_rng(seed + 100 * i), sys_, B)
        out.append(tuple(torch.tensor(x, device="cuda") for x in (q, (1.0 + 0.5 * i) * qd, qdd, tau)))
    return out


def _call(hm, which, st):
    q, qd, qdd, tau = st
    if which == "aba":
        return (hm.aba(q, qd, tau, G),)
    if which == "rnea_aba":
        return hm.rnea_aba(q, qd, qdd, tau, G)
    return hm.step(DT, q, qd, tau, G)


@gpu
@pytest.mark.parametrize("B", [65, 197])
@pytest.mark.parametrize("shape", ["humanoid", "centaur"])
def test_back_to_back_launches_never_take_the_previous_launch_s_trunk_columns(hip_lib, shape, B):
    import torch
    sys_, hm = _zv_model(shape)
    states = _states(sys_, B, 3, 11 * B)
    for which in ("aba", "rnea_aba", "step"):
        alone = []
        for st in states:
            torch.cuda.synchronize()
            alone.append(_call(hm, which, st))
            torch.cuda.synchronize()
        for a, b in ((0, 1), (1, 2), (0, 2)):  # every configuration's result differs from launch to launch: a stale column shows in every row
            assert bool((alone[a][-1] != alone[b][-1]).any(dim=1).all()), (shape, B, which, a, b)
        torch.cuda.synchronize()
        chained = [_call(hm, which, st) for st in states]  # one stream, nothing in between
        torch.cuda.synchronize()
        for i, (a, c) in enumerate(zip(alone, chained)):
            for k, (x, y) in enumerate(zip(a, c)):
                assert not bool(torch.isnan(y).any()), (shape, B, which, i, k)
                assert torch.equal(x, y), (shape, B, which, "launch", i, "output", k, float((x - y).abs().max()))
    hm.check()  # (MH_OK: nobody gave up)


@gpu
@pytest.mark.parametrize("B", [65, 197])
@pytest.mark.parametrize("shape", ["humanoid", "centaur"])
def test_a_captured_launch_replays_with_inputs_overwritten_in_place(hip_lib, shape, B):
    import torch
    sys_, hm = _zv_model(shape)
    states = _states(sys_, B, 4, 13 * B)
    eager = [_call(hm, "rnea_aba", st) for st in states]
    torch.cuda.synchronize()
    q, qd, qdd, tau = (x.clone() for x in states[0])
    t_out, a_out = torch.empty_like(qd), torch.empty_like(qd)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        hm.bind_rnea_aba(q, qd, qdd, tau, t_out, a_out, G)()  # (warm-up on the capturing stream: nothing is allocated under capture)
        s.synchronize()
        with torch.cuda.graph(graph, stream=s):
            hm.bind_rnea_aba(q, qd, qdd, tau, t_out, a_out, G)()  # (bound inside: the binding takes the current -- capturing -- stream)
    torch.cuda.synchronize()
    for i in (1, 2, 3):
        for dst, src in zip((q, qd, qdd, tau), states[i]):
            dst.copy_(src)
        t_out.zero_(), a_out.zero_()
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        assert not bool(torch.isnan(a_out).any()) and not bool(torch.isnan(t_out).any()), (shape, B, i)
        assert torch.equal(t_out, eager[i][0]), (shape, B, "replay", i, "efforts")
        assert torch.equal(a_out, eager[i][1]), (shape, B, "replay", i, "accelerations", float((a_out - eager[i][1]).abs().max()))
    hm.check()  # (MH_OK: nobody gave up)


def test_no_two_stage_kernel_drains_and_flags_its_columns():
    """Host only: the code objects the build left in the tree, disassembled."""
    import isa_handoff
    from mecano_amd import build as mbuild
    two_stage = 0
    for name, desc in mbuild.registered_models().items():
        found = isa_handoff.zv_kernels(isa_handoff.disassemble(mbuild.build_spec(desc)))
        assert found or name == "arm7", f"{name}: no spec_zv_kernel in its code object"
        for kernel, instrs in found.items():
            assert isa_handoff.check_handoff(instrs) == [], (name, kernel[:60])
            if isa_handoff.is_self_signal(instrs):
                two_stage += 1
                assert isa_handoff.drained_and_flagged_runs(instrs) == [], (name, kernel[:60])
    assert two_stage >= 4  # humanoid, quadruped, torso, centaur: the identity-map kernel of each (and its simulation step)
