"""The bias-split forward dynamics against the tree-split kernels of the same code object (MH_ZV=0), row for row, on the humanoid and the
centaur at B = 197, 4 096 and 4 097 (a ragged last group): mh_aba_f64 and mh_rnea_aba_f64.  The two-stage inertia job relays the outward
acceleration of a sub-trunk body through LDS to the wave that owns a leg and the neck (mh_zv_kernels.h: ZvWalk, ZvRelayCtx); a relay
that is read before it is written, or a trunk acceleration written by the wrong wave, shows as whole rows going wrong here.

The bound: the worst scaled difference max|a - a0| / max(1, max|a0|) that the commit BEFORE the relay reaches in this very comparison
(tools/measure_tail_parity.py; profiles/tail_parity.txt: 4.6e-16 on the humanoid, 8.6e-16 on the centaur) times 4 -- the relay moves
values, it rounds nothing differently and adds no operation.  The efforts of the pair call come from the inverse-dynamics job, which the
relay does not touch: bit for bit.
"""
import os
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tools"))

pytestmark = pytest.mark.gpu

PARENT_WORST = {"humanoid": 4.594e-16, "centaur": 8.566e-16}  # profiles/tail_parity.txt
FACTOR = 4.0


def test_bias_split_matches_tree_split_row_for_row(hip_lib):
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    import measure_tail_parity as m
    rows = m.cases()
    assert {(r[0], r[1]) for r in rows} == {(s, b) for s in m.SHAPES for b in m.BATCHES}
    for name, B, call, err, same in rows:
        print(f"{name} B={B} {call}: worst scaled difference {err:.3e} (bound {FACTOR * PARENT_WORST[name]:.3e}), efforts bit for bit: {same}")
    for name, B, call, err, same in rows:
        assert err <= FACTOR * PARENT_WORST[name], (name, B, call, err)
        assert same, (name, B, call, "the pair call's efforts differ from the tree-split kernels'")
