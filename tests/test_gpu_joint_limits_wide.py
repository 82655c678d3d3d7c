"""mh_joint_limit_impulse_* on the device where tests/test_gpu_joint_limits.py does not reach: a warm start held to the checker, lists out
of joint order with one range per row, prismatic rows behind shuffled index maps, rows closed in one lane of a wave or in none, limits at
infinity and ranges of no width, and the fp32 LDS boundary (L = 32 / 33) and the cap (L = 64) on a model whose bound says something.  The
cases and the faults they are here to catch are those of tests/test_joint_limits_wide_cpu.py, where
test_planted_faults_are_rejected_on_the_inputs_of_the_device_tests holds the comparison to each of them.  The comparison is hold_parity of
tests/test_gpu_joint_limits.py throughout: close_aba on (qd+, impulse) and on the residual with the checker's cond_kkt, 8 sqrt(8 n) cond u,
u = 2^-53 or 2^-24 (fp32 against the fp64 checker on the fp32-rounded inputs), exact zeros on open rows, no limit that pulls, the momentum
balance; poisoned outputs with guard rows.  B <= 130.

Worst achieved share of the bound per group, fp64 / fp32 (profiles/joint_limits_wide_parity_errors.json; the share is achieved / factor,
the factor 8 sqrt(8 n)):
    warm start                 (qd+, impulse) 0.0030 / 0.0002   residual 0.0030 / 0.0006   momentum balance 0.0101 / 0.0011
    list order, kinds, maps    (qd+, impulse) 0.0071 / 0.0010   residual 0.18   / 0.056    momentum balance 0.0052 / 0.0007
    sparse closure             (qd+, impulse) 0.0001 / 0.0000   residual 0.0002 / 0.0000   momentum balance 0.0002 / 0.0000
    infinite, degenerate       (qd+, impulse) 0.0065 / 0.0009   residual 0.26   / 0.10     momentum balance 0.0057 / 0.0006
    comb16x4, L = 32, 33, 64   (qd+, impulse) 0.0009 / 0.0001   residual 0.033  / 0.024    momentum balance 0.0004 / 0.0001
None is above one half.  (The residual is one number per configuration, the largest change of an impulse in the last sweep: a difference
of two impulses of size 1e2 held relative to max(1, itself), which is why it takes the largest share.)"""
import numpy as np
import pytest

from test_gpu_constrained_dynamics import AOS, SOA, dev, hip_model, laid_out, torch_cuda  # noqa: F401
from test_gpu_joint_limits import call, device_state, hold_parity, set_path
from test_joint_limits_cpu import model_of
from test_joint_limits_wide_cpu import B_SPARSE, B_WIDE, MARGIN, SPARSE_PATTERN, designed_closure, prismatic_rows, solved

pytestmark = pytest.mark.gpu

PRECISIONS = ["f64", "f32"]
NP_DTYPE = {"f64": np.float64, "f32": np.float32}


def torch_dtype(torch, dtype_name):
    return torch.float64 if dtype_name == "f64" else torch.float32


def bits(t):
    """the bit patterns of a device tensor ([B, ...] view or not), as a numpy array of integers"""
    a = np.ascontiguousarray(t.cpu().numpy())
    return a.view(np.int64 if a.dtype == np.float64 else np.int32)


def same_bits(got, want):
    return all(np.array_equal(bits(g), bits(w)) for g, w in zip(got, want))


def rows_of(t, B, layout):
    """[B, entries] view of an output of `call`"""
    return t.reshape(B, -1) if layout == AOS or t.dim() == 1 else t.t()


@pytest.mark.parametrize("dtype_name", PRECISIONS)
@pytest.mark.parametrize("model", ["arm7", "humanoid30", "comb16x4"])
def test_warm_start_matches_checker(torch_cuda, model, dtype_name):
    """A start of twice a standard-normal draw, nonzero on open rows and of the wrong sign for its side on about half of the closed ones:
    1, 3 and 50 sweeps, compliance 0 and 1e-6, both layouts; in place once; and NaN and +-inf in the start of OPEN rows change no bit."""
    torch = torch_cuda
    dtype = torch_dtype(torch, dtype_name)
    case = "warm:" + model
    hm = hip_model(model_of(model)[1])
    for compliance in (0.0, 1.0e-6):
        for sweeps in (1, 3, 50):
            name, I, R = solved(case, NP_DTYPE[dtype_name], sweeps, compliance)
            wrong_side = (R["s"] * I["init"] < 0) & R["closed"]
            assert not R["bad"].any() and wrong_side.mean() > 0.2 * R["closed"].mean() and (I["init"][~R["closed"]] != 0).all()
            for layout in (AOS, SOA):
                label = f"{case} sweeps={sweeps} eps={compliance} layout={layout} {dtype_name}"
                hold_parity(torch, hm, name, I, R, B_WIDE, layout, dtype_name, sweeps, compliance, label, init=I["init"])
    name, I, R = solved(case, NP_DTYPE[dtype_name], 3, 0.0)
    poisoned_start = I["init"].copy()
    open_rows = np.argwhere(~R["closed"])
    assert len(open_rows) >= 3
    for k, (cfg, row) in enumerate(open_rows):
        poisoned_start[cfg, row] = (np.nan, np.inf, -np.inf)[k % 3]
    for layout in (AOS, SOA):
        hold_parity(torch, hm, name, I, R, B_WIDE, layout, dtype_name, 3, 0.0, f"{case} in place layout={layout} {dtype_name}", init=I["init"], in_place=True)
        q, qd = device_state(torch, I, B_WIDE, layout, dtype)
        want = [t.clone() for t in call(hm, q, qd, I, 3, layout, init=laid_out(dev(torch, I["init"], dtype), layout))]
        got = call(hm, q, qd, I, 3, layout, init=laid_out(dev(torch, poisoned_start, dtype), layout))
        torch.cuda.synchronize()
        assert not any(torch.isnan(t).any() for t in want) and want[1].any()
        assert same_bits(got, want), f"{case} layout={layout} {dtype_name}: the start of an open row reached the outputs"


@pytest.mark.parametrize("dtype_name", PRECISIONS)
@pytest.mark.parametrize("what", ["humanoid30_l24_shuffled", "humanoid30_l24_reversed", "humanoid30_l22_shuffled", "onedof12", "mixed12"])
def test_lists_out_of_joint_order_with_a_range_per_row(torch_cuda, what, dtype_name):
    """The humanoid's 24 rows shuffled and reversed (streamed in fp64, resident in fp32) and 22 shuffled (resident in fp64); every one-DoF
    joint of onedof12 and mixed12, shuffled, prismatic ones among them, behind shuffled index maps (on mixed12 no q index is the qd
    index).  One range per row; 3 and 50 sweeps."""
    torch = torch_cuda
    case = "order:" + what
    for sweeps in (3, 50):
        name, I, R = solved(case, NP_DTYPE[dtype_name], sweeps)
        assert not R["bad"].any()
        if name != "humanoid30":
            assert ((np.abs(R["impulse"]) > 0.1) & R["closed"] & prismatic_rows(name, I)[None, :]).any(), "no prismatic row presses"
        hm = hip_model(model_of(name)[1])
        for layout in (AOS, SOA):
            hold_parity(torch, hm, name, I, R, B_WIDE, layout, dtype_name, sweeps, 0.0, f"{case} sweeps={sweeps} layout={layout} {dtype_name}")


@pytest.mark.parametrize("dtype_name", PRECISIONS)
def test_rows_closed_in_one_lane_of_a_wave_or_in_none(torch_cuda, dtype_name):
    """The designed pattern -- wave 0: rows closed in lanes 5, 40 and 63 only, one of them in exactly one lane; wave 1: one row in lane 0;
    the ragged wave: nothing -- on each path, forced and chosen.  A configuration without a closed row returns the bits of qd (a -0.0 among
    them), impulses of zero and residual 0; the three paths agree bit for bit; a batch with nothing closed returns the bits of qd."""
    torch = torch_cuda
    dtype = torch_dtype(torch, dtype_name)
    name, I, R = solved("sparse:designed", NP_DTYPE[dtype_name], 3)
    L = len(I["joints"])
    assert np.array_equal(R["closed"], designed_closure(B_SPARSE, L, SPARSE_PATTERN)) and np.abs(R["impulse"]).max() > 5.0
    idle = ~R["closed"].any(axis=1)
    assert np.signbit(I["qd"][idle]).any() and (I["qd"][idle] == 0).any()
    _, I0, R0 = solved("sparse:none", NP_DTYPE[dtype_name], 3)
    assert not R0["closed"].any()
    hm = hip_model(model_of(name)[1])
    try:
        for layout in (AOS, SOA):
            got = []
            for path in (1, 0, -1):
                set_path(hm, path)
                label = f"sparse path={path} layout={layout} {dtype_name}"
                v, p, r = hold_parity(torch, hm, name, I, R, B_SPARSE, layout, dtype_name, 3, 0.0, label)
                assert np.array_equal(bits(v)[idle], bits(dev(torch, I["qd"], dtype))[idle]), label + ": qd_out of a configuration with no closed row is not qd"
                assert not p[torch.tensor(idle, device="cuda")].any() and not r[torch.tensor(idle, device="cuda")].any(), label
                got.append([bits(t) for t in (v, p, r)])
                v, _, _ = hold_parity(torch, hm, name, I0, R0, B_SPARSE, layout, dtype_name, 3, 0.0, f"nothing closed path={path} layout={layout} {dtype_name}")
                assert np.array_equal(bits(v), bits(dev(torch, I0["qd"], dtype))), label + ": nothing closed, and qd_out is not qd"
            for a, b, c in zip(*got):
                assert np.array_equal(a, b) and np.array_equal(a, c), f"sparse layout={layout} {dtype_name}: the paths differ"
    finally:
        set_path(hm, -1)


@pytest.mark.parametrize("dtype_name", PRECISIONS)
@pytest.mark.parametrize("model", ["humanoid30", "mixed12"])
def test_limits_at_infinity_and_ranges_of_no_width(torch_cuda, model, dtype_name):
    """Rows without a lower limit, without an upper limit, with neither, with lower == upper, and finite ones; erp 50 and 0 (0 inf is
    no number), margin 0.25 and 0, both paths: parity, no NaN, and exactly 0 on the rows with neither limit."""
    torch = torch_cuda
    case = "inf:" + model
    hm = hip_model(model_of(model)[1])
    try:
        for erp in (50.0, 0.0):
            for margin in (MARGIN, 0.0):
                name, I, R = solved(case, NP_DTYPE[dtype_name], 3, margin=margin, erp=erp)
                neither = np.isinf(I["lower"]) & np.isinf(I["upper"])
                assert not R["bad"].any() and neither.any() and R["closed"][:, I["lower"] == I["upper"]].all() and np.abs(R["impulse"]).max() > 0.1
                for path in (1, 0):
                    set_path(hm, path)
                    for layout in (AOS, SOA):
                        label = f"{case} erp={erp} margin={margin} path={path} layout={layout} {dtype_name}"
                        v, p, r = hold_parity(torch, hm, name, I, R, B_WIDE, layout, dtype_name, 3, 0.0, label)
                        assert not p[:, torch.tensor(neither, device="cuda")].any(), label + ": a row with neither limit has an impulse"
    finally:
        set_path(hm, -1)


def test_an_infinite_state_is_nan_in_its_own_outputs_only(torch_cuda):
    """+inf in q of a listed joint and -inf in qd of a closed row, one configuration each, among rows with limits at infinity: NaN in all
    their outputs, every neighbour bit-identical."""
    torch = torch_cuda
    B, bad_rows = B_WIDE, [20, 33]
    for dtype_name in PRECISIONS:
        dtype = torch_dtype(torch, dtype_name)
        name, I, R = solved("inf:humanoid30", NP_DTYPE[dtype_name], 3)
        hm = hip_model(model_of(name)[1])
        first_closed = int(np.nonzero(R["closed"][bad_rows[1]])[0][0])
        for layout in (AOS, SOA):
            q, qd = device_state(torch, I, B, layout, dtype)
            good = [t.clone() for t in call(hm, q, qd, I, 3, layout)]
            q, qd = q.clone(), qd.clone()
            (q if layout == AOS else q.t())[bad_rows[0], int(R["c"][4])] = float("inf")
            (qd if layout == AOS else qd.t())[bad_rows[1], int(R["d"][first_closed])] = float("-inf")
            got = call(hm, q, qd, I, 3, layout)
            torch.cuda.synchronize()
            keep = torch.ones(B, dtype=torch.bool, device="cuda")
            keep[bad_rows] = False
            for g, w in zip(got, good):
                g, w = rows_of(g, B, layout), rows_of(w, B, layout)
                assert torch.isnan(g[bad_rows]).all(), f"layout={layout} {dtype_name}: a bad configuration has numbers in its outputs"
                assert not torch.isnan(w).any() and np.array_equal(bits(g[keep]), bits(w[keep])), f"layout={layout} {dtype_name}: a neighbour of a bad configuration changed"


@pytest.mark.parametrize("dtype_name", PRECISIONS)
@pytest.mark.parametrize("L", [32, 33, 64])
def test_the_fp32_lds_boundary_and_the_cap_on_the_comb(torch_cuda, L, dtype_name):
    """comb16x4, the list interleaved by depth (coupled rows 16 apart), its first 32 rows (the last length resident in fp32), 33 (the first
    streamed) and all 64 (the cap): 3 and 20 sweeps.  cond_kkt is 1e3 at most: the fp32 bound is 1e-2 relative, where on tree128 it is 1e2."""
    torch = torch_cuda
    for sweeps in (3, 20):
        name, I, R = solved(f"comb:{L}", NP_DTYPE[dtype_name], sweeps)
        assert not R["bad"].any() and R["cond_kkt"].max() < 3.0e3 and np.abs(R["impulse"]).max() > 0.1
        hm = hip_model(model_of(name)[1])
        for layout in (AOS, SOA):
            hold_parity(torch, hm, name, I, R, B_WIDE, layout, dtype_name, sweeps, 0.0, f"comb16x4 L={L} sweeps={sweeps} layout={layout} {dtype_name}")


@pytest.mark.parametrize("L,dtype_name", [(32, "f32"), (22, "f64")])
def test_resident_and_streamed_solves_of_the_comb_give_the_same_bits(torch_cuda, L, dtype_name):
    """the longest list whose triangle fits into LDS at either precision, each path forced"""
    torch = torch_cuda
    dtype = torch_dtype(torch, dtype_name)
    name, I, R = solved(f"comb:{L}", NP_DTYPE[dtype_name], 20)
    hm = hip_model(model_of(name)[1])
    try:
        for layout in (AOS, SOA):
            q, qd = device_state(torch, I, B_WIDE, layout, dtype)
            got = []
            for path in (1, 0):
                set_path(hm, path)
                got.append([t.clone() for t in call(hm, q, qd, I, 20, layout)])
            torch.cuda.synchronize()
            assert got[0][1].any() and not any(torch.isnan(t).any() for t in got[0])
            assert same_bits(got[0], got[1]), f"comb16x4 L={L} {dtype_name} layout={layout}: the two paths differ"
    finally:
        set_path(hm, -1)
