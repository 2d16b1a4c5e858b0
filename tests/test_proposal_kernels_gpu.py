"""The proposal kernels (bmhrl_amd/csrc/proposal.hip) on the MI355X: proposal_select against what the reference returned
(tests/golden/proposals.json + proposals.npz) and against tests/proposal_reference.select where the fixture cannot go (equal confidences, many
chunks), bit for bit; proposal_assign and proposal_head against the float64 restatement on the same fp32 inputs.

Bounds of the head.  With u = 2^-23: a sum s of terms t_i is held to |s - s64| <= C * u * sum|t_i| / n,
an element v to |v - v64| <= C * u * m, where m = |v64| for the predictions and, for dx, the sum of the absolute values of
the products v is a difference of (proposal_reference.dx_magnitude: sigmoid(c) - tx and l - tw cancel).  The worst ratios
measured on the MI355X over the nine shapes below were 0.99 (sums: with a handful of owned cells the error of a term, not of
the additions, is what shows), 1.39 (predictions: expf, a division and a product) and 2.26 (dx: the sigmoid, the difference
and three products); C = twice the worst, rounded up to a power of two: 2, 4 and 8.  Every test prints its ratios before it asserts."""
import numpy as np
import pytest
import torch

from tests import proposal_reference as R

pytestmark = pytest.mark.gpu

U = 2.0 ** -23
C_SUM, C_PRED, C_DX = 2.0, 4.0, 8.0
SHAPES = [(S, A) for S in (1, 7, 300) for A in (1, 3, 128)]


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from bmhrl_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def fixture_cases():
    return R.load_golden()


def bits(t):
    return (t.detach().cpu().contiguous().numpy() if isinstance(t, torch.Tensor) else np.ascontiguousarray(t)).view(np.uint32)


# ------------------------------------------------------------------------------------------------ proposal_select
def run_select(dev, pred, durations, k, thr):
    from bmhrl_amd import ops
    props, count = ops.proposal_select(torch.from_numpy(np.asarray(pred, dtype=np.float32)).to(dev),
                                       torch.tensor(durations, dtype=torch.float32, device=dev), k, thr)
    return props.cpu().numpy(), count.cpu().numpy()


def test_select_equals_the_reference_bit_for_bit(dev, fixture_cases):
    g = fixture_cases
    assert len(g["cases"]) == 30
    for case in g["cases"]:
        N, k, thr = case["N"], case["k"], case["nms_tiou"]
        props, count = run_select(dev, g["inputs"][N], g["durations"], k, thr)
        for b in range(3):
            want = case["postprocessed"][b] if thr is None else case["nms"][b]
            assert count[b] == len(want), (N, k, thr, b)
            assert np.array_equal(bits(props[b, :len(want)]), bits(want)), (N, k, thr, b)
            assert not bits(props[b, len(want):]).any(), (N, k, thr, b)         # zeros behind the survivors


def _random_pred(rng, B, N, dur):
    pred = np.empty((B, N, 3), dtype=np.float32)
    pred[:, :, 0] = rng.uniform(-2.0, dur + 2.0, (B, N))
    pred[:, :, 1] = rng.uniform(0.1, dur / 3, (B, N))
    pred[:, :, 2] = rng.uniform(0.0, 0.5, (B, N))
    return pred


def _restated_cases():
    rng = np.random.default_rng(11)
    cases = {}
    p = _random_pred(rng, 2, 300, 50.0)
    p[:, :, 2] = 0.25
    cases["all confidences equal"] = (p, 100, 0.5)
    p = _random_pred(rng, 2, 5000, 50.0)
    p[:, 4090:4102, 2] = 0.75                                   # the highest, equal, on both sides of a 4096-row chunk edge
    cases["equal across a chunk boundary"] = (p, 8, None)
    p = _random_pred(rng, 2, 70001, 50.0)
    for rows in (range(0, 40), range(35000, 35040), range(69961, 70001)):
        for r in rows:
            p[:, r, 2] = 0.5 + rng.uniform(0.0, 0.5, 2)
    p[0, 70000, 2] = p[0, 0, 2] = p[0, 35010, 2] = 0.999        # a tie of the first, a middle and the last row
    cases["top-k spread over the first, a middle and the last chunk"] = (p, 100, 0.7)
    cases["N < k"] = (_random_pred(rng, 3, 3, 50.0), 5, 0.9)
    cases["k = 1"] = (_random_pred(rng, 3, 4097, 50.0), 1, 0.4)
    cases["k at the maximum"] = (_random_pred(rng, 2, 9000, 50.0), 128, 0.6)
    cases["no suppression, k at the maximum"] = (_random_pred(rng, 1, 129, 50.0), 128, None)
    return cases


RESTATED = _restated_cases()


@pytest.mark.parametrize("name", list(RESTATED))
def test_select_equals_the_restatement(dev, name):
    from bmhrl_amd import ops
    pred, k, thr = RESTATED[name]
    assert k <= ops.PROPOSAL_MAX_K == 128
    durations = [50.0, 31.7, 44.0][:pred.shape[0]]
    want_props, want_count = R.select(pred, durations, k, thr)
    props, count = run_select(dev, pred, durations, k, thr)
    assert np.array_equal(count, want_count)
    assert np.array_equal(bits(props), bits(want_props))
    for b in range(pred.shape[0]):
        assert not bits(props[b, count[b]:]).any()
    again, count2 = run_select(dev, pred, durations, k, thr)
    assert np.array_equal(bits(again), bits(props)) and np.array_equal(count2, count)


def test_select_refuses_what_it_does_not_support(dev):
    from bmhrl_amd import _lib, ops
    lib = _lib.load()
    pred = torch.rand(2, 16, 3, device=dev)
    dur = torch.full((2,), 10.0, device=dev)
    props = torch.zeros(2, 128, 3, device=dev)
    count = torch.zeros(2, dtype=torch.int32, device=dev)
    P, D, O, Cn = pred.data_ptr(), dur.data_ptr(), props.data_ptr(), count.data_ptr()
    st = ops.stream()

    def call(pred_p=P, B=2, N=16, dur_p=D, k=4, props_p=O, count_p=Cn, ws=None, ws_n=0):
        return lib.bmhrl_proposal_select(pred_p, B, N, dur_p, k, 0.5, props_p, count_p, ws, ws_n, st)

    assert call() == 0
    assert call(k=0) == -22 and call(k=129) == -22 and call(N=0) == -22 and call(N=(1 << 24) + 1) == -22 and call(B=0) == -22
    assert call(pred_p=None) == -22 and call(dur_p=None) == -22 and call(props_p=None) == -22 and call(count_p=None) == -22
    assert call(N=5000) == -22                                  # more than one chunk needs the workspace
    torch.cuda.synchronize()
    for bad_k in (0, 129):
        with pytest.raises(_lib.HipError):
            ops.proposal_select(pred, dur, bad_k, 0.5)


# ------------------------------------------------------------------------------------------------ proposal_assign
CELL_SEC = 0.5


def make_targets(S, A, seed):
    """anchors (A) and targets (N, 4) for B = 3: two rows on one cell, a centre on a cell edge, one past the end, one below 0,
    equal-tIoU anchors (a duplicated anchor length), random rows; video 2 has no target"""
    rng = np.random.default_rng(seed)
    anchors = np.sort(rng.uniform(0.5, 40.0, A)).astype(np.float32)
    if A >= 3:
        anchors[A // 2 + 1] = anchors[A // 2]                    # two equal anchors: equal tIoU with every target
    mid = float(anchors[A // 2])
    c = S // 2
    rows = [
        [0, (c + 0.25) * CELL_SEC, mid * 1.1, 0],               # same video, cell and anchor as the next row, ...
        [0, (c + 0.5) * CELL_SEC, mid * 1.1, 1],                # ... which owns the cell (the larger row)
        [1, (S - 1) * CELL_SEC, float(anchors[0]) * 0.9, 2],    # exactly on a cell edge
        [1, (S + 0.5) * CELL_SEC, mid, 3],                      # past the last cell: skipped
        [1, -0.25 * CELL_SEC, mid, 4],                          # below 0: skipped
        [1, (S - 1 + 0.75) * CELL_SEC, mid, 5],                 # its length IS the duplicated anchor: the smaller index
    ]
    for j in range(6):
        rows.append([int(rng.integers(0, 2)), float(rng.uniform(0, S * CELL_SEC)), float(rng.uniform(0.3, 50.0)), 6 + j])
    return torch.from_numpy(anchors), torch.tensor(rows, dtype=torch.float32)


@pytest.mark.parametrize("S,A", SHAPES)
def test_assign_against_the_restatement(dev, S, A):
    from bmhrl_amd import ops
    anchors, targets = make_targets(S, A, seed=S * 1000 + A)
    owner64, tx64, tw64, counts64, best = R.assign(targets, anchors, CELL_SEC, 3, S)
    if A >= 3:
        assert best[5] == A // 2                                  # the tie went to the smaller of the two equal anchors
    assert best[0] == best[1] and not (owner64 == 0).any()     # row 1 took row 0's cell (a later row may have taken it again)
    assert (owner64[2] == -1).all() and not (owner64 == 3).any() and not (owner64 == 4).any()
    owner, tx, tw, counts = ops.proposal_assign(targets.to(dev), anchors.to(dev), CELL_SEC, 3, S)
    assert owner.dtype == torch.int32 and tuple(owner.shape) == (3, A, S)
    assert torch.equal(owner.cpu().long(), owner64)
    assert counts.cpu().tolist() == counts64 and sum(counts64) == 3 * A * S
    # tx = g - floor(g) is exact in fp32.  tw: the argument of the log is an fp32 quotient of the two fp32 quotients (relative
    # 2^-24, which the log turns into an absolute 2^-24), logf is good to about 2 ulp and its result is rounded once more
    assert torch.equal(tx.cpu().double(), tx64)
    err = (tw.cpu().double() - tw64).abs()
    bound = 2.0 ** -23 + 4 * 2.0 ** -24 * tw64.abs()
    print(f"assign S={S} A={A}: worst tw error / bound = {float((err / bound).max()):.3f}")
    assert (err <= bound).all()
    again = ops.proposal_assign(targets.to(dev), anchors.to(dev), CELL_SEC, 3, S)
    assert all(torch.equal(a, b) for a, b in zip((owner, tx, tw, counts), again))


def test_assign_without_targets_and_bad_arguments(dev):
    from bmhrl_amd import _lib, ops
    anchors = torch.tensor([1.0, 2.0], device=dev)
    owner, tx, tw, counts = ops.proposal_assign(torch.zeros(0, 4, device=dev), anchors, CELL_SEC, 2, 5)
    assert (owner == -1).all() and counts.tolist() == [0, 20] and tx.numel() == 0
    lib = _lib.load()
    o, c = owner.data_ptr(), counts.data_ptr()
    assert lib.bmhrl_proposal_assign(None, 0, anchors.data_ptr(), 2, 0.5, 2, 5, o, None, None, c, ops.stream()) == 0
    assert lib.bmhrl_proposal_assign(None, 1, anchors.data_ptr(), 2, 0.5, 2, 5, o, None, None, c, ops.stream()) == -22
    assert lib.bmhrl_proposal_assign(None, 0, None, 2, 0.5, 2, 5, o, None, None, c, ops.stream()) == -22
    assert lib.bmhrl_proposal_assign(None, 0, anchors.data_ptr(), 2, 0.0, 2, 5, o, None, None, c, ops.stream()) == -22
    assert lib.bmhrl_proposal_assign(None, 0, anchors.data_ptr(), 2, 0.5, 2, 0, o, None, None, c, ops.stream()) == -22
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ proposal_head
def head_case(S, A, with_targets=True, seed=0):
    gen = torch.Generator().manual_seed(seed + S * 131 + A)
    B = 3
    x = torch.randn(B, S, 3 * A, generator=gen)
    x.view(B, S, A, 3)[..., 2] = (torch.rand(B, S, A, generator=gen) * 60 - 30)      # |o| up to 30: the stable softplus matters
    anchors, targets = make_targets(S, A, seed=S * 1000 + A)
    if not with_targets:
        targets = targets[:0]
    owner64, tx64, tw64, counts, _ = R.assign(targets, anchors, CELL_SEC, B, S)
    tx32, tw32 = tx64.float(), tw64.float()                     # the SAME fp32 inputs go to the kernel and to the restatement
    return x, anchors, owner64, tx32, tw32, counts


def run_head(dev, x, anchors, owner64, tx32, tw32, counts, dscale=None, pad=64, obj_coeff=1.0, noobj_coeff=100.0):
    from bmhrl_amd import ops
    B, S, A3 = x.shape
    A = A3 // 3
    sentinel = -12345.0
    buf = torch.full((pad + x.numel() + pad,), sentinel, device=dev)
    dx = buf[pad:pad + x.numel()].view(B, S, A3)
    n_total, off = A * S + 7, 3
    pred = torch.full((B, n_total, 3), sentinel, device=dev)
    assigned = (owner64.to(torch.int32).to(dev), tx32.to(dev), tw32.to(dev), torch.tensor(counts, dtype=torch.int32, device=dev))
    sums = ops.proposal_head(x.to(dev), anchors.to(dev), CELL_SEC, pred, off, assigned, obj_coeff, noobj_coeff, dx=dx,
                             dscale=None if dscale is None else torch.tensor([dscale], device=dev))
    assert (buf[:pad] == sentinel).all() and (buf[pad + x.numel():] == sentinel).all()        # nothing outside dx
    assert (pred[:, :off] == sentinel).all() and (pred[:, off + A * S:] == sentinel).all()    # nothing outside the head's rows
    return pred[:, off:off + A * S].cpu(), sums.cpu(), dx.cpu().clone()


def restated_head(x, anchors, owner64, tx32, tw32, obj_coeff=1.0, noobj_coeff=100.0):
    x64 = x.double().requires_grad_(True)
    assigned = (owner64, tx32.double(), tw32.double())
    pred, sums, mags = R.head(x64, anchors.double(), CELL_SEC, assigned, obj_coeff, noobj_coeff)
    sums[4].backward()
    return pred.detach(), sums.detach(), mags, x64.grad, R.dx_magnitude(x64, anchors.double(), assigned, obj_coeff, noobj_coeff)


def check_head(tag, got, want):
    pred, sums, dx = got
    pred64, sums64, mags, dx64, dx_mag = want
    r_pred = float(((pred.double() - pred64).abs() / (U * pred64.abs() + 1e-37)).max())
    r_sum = float(((sums.double() - sums64).abs() / (U * mags + 1e-37)).max())
    r_dx = float(((dx.double() - dx64).abs() / (U * dx_mag.abs() + 1e-37)).max())
    print(f"head {tag}: error / (2^-23 * magnitude): predictions {r_pred:.3f}  sums {r_sum:.3f}  dx {r_dx:.3f}")
    assert torch.isfinite(dx).all() and torch.isfinite(sums).all()
    assert r_pred <= C_PRED and r_sum <= C_SUM and r_dx <= C_DX


@pytest.mark.parametrize("S,A", SHAPES)
def test_head_against_the_float64_restatement(dev, S, A):
    x, anchors, owner64, tx32, tw32, counts = head_case(S, A)
    got = run_head(dev, x, anchors, owner64, tx32, tw32, counts)
    check_head(f"S={S} A={A}", got, restated_head(x, anchors, owner64, tx32, tw32))
    again = run_head(dev, x, anchors, owner64, tx32, tw32, counts)
    assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(got, again))                  # two runs, equal bits


def test_head_coefficients_and_gradient_scale(dev):
    x, anchors, owner64, tx32, tw32, counts = head_case(7, 3, seed=5)
    got = run_head(dev, x, anchors, owner64, tx32, tw32, counts, dscale=0.5, obj_coeff=2.0, noobj_coeff=30.0)
    pred64, sums64, mags, dx64, dx_mag = restated_head(x, anchors, owner64, tx32, tw32, 2.0, 30.0)
    check_head("coefficients 2 / 30, dscale 0.5", got, (pred64, sums64, mags, 0.5 * dx64, 0.5 * dx_mag))


@pytest.mark.parametrize("S,A", [(7, 3), (300, 128)])
def test_head_without_any_owned_cell(dev, S, A):
    """n_obj == 0: the three object terms and their gradients are 0, not NaN"""
    x, anchors, owner64, tx32, tw32, counts = head_case(S, A, with_targets=False)
    assert counts[0] == 0
    pred, sums, dx = got = run_head(dev, x, anchors, owner64, tx32, tw32, counts)
    assert sums[:3].tolist() == [0.0, 0.0, 0.0] and float(sums[3]) > 0 and torch.isfinite(sums).all()
    d = dx.view(3, S, A, 3)
    assert (d[..., 0] == 0).all() and (d[..., 1] == 0).all() and torch.isfinite(dx).all()
    check_head(f"no target, S={S} A={A}", got, restated_head(x, anchors, owner64, tx32, tw32))


def test_head_inference_writes_predictions_only(dev):
    from bmhrl_amd import _lib, ops
    x, anchors, owner64, tx32, tw32, counts = head_case(7, 3)
    trained, _, _ = run_head(dev, x, anchors, owner64, tx32, tw32, counts)
    xd, ad = x.to(dev), anchors.to(dev)
    pred = torch.zeros(3, 21, 3, device=dev)
    assert ops.proposal_head(xd, ad, CELL_SEC, pred, 0) is None
    assert np.array_equal(bits(pred), bits(trained))            # the same predictions with and without targets
    # the C entry point itself: a loss slice passed in inference mode is left as it was; a gradient is refused
    sums = torch.full((5,), 7.0, device=dev)
    lib = _lib.load()
    args = lambda dx: (xd.data_ptr(), ad.data_ptr(), CELL_SEC, 3, 7, 3, pred.data_ptr(), 21, 0, None, None, None, None, 1.0, 100.0,
                       None, dx, sums.data_ptr(), None, None, ops.stream())
    assert lib.bmhrl_proposal_head(*args(None)) == 0
    assert sums.tolist() == [7.0] * 5
    assert lib.bmhrl_proposal_head(*args(torch.zeros_like(xd).data_ptr())) == -22
    bad_off = list(args(None))
    bad_off[8] = 1                                              # rows 1 .. 21 of a 21-row tensor
    assert lib.bmhrl_proposal_head(*bad_off) == -22
    with pytest.raises(ValueError):
        ops.proposal_head(xd, ad, CELL_SEC, pred, 0, dx=torch.zeros_like(xd))
