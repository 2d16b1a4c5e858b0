"""tests/loss_reference.py against torch.nn.functional.kl_div on an independently built distribution, against the outputs
recorded from the original project (tests/golden/losses.npz, kat.npz) and against hash values written out by hand; and the
conditions that tests/test_loss_paths_gpu.py relies on, checked here because they need no GPU: every row of the special-row
table is the case its name says (in float64), and the sampler inputs leave at least 90 % of the rows decided.

Bounds: float64 against float64 agrees to rounding, 1e-12 relative.  The recorded outputs are float32 results of float32
arithmetic: 1e-5 of the largest entry, the bound the recorded cases have always been held to."""
import pytest
import torch
import torch.nn.functional as F

from tests import loss_cases as C
from tests import loss_reference as R

TOL64 = 1e-12
TOL_RECORDED = 1e-5


def rel(a, b, floor=1e-30):
    a, b = torch.as_tensor(a).double(), torch.as_tensor(b).double()
    return float((a - b).abs().max() / max(float(b.abs().max()), floor))


def _dist_by_loops(V, trg, a, amp, smoothing, pad, zero_rows):
    """the target distribution written entry by entry, independently of loss_reference.target_distribution"""
    d = torch.zeros(len(trg), V, dtype=torch.float64)
    for r in range(len(trg)):
        for c in range(V):
            d[r, c] = smoothing / (V - 2)
        d[r, int(trg[r])] = (1 - smoothing) * (1 - (float(amp[r]) if a is not None else 0.0))
        d[r, pad] = 0.0
        if a is not None:
            d[r, int(a[r])] += (1 - smoothing) * float(amp[r])
        if r in zero_rows:
            d[r] = 0.0
    return d + 1e-8 if a is not None else d


@pytest.mark.parametrize("trg,zero_rows", [([1, 4, 2, 5, 3], ()), ([1, 4, 1, 5, 3], (0, 2)), ([2, 1, 3, 4, 1], (1, 4)), ([2, 3, 4, 5, 6], ())])
@pytest.mark.parametrize("biased", [False, True])
def test_divergence_is_kl_div_of_the_materialised_distribution(trg, zero_rows, biased):
    """incl. the guard: a padded row 0 alone is not zeroed; with another padded row both are"""
    V, pad, smoothing = 7, 1, 0.7
    g = torch.Generator().manual_seed(len(zero_rows))
    logp = torch.log_softmax(torch.randn(5, V, generator=g, dtype=torch.float64), -1)
    trg = torch.tensor(trg)
    a = torch.tensor([3, 4, 1, 0, 6]) if biased else None            # a == t in row 1, a == pad in row 2
    amp = torch.tensor([0.0, 0.3, 1.0, 0.25, 0.6], dtype=torch.float64) if biased else None
    want = F.kl_div(logp, _dist_by_loops(V, trg, a, amp, smoothing, pad, zero_rows), reduction="none")
    got = R.divergence(logp, trg, a, amp, smoothing, pad)
    assert rel(got, want) < TOL64
    assert R.zeroed_rows(trg, pad).tolist() == [r in zero_rows for r in range(5)]
    # the override: 1 zeroes every padded row, 0 none
    padded = [int(t) == pad for t in trg]
    assert R.zeroed_rows(trg, pad, 1).tolist() == padded and not R.zeroed_rows(trg, pad, 0).any()
    for z in (0, 1):
        want = F.kl_div(logp, _dist_by_loops(V, trg, a, amp, smoothing, pad, [r for r in range(5) if padded[r] and z]), reduction="none")
        assert rel(R.divergence(logp, trg, a, amp, smoothing, pad, z), want) < TOL64


def test_recorded_random_case(golden):
    """losses.npz: 21 rows, V = 37, smoothing 0.7, pad 1 -- divergences, amplitudes, d / d logits, REINFORCE and its gradient"""
    g = golden("losses")
    T = lambda k: torch.from_numpy(g[k])
    logits, trg, a = T("logits").double(), T("trg"), T("sampled").reshape(-1)
    B, S, V = logits.shape
    rows = B * S
    x = logits.reshape(rows, V)
    logp = torch.log_softmax(x, -1)
    n_tok = float((trg != 1).sum())
    assert rel(R.divergence(logp, trg, None, None, 0.7, 1), T("ls")) < TOL_RECORDED
    assert rel(R.kl_grad(x, trg, None, None, None, 0.7, 1, scale=1 / n_tok, wrt_logits=True), T("ls_grad_logits").reshape(rows, V)) < TOL_RECORDED
    mask = trg != 1
    n_row = mask.sum(-1, keepdim=True).expand(B, S).reshape(-1).double()
    for tag in ("raw", "stab"):
        sc = ((T("score") - T("baseline")) * mask.float() if tag == "stab" else T("score")).reshape(-1).double()
        _, amp = R.amplitude(logp, a, sc, n_row)
        assert rel(amp, T(f"bkl_{tag}_amp").reshape(-1)) < TOL_RECORDED
        assert rel(R.divergence(logp, trg, a, amp, 0.7, 1), T(f"bkl_{tag}")) < TOL_RECORDED
        got = R.kl_grad(x, trg, a, sc, n_row, 0.7, 1, scale=1 / (n_tok * 0.2), wrt_logits=True)
        assert rel(got, T(f"bkl_{tag}_grad_logits").reshape(rows, V)) < TOL_RECORDED
    xr = x.clone().requires_grad_(True)
    rp, rv = R.reinforce(torch.softmax(xr, -1), False, a, T("score").reshape(-1).double(), T("baseline").reshape(-1).double())
    loss = rp.mean() + rv.mean()
    loss.backward()
    assert rel(loss.detach(), T("reinforce")) < TOL_RECORDED
    assert rel(xr.grad, T("reinforce_grad_logits").reshape(rows, V)) < TOL_RECORDED
    # the gradient w.r.t. the probabilities, by the helper, pulled back through the softmax by hand-free autograd
    p = torch.softmax(x, -1).requires_grad_(True)
    dp, _, _ = R.reinforce_grad(p, a, T("score").reshape(-1).double(), T("baseline").reshape(-1).double())
    xs = x.clone().requires_grad_(True)
    torch.softmax(xs, -1).backward(dp)
    assert rel(xs.grad, xr.grad) < TOL64


def test_recorded_appendix_cases(golden):
    """kat.npz: the 6 x 6 cases incl. the index-sum guard (the only padded flat index is 0) and a given amplitude"""
    k = golden("kat")
    lp = torch.from_numpy(k["a4_lp"]).double().reshape(6, 6)
    assert rel(R.divergence(lp, torch.tensor([2, 4, 1, 5, 3, 2]), None, None, 0.7, 1), k["a4_ls"]) < TOL_RECORDED
    assert rel(R.divergence(lp, torch.tensor([1, 4, 2, 5, 3, 2]), None, None, 0.7, 1), k["a4_ls_guard"]) < TOL_RECORDED
    amp = torch.tensor([.5, .25, 1., .8, 0., .1], dtype=torch.float64)
    a = torch.tensor([2, 0, 3, 1, 3, 4])
    assert rel(R.divergence(lp, torch.tensor([2, 4, 1, 5, 3, 2]), a, amp, 0.7, 1), k["a4_bkl"]) < TOL_RECORDED
    rp, rv = R.reinforce(torch.exp(lp), False, a, torch.tensor([.1, .2, .3, .4, .5, .6], dtype=torch.float64),
                         torch.tensor([.3, .1, .0, .2, .2, .9], dtype=torch.float64))
    assert rel(rp.mean() + rv.mean(), k["a4_reinforce"]) < TOL_RECORDED
    rp2, _ = R.reinforce(lp, True, a, torch.tensor([.1, .2, .3, .4, .5, .6], dtype=torch.float64),
                         torch.tensor([.3, .1, .0, .2, .2, .9], dtype=torch.float64))
    assert rel(rp2, rp) < TOL64


def test_uniform01_is_the_hash_of_common_h():
    """z = idx * 0x9E3779B97F4A7C15 + seed; two xorshift-multiply rounds (>> 30, * 0xBF58476D1CE4E5B9; >> 27,
    * 0x94D049BB133111EB); z ^= z >> 31; the top 32 bits.  (0, 1) is the first output of splitmix64 from state 0,
    0xE220A8397B1DCDAF; the others were worked out with 64-bit unsigned arithmetic."""
    for seed, idx, h in [(0, 0, 0x00000000), (0, 1, 0xE220A839), (1, 0, 0x5692161D), (123, 7, 0xFFFC0AE2),
                         (0xFFFFFFFFFFFFFFFF, 5, 0xB4A0472E), (100000, 1063, 0x814B258F)]:
        assert R.hash_u32(seed, idx) == h
        assert R.uniform01(seed, idx) == (h >> 8) / 16777216.0 and 0.0 <= R.uniform01(seed, idx) < 1.0
    assert R.uniform01(1, 0) == 5673494 / 16777216.0
    # the effective seed wraps like the device's 64-bit addition
    assert R.uniform01((1 << 64) + 123, 7) == R.uniform01(123, 7)


def test_inverse_cdf_picks_the_first_column_above_u():
    lp = torch.log(torch.tensor([0.1, 0.2, 0.0, 0.3, 0.4], dtype=torch.float64))
    for u, want in [(0.0, 0), (0.0999, 0), (0.1001, 1), (0.2999, 1), (0.3001, 3), (0.61, 4), (0.9999, 4)]:
        pick, cdf, total = R.inverse_cdf(lp, u)
        assert pick == want and abs(total - 1.0) < 1e-15 and cdf.shape == (5,)


def test_manager_amplitude_on_a_case_written_out():
    """B = 1, S = 5: segments of length 2 and 1, then a tail"""
    p = torch.tensor([[0.5, 0.25, 0.1, 0.9, 0.8]], dtype=torch.float64)
    V = 4
    a = torch.tensor([[0, 1, 2, 3, 0]])
    logp = torch.full((1, 5, V), -9.0, dtype=torch.float64)
    logp.scatter_(2, a.unsqueeze(-1), torch.log(p).unsqueeze(-1))
    score = torch.tensor([[1.0, 2.0, 3.0, 4.0, 5.0]], dtype=torch.float64)
    seg = torch.tensor([[0, 1, 1, 0, 0]])
    got = R.manager_amplitude(logp, a, score, torch.tensor([2.0], dtype=torch.float64), seg)
    want = torch.tensor([[1.0 * 0.125 * 2, 2.0 * 0.125 * 2, 3.0 * 0.1 * 2, 0.0, 0.0]], dtype=torch.float64)
    assert rel(got, want) < TOL64


@pytest.mark.parametrize("variant", C.VARIANTS)
@pytest.mark.parametrize("pad", [1, 0])
@pytest.mark.parametrize("V", [7, 300, 10172])
def test_special_rows_are_the_cases_they_name(V, pad, variant):
    c = C.special_case(V, pad, variant)
    i, trg, a = c["index"], c["trg"], c["a"]
    raw, amp = R.amplitude(c["logp"].double(), a, c["score"].double(), c["n_row"].double())
    assert set(i) == set(C.SPECIAL_ROWS) and len(trg) == len(C.SPECIAL_ROWS)
    assert int(trg[0]) == pad and i["t_pad_row0"] == 0
    padded = [r for r in range(len(trg)) if int(trg[r]) == pad]
    if variant == "row0":
        assert padded == [0] and int(a[0]) == pad and not R.zeroed_rows(trg, pad).any()             # guard off
    else:
        assert padded == [0, i["last"]] and int(a[0]) != pad and int(a[i["last"]]) == pad
        assert R.zeroed_rows(trg, pad).tolist() == [r in padded for r in range(len(trg))]           # guard on
    assert int(a[i["a_eq_t"]]) == int(trg[i["a_eq_t"]]) != pad
    assert int(a[i["a_eq_pad"]]) == pad != int(trg[i["a_eq_pad"]])
    assert float(raw[i["raw_neg"]]) < 0 and float(amp[i["raw_neg"]]) == 0.0
    assert float(raw[i["raw_gt1"]]) > 1 and float(amp[i["raw_gt1"]]) == 1.0
    assert float(c["score"][i["score0"]]) == 0.0 and float(raw[i["score0"]]) == 0.0
    assert float(raw[i["raw_eq1"]]) == 1.0 and float(c["logp"][i["raw_eq1"], a[i["raw_eq1"]]]) == 0.0
    for name in ("a_eq_t", "a_eq_pad", "inside", "ordinary", "t_pad_row0", "last"):
        assert 0.0 < float(raw[i[name]]) < 1.0, name
    for name in ("raw_neg", "raw_gt1", "score0", "raw_eq1", "ordinary", "inside"):                  # three distinct special columns
        r = i[name]
        assert len({int(trg[r]), int(a[r]), 0, 1}) == 4, name
    # what the clamp does to the amplitude gradient, by autograd: none outside [0, 1], some on the closed upper edge
    e = R.kl_amp_grad(c["logp"].double(), trg, a, c["score"].double(), c["n_row"].double(), 0.7, pad)
    assert float(e[i["raw_neg"]]) == 0.0 and float(e[i["raw_gt1"]]) == 0.0 and float(e[i["score0"]]) == 0.0
    assert abs(float(e[i["raw_eq1"]])) > 1.0 and abs(float(e[i["inside"]])) > 1e-3
    assert float(e[i["a_eq_t"]]) == pytest.approx(0.0, abs=1e-12)         # the target loses what the sampled token gains
    if variant == "later":
        assert float(e[0]) == 0.0 and float(e[i["last"]]) == 0.0           # zeroed rows


@pytest.mark.parametrize("row_offset", [0, 1000])
@pytest.mark.parametrize("V", C.SAMPLER_V)
def test_sampler_inputs_leave_nine_rows_in_ten_decided(V, row_offset):
    """a row is decided when u total lies more than tol from every cdf boundary: there every correct fp32 sampler returns the
    float64 pick.  u is computed on the host, so the condition is checked here on the inputs the GPU test uses."""
    lp, seed, rows = C.sampler_case(V, row_offset)
    assert lp.shape == (C.SAMPLER_ROWS, V) and seed > C.SAMPLER_DEV_WORD
    decided = sum(1 for r in rows if r[5])
    print(f"V={V} row_offset={row_offset} seed={seed}: {decided} of {len(rows)} rows decided")
    assert decided >= 0.9 * len(rows)
    for u, pick, cdf, total, tol, _ in rows:
        assert 0 <= pick < V and float(cdf[pick]) > u * total and (pick == 0 or float(cdf[pick - 1]) <= u * total)


@pytest.mark.parametrize("V", [9, 257, 1000])
def test_greedy_inputs_hold_their_duplicated_maxima(V):
    lp, want, chunk = C.greedy_logp(V)
    assert chunk == (V + 255) // 256
    m = [torch.nonzero(r == r.max()).reshape(-1).tolist() for r in lp]
    assert len(m[0]) == 2 and m[0][0] // chunk != m[0][1] // chunk        # in two threads' chunks
    assert m[1][0] // chunk == m[1][-1] // chunk and len(m[1]) == (2 if chunk > 1 else 1)
    assert m[3] == [0, V - 1] and len(m[4]) == V
    assert [x[0] for x in m] == want


def test_reinforce_inputs_sit_where_they_are_meant_to():
    c = C.reinforce_case()
    pa = torch.gather(c["probs"], 1, c["action"][:, None]).squeeze(1).double()
    assert float(pa[c["below"]]) < R.REINFORCE_LO == float(pa[c["lower"]]) < float(pa[c["inside"]]) < R.REINFORCE_HI == float(pa[c["upper"]])
    assert float(pa[c["above"]]) > R.REINFORCE_HI
    dp, dv, dc = R.reinforce_grad(c["probs"].double(), c["action"], c["value"].double(), c["critic"].double())
    ga = torch.gather(dp, 1, c["action"][:, None]).squeeze(1)
    assert float(ga[c["below"]]) == 0.0 and float(ga[c["above"]]) == 0.0
    assert float(ga[c["lower"]]) != 0.0 and float(ga[c["upper"]]) != 0.0    # the closed interval carries gradient
    assert int((dp != 0).sum()) == c["rows"] - 2 and rel(dv, -dc) < TOL64
