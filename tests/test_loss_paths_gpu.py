"""csrc/loss.hip path by path against the float64 formulas of tests/loss_reference.py (which tests/test_loss_reference_cpu.py
proves against torch's kl_div and the recorded outputs of the original project): every instantiation of the log-softmax
kernels and of the one-launch head loss, the label-smoothing / biased KL kernels on a table of special rows, the three autograd
nodes built on them, the token reduce, the REINFORCE terms and the sampler.  Every case asserts the path it is meant to reach
(V % 4, alignment, ld and the NV implied by V) and prints its figures before it asserts them (pytest -s).

Tolerances are not fixed numbers (the convention of tests/test_word_loss_gpu.py).  The yardstick is the SAME oracle formulas
(materialised distribution, torch autograd) evaluated in float32 on the device on the same inputs.  A kernel result may err
against float64 by twice the yardstick's error on the same quantity (on the same column class where classes are used) or by
2^-22 of that quantity's largest magnitude, whichever is larger; a bf16 output gets 2^-8 of the value on top (one rounding to
bf16 is 2^-9 relative).  No kernel of loss.hip is a yardstick for another.

One quantity has the factor 4 instead of 2: the amplitude term keep g raw in the gradient of the biased form (smooth_kl_bwd
with a sampled token).  W.r.t. the log-probs it sits at the row's sampled column alone, so only the class "sampled" has the
factor 4 there and the rest, target and pad classes, exactly -dist scale, keep 2; w.r.t. the logits it reaches every column
through the row sum G of the log-softmax backward, so all four classes have it.  raw = score p(a) n_row carries three roundings; g =
(log d_a + 1 - logp_a) - (log d_t + 1 - logp_t) is a difference of terms several times its own size, five roundings at their
magnitude; the product, the sum with -d_a and the scale add four: a dozen roundings of 2^-24 each, none of which the closed
form can avoid, against a bound of 2^-22 = four of them.  Measured: 2.25 ulp of the value at V = 7, pad 0, the a == pad row
(4.96e-8 against a yardstick of 2.29e-8, whose autograd forms the same quantities in another order and was 1.1 ulp off)."""
import functools
import math

import pytest
import torch

from tests import loss_cases as C
from tests import loss_reference as R

pytestmark = pytest.mark.gpu

SENT = -512.0                  # sentinel (exact in bf16 too)
EPS22 = 2.0 ** -22
NAN = float("nan")
WORST = {}                     # kernel -> [worst err / yardstick, worst err / bound]


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from bmhrl_amd import _lib
    _lib.load()  # must exist: the product has no fallback
    yield torch.device("cuda:0")
    print("\nworst figures per kernel: err / yardstick (yardstick floored at 2^-23 of the magnitude), err / bound")
    for k in sorted(WORST):
        print(f"  {k:28s} {WORST[k][0]:8.3f} {WORST[k][1]:8.3f}")


def check(kernel, what, got, ref, yard, cls=None, bf16=False, factor4=()):
    """got (device) against ref (float64, CPU) under the bound of the module docstring; yard: the float32 oracle's result;
    factor4: the column classes that have the factor 4 (module docstring), every other has 2"""
    ref = ref.detach().double().cpu()
    got = got.detach().double().cpu().reshape(ref.shape)
    yard = yard.detach().double().cpu().reshape(ref.shape)
    groups = [("all", torch.ones_like(ref, dtype=torch.bool))] if cls is None else \
        [(n, cls.cpu() == k) for k, n in enumerate(R.CLASS_NAMES)]
    bad = []
    for name, m in groups:
        if not bool(m.any()):
            continue
        r = ref[m]
        e_y, mag = float((yard[m] - r).abs().max()), float(r.abs().max())
        tol = max((4.0 if name in factor4 else 2.0) * e_y, EPS22 * mag)
        err = (got[m] - r).abs()
        allowed = tol + (2.0 ** -8 * r.abs() if bf16 else torch.zeros_like(r))
        ok = bool((err <= allowed).all())
        e = float(err.max())
        used = float(torch.where(err > 0, err / allowed.clamp_min(1e-300), torch.zeros_like(err)).max())
        vs_y = e / max(e_y, EPS22 * mag / 2, 1e-300) if not bf16 else float("nan")
        print(f"{kernel} | {what} [{name}]: err {e:.3e}  yardstick {e_y:.3e}  bound {tol:.3e}{' + 2^-8 |v|' if bf16 else ''}  "
              f"err/yardstick {vs_y:.2f}  err/bound {used:.2f}")
        w = WORST.setdefault(kernel, [0.0, 0.0])
        if vs_y == vs_y:
            w[0] = max(w[0], vs_y)
        w[1] = max(w[1], used if used == used else float("inf"))
        if not ok:
            bad.append((name, e, tol))
    assert not bad, (kernel, what, bad)


def rows_buf(dev, x, ld, off=0, fill=NAN):
    """x (rows, V) as a view with row stride ld of a `fill`-filled device buffer; the view starts `off` elements behind a
    16-byte boundary and the buffer has a tail behind the last row -> buffer, view"""
    rows, V = x.shape
    buf = torch.full((off + rows * ld + 8,), fill, device=dev, dtype=x.dtype)
    v = buf[off:off + rows * ld].view(rows, ld)[:, :V]
    v.copy_(x)
    assert buf.data_ptr() % 16 == 0 and v.data_ptr() == buf.data_ptr() + off * x.element_size()
    return buf, v


def slack_untouched(buf, v, ld, off=0, fill=NAN):
    """everything of the buffer outside the (rows, V) view still holds `fill`"""
    rows, V = v.shape
    keep = torch.ones(buf.numel(), dtype=torch.bool, device=buf.device)
    keep[off:off + rows * ld].view(rows, ld)[:, :V] = False
    rest = buf[keep]
    return bool(torch.isnan(rest).all()) if fill != fill else bool((rest == fill).all())


def pad8(n):
    return (n + 7) // 8 * 8


# ------------------------------------------------------------------------------------------------ log-softmax, fwd and bwd
def implied_nv(V, table):
    """the instantiation the dispatchers pick for a register-resident row: the smallest of `table` with 1024 NV >= V"""
    nv = (V + 1023) // 1024
    return next(t for t in table if nv <= t)


def vec_path(V, lds, ptrs16, ptrs8=()):
    """the NV of the vector kernels, or None for the scalar ones, from the conditions the dispatcher states"""
    ok = V % 4 == 0 and all(ld % 4 == 0 for ld in lds) and all(p % 16 == 0 for p in ptrs16) and all(p % 8 == 0 for p in ptrs8)
    return implied_nv(V, (1, 2, 4, 8, 12)) if ok and V <= 256 * 4 * 12 else None


# V, ld, offset of the base pointer in floats, the instantiation this case is for (None: the scalar kernels)
LSM_CASES = [(4, 4, 0, 1), (52, 52, 0, 1), (1028, 1028, 0, 2), (2052, 2052, 0, 4), (4100, 4100, 0, 8), (8196, 8196, 0, 12),
             (12288, 12288, 0, 12), (51, 51, 0, None), (12292, 12292, 0, None),
             (52, 54, 0, None), (52, 52, 1, None),                      # the two conditions that must send a call to the scalar kernel
             (52, 56, 0, 1), (1028, 1032, 0, 2), (51, 55, 0, None)]     # slack columns on both kinds of path


@pytest.mark.parametrize("V,ld,off,want", LSM_CASES)
def test_log_softmax_fwd_and_bwd_paths(dev, V, ld, off, want):
    from bmhrl_amd import ops
    rows = 5
    g = torch.Generator().manual_seed(V + ld + off)
    x = 3 * torch.randn(rows, V, generator=g)
    x[1] += 30.0                                                   # a row far from 0: the max subtraction matters
    buf, v = rows_buf(dev, x, ld, off)
    assert vec_path(V, [ld], [v.data_ptr()]) == want, "this case no longer reaches the path it is for"
    blockers = (V % 4 != 0, ld % 4 != 0, v.data_ptr() % 16 != 0, V > 12288)
    assert not any(blockers) if want else any(blockers)
    if V == 52:
        assert sum(blockers) == (want is None), "the V = 52 fallbacks are scalar for exactly one reason each"
    ops.log_softmax_(v, ld, rows, V)
    ref = torch.log_softmax(x.double(), -1)
    name = f"<{want}>" if want else " scalar"
    check(f"log_softmax{name}", f"V={V} ld={ld} off={off}", v, ref, torch.log_softmax(x.to(dev), -1))
    assert slack_untouched(buf, v, ld, off)
    # backward: bf16 d logits = dlogp - exp(logp) sum(dlogp); the log-probs are an input, so the oracle's logits are the log-probs
    lp = ref.float()
    d = torch.randn(rows, V, generator=g)
    (_, lpv), (_, dv) = rows_buf(dev, lp, ld, off), rows_buf(dev, d, ld, off)
    ldg = pad8(V) + 8
    gb = torch.full((rows, ldg), SENT, dtype=torch.bfloat16, device=dev)
    assert vec_path(V, [ld, ldg], [lpv.data_ptr(), dv.data_ptr()], [gb.data_ptr()]) == want
    ops.log_softmax_bwd(dv, lpv, ld, gb, ldg, rows, V)
    check(f"log_softmax_bwd{name}", f"V={V} ld={ld} off={off}", gb[:, :V], R.log_softmax_bwd(lp.double(), d.double()),
          R.log_softmax_bwd(lp.to(dev), d.to(dev)), bf16=True)
    assert bool((gb[:, V:] == SENT).all()), "padding columns of the bf16 output written"


# ------------------------------------------------------------------------------------------------ the KL kernels
S1, S2 = 0.37, 1.7             # loss_scale, loss_scale2


def f32(v):
    return float(torch.tensor(v, dtype=torch.float32))


@functools.lru_cache(maxsize=None)
def kl_refs(V, pad, variant, smoothing, zpr):
    """float64 results and float32-on-the-device yardsticks of every KL quantity of one case, computed once"""
    c = C.special_case(V, pad, variant)
    out = {}
    for tag, dt, where in (("ref", torch.float64, "cpu"), ("yard", torch.float32, "cuda:0")):
        lp = c["logp"].to(where, dt)
        trg, a = c["trg"].to(where), c["a"].to(where)
        sc, nr = c["score"].to(where, dt), c["n_row"].to(where, dt)
        o = {}
        o["rows_ls"], _ = R.kl_rows(lp, trg, None, None, None, smoothing, pad, zpr)
        o["rows_bkl"], o["amp"] = R.kl_rows(lp, trg, a, sc, nr, smoothing, pad, zpr)
        o["full_ls"] = R.divergence(lp, trg, None, None, smoothing, pad, zpr)
        o["full_bkl"] = R.divergence(lp, trg, a, o["amp"], smoothing, pad, zpr)
        for wl in (False, True):
            o[f"g_ls_{int(wl)}"] = R.kl_grad(lp, trg, None, None, None, smoothing, pad, zpr, 1.0, wl)
            o[f"g_bkl_{int(wl)}"] = R.kl_grad(lp, trg, a, sc, nr, smoothing, pad, zpr, 1.0, wl)
        o["e"] = R.kl_amp_grad(lp, trg, a, sc, nr, smoothing, pad, zpr)
        out[tag] = {k: t.detach().double().cpu() for k, t in o.items()}
    out["cls_ls"] = R.column_classes(V, c["trg"], None, pad)
    out["cls_bkl"] = R.column_classes(V, c["trg"], c["a"], pad)
    out["zeroed"] = R.zeroed_rows(c["trg"], pad, zpr)
    return out


KL_CASES = [(V, pad, variant) for V in (7, 300) for pad in (1, 0) for variant in C.VARIANTS] + \
    [(10172, 1, "row0"), (10172, 1, "later")]


@pytest.mark.parametrize("V,pad,variant", KL_CASES)
def test_kl_kernels_on_the_special_rows(dev, V, pad, variant):
    """smooth_kl_fwd (row sums, amp_out), smooth_kl_full, smooth_kl_bwd (both wrt, fp32 / bf16 outputs, loss_scale2, ldg > V) and
    smooth_kl_amp_grad, plain and biased, for smoothing x zero_pad_rows x ld; the slack columns hold NaN"""
    from bmhrl_amd import ops
    c = C.special_case(V, pad, variant)
    rows, i = len(C.SPECIAL_ROWS), c["index"]
    trg, a, sc, nr = (c[k].to(dev) for k in ("trg", "a", "score", "n_row"))
    s1, s12 = torch.tensor([S1], device=dev), torch.tensor([S2], device=dev)
    k1, k12 = f32(S1), f32(f32(S1) * f32(S2))
    ldg = pad8(V) + 8
    for smoothing in (0.7, 0.1):
        for zpr in (-1, 0, 1):
            K = kl_refs(V, pad, variant, smoothing, zpr)
            ref, yard = K["ref"], K["yard"]
            for ld in (V, V + 4):
                what = f"V={V} pad={pad} {variant} s={smoothing} zpr={zpr} ld={ld}"
                buf, lp = rows_buf(dev, c["logp"], ld)
                assert lp.stride(0) == ld and (ld == V or bool(torch.isnan(buf[V:ld]).all()))
                for tag, bt, s_, n_ in (("ls", None, None, None), ("bkl", a, sc, nr)):
                    cls = K[f"cls_{tag}"]
                    rl = torch.full((rows,), SENT, device=dev)
                    amp = torch.full((rows,), SENT, device=dev) if bt is not None else None
                    ops.smooth_kl_fwd(lp, ld, trg, bt, s_, n_, smoothing, pad, zpr, rl, amp, rows, V)
                    check(f"smooth_kl_fwd {tag}", what, rl, ref[f"rows_{tag}"], yard[f"rows_{tag}"])
                    if amp is not None:
                        check("smooth_kl_fwd amp_out", what, amp, ref["amp"], yard["amp"])
                        assert float(amp[i["raw_neg"]]) == 0.0 and float(amp[i["raw_gt1"]]) == 1.0 and float(amp[i["raw_eq1"]]) == 1.0
                    full = torch.full((rows, V), SENT, device=dev)
                    ops.smooth_kl_full(lp, ld, trg, bt, s_, n_, smoothing, pad, zpr, full, rows, V)
                    check(f"smooth_kl_full {tag}", what, full, ref[f"full_{tag}"], yard[f"full_{tag}"], cls)
                    for wl in (False, True):
                        r, y = ref[f"g_{tag}_{int(wl)}"], yard[f"g_{tag}_{int(wl)}"]
                        kn = f"smooth_kl_bwd {tag} wrt_{'logits' if wl else 'logp'}"
                        # (the amplitude term: see the module docstring)
                        fac = () if tag == "ls" else R.CLASS_NAMES if wl else ("sampled",)
                        # fp32 and bf16 together, bf16 behind ldg > V
                        gf = torch.full((rows, V), SENT, device=dev)
                        gb = torch.full((rows, ldg), SENT, dtype=torch.bfloat16, device=dev)
                        ops.smooth_kl_bwd(lp, ld, trg, bt, s_, n_, smoothing, pad, zpr, s1, gb, ldg, gf, rows, V, wrt_logits=wl)
                        check(kn, what + " f32 (both)", gf, r * k1, y * k1, cls, factor4=fac)
                        check(kn + " bf16", what + " (both)", gb[:, :V], r * k1, y * k1, cls, bf16=True, factor4=fac)
                        assert bool((gb[:, V:] == SENT).all())
                        # each alone, with loss_scale2 multiplied in
                        gf2 = torch.full((rows, V), SENT, device=dev)
                        ops.smooth_kl_bwd(lp, ld, trg, bt, s_, n_, smoothing, pad, zpr, s1, None, 0, gf2, rows, V, wrt_logits=wl,
                                          loss_scale2=s12)
                        check(kn, what + " f32 alone, loss_scale2", gf2, r * k12, y * k12, cls, factor4=fac)
                        gb2 = torch.full((rows, ldg), SENT, dtype=torch.bfloat16, device=dev)
                        ops.smooth_kl_bwd(lp, ld, trg, bt, s_, n_, smoothing, pad, zpr, s1, gb2, ldg, None, rows, V, wrt_logits=wl,
                                          loss_scale2=s12)
                        check(kn + " bf16", what + " alone, loss_scale2", gb2[:, :V], r * k12, y * k12, cls, bf16=True, factor4=fac)
                        assert bool((gb2[:, V:] == SENT).all())
                e = torch.full((rows,), SENT, device=dev)
                ops.smooth_kl_amp_grad(lp, ld, trg, a, sc, nr, smoothing, pad, zpr, e, rows, V)
                check("smooth_kl_amp_grad", what, e, ref["e"], yard["e"])
                dead = [i["raw_neg"], i["raw_gt1"], i["score0"]] + [r for r in range(rows) if bool(K["zeroed"][r])]
                assert all(float(e[r]) == 0.0 for r in dead), "gradient where the clamp is active or the row is zeroed"
                assert float(e[i["raw_eq1"]]) != 0.0, "raw == 1.0 lies on the closed interval: it carries gradient"
                assert slack_untouched(buf, lp, ld)


# ------------------------------------------------------------------------------------------------ the autograd nodes
@pytest.mark.parametrize("V,pad,variant", [(7, 1, "row0"), (300, 1, "later"), (300, 0, "row0")])
def test_given_amp_kl_node(dev, V, pad, variant):
    """functional.GivenAmpKLFn: value, d log-probs (amplitude held fixed) and d amplitude, for amplitudes 0, 0.3, 1 and random on
    every kind of row (the list is rotated over the rows)"""
    from bmhrl_amd.functional import GivenAmpKLFn
    c = C.special_case(V, pad, variant)
    rows, smoothing = len(C.SPECIAL_ROWS), 0.7
    B, S = 2, rows // 2
    g = torch.Generator().manual_seed(V)
    base = torch.tensor([0.0, 0.3, 1.0, 0.0, 1.0] + torch.rand(rows - 5, generator=g).tolist())
    drow = torch.randn(rows, generator=g)
    cls = R.column_classes(V, c["trg"], c["a"], pad)
    for shift in range(5):
        amp = torch.roll(base, shift)
        what = f"V={V} pad={pad} {variant} amp rotated by {shift}"
        r_rows, r_glp, r_gamp = R.given_amp(c["logp"].double(), c["trg"], c["a"], amp.double(), smoothing, pad, drow.double())
        y_rows, y_glp, y_gamp = R.given_amp(c["logp"].to(dev), c["trg"].to(dev), c["a"].to(dev), amp.to(dev), smoothing, pad, drow.to(dev))
        lp = c["logp"].to(dev).view(B, S, V).requires_grad_(True)
        am = amp.to(dev).view(B, S).requires_grad_(True)
        out = GivenAmpKLFn.apply(lp, c["trg"].to(dev).view(B, S), c["a"].to(dev).view(B, S), am, smoothing, pad)
        (out.view(-1) * drow.to(dev)).sum().backward()
        check("GivenAmpKLFn rows", what, out, r_rows, y_rows)
        # the kernels' given-amplitude form called directly: the unreduced divergence, the row sums and d rows / d amp
        from bmhrl_amd import ops
        lpd, t_, a_, am_ = c["logp"].to(dev), c["trg"].to(dev), c["a"].to(dev), amp.to(dev)
        full = torch.full((rows, V), SENT, device=dev)
        ops.smooth_kl_full(lpd, V, t_, a_, am_, None, smoothing, pad, -1, full, rows, V, amp_given=True)
        check("smooth_kl_full given amp", what, full, R.divergence(c["logp"].double(), c["trg"], c["a"], amp.double(), smoothing, pad),
              R.divergence(lpd, t_, a_, am_, smoothing, pad), cls)
        rl, e = torch.full((rows,), SENT, device=dev), torch.full((rows,), SENT, device=dev)
        ops.smooth_kl_fwd(lpd, V, t_, a_, am_, None, smoothing, pad, -1, rl, None, rows, V, amp_given=True)
        check("smooth_kl_fwd given amp", what, rl, r_rows, y_rows)
        ops.smooth_kl_amp_grad(lpd, V, t_, a_, am_, None, smoothing, pad, -1, e, rows, V, amp_given=True)
        check("smooth_kl_amp_grad given amp", what, e * drow.to(dev), r_gamp, y_gamp)
        with pytest.raises(ValueError, match="n_row is required"):
            ops.smooth_kl_fwd(lpd, V, t_, a_, am_, None, smoothing, pad, -1, rl, None, rows, V)      # n_row forgotten: an error
        check("GivenAmpKLFn d logp", what, lp.grad.view(rows, V), r_glp, y_glp, cls)
        check("GivenAmpKLFn d amp", what, am.grad.view(rows), r_gamp, y_gamp)


def test_manager_kl_node(dev):
    """functional.ManagerKLFn against manager_amplitude with autograd: B = 2, S = 7, segments of length 1 and 3 and a tail"""
    from bmhrl_amd.functional import ManagerKLFn
    B, S, V, pad, smoothing = 2, 7, 7, 1, 0.7
    g = torch.Generator().manual_seed(5)
    logp = torch.log_softmax(torch.randn(B, S, V, generator=g, dtype=torch.float64), -1).float()
    trg = torch.randint(2, 4, (B, S), generator=g)
    trg[1, 6] = pad                                                # a padded row in the tail (zeroed: its flat index is 13)
    a = torch.randint(4, V, (B, S), generator=g)
    a[0, 1] = trg[0, 1]
    seg = torch.tensor([[1, 0, 0, 1, 0, 0, 0], [0, 0, 1, 1, 0, 0, 0]], dtype=torch.int32)
    n_seg = torch.tensor([[2.0], [2.0]])
    amp64 = R.manager_amplitude(logp.double(), a, torch.ones(B, S, dtype=torch.float64), n_seg.double().view(B), seg)
    score = torch.rand(B, S, generator=g).double() * 1.6 / amp64.clamp_min(1e-3)     # raw in (0, 1.6): some clamped at 1
    score[0, 2] = -score[0, 2]                                     # and one clamped at 0
    score = score.float()
    drow = torch.randn(B * S, generator=g)
    r_rows, r_amp, r_g = R.manager_kl(logp.double(), trg.view(-1), a, score.double(), n_seg.double().view(B), seg, smoothing, pad, drow.double())
    assert int(((r_amp > 0) & (r_amp < 1)).sum()) >= 4 and int((r_amp == 1).sum()) >= 1 and bool((r_amp.view(B, S)[:, 4:] == 0).all())
    y_rows, y_amp, y_g = R.manager_kl(logp.to(dev), trg.view(-1).to(dev), a.to(dev), score.to(dev), n_seg.view(B).to(dev), seg, smoothing,
                                      pad, drow.to(dev))
    lp = logp.to(dev).requires_grad_(True)
    rows, amp = ManagerKLFn.apply(lp, trg.to(dev), a.to(dev), score.to(dev), n_seg.to(dev), seg.to(dev), smoothing, pad)
    (rows * drow.to(dev)).sum().backward()
    cls = R.column_classes(V, trg, a.view(-1), pad)
    check("ManagerKLFn rows", "B=2 S=7", rows, r_rows, y_rows)
    check("ManagerKLFn amplitude", "B=2 S=7", amp, r_amp, y_amp)
    check("ManagerKLFn d logp", "B=2 S=7", lp.grad.view(B * S, V), r_g.view(B * S, V), y_g.view(B * S, V), cls)


# ------------------------------------------------------------------------------------------------ the one-launch head loss
def head_case(rows, V, pad_rows, seed):
    g = torch.Generator().manual_seed(seed)
    x = 3 * torch.randn(rows, V, generator=g)
    trg = torch.randint(2, V, (rows,), generator=g)
    for r in pad_rows:
        trg[r] = 1
    return x, trg


def run_head_loss(dev, rows, V, want, pad_rows, weight, factor, dloss, ld, ldg):
    from bmhrl_amd import ops
    pad, smoothing = 1, 0.7
    x, trg = head_case(rows, V, pad_rows, seed=rows + V)
    what = f"rows={rows} V={V} pads={pad_rows} weight={weight} factor={factor} dloss={dloss} ld={ld} ldg={ldg}"
    w64 = None if weight is None else f32(weight)
    d64 = 1.0 if dloss is None else f32(dloss)
    ref = R.head_loss(x.double(), trg, smoothing, pad, w64, factor, d64)
    yard = R.head_loss(x.to(dev), trg.to(dev), smoothing, pad, w64, factor, d64)
    counter = torch.zeros(4, dtype=torch.int32, device=dev)
    wt = None if weight is None else torch.tensor([weight], device=dev)
    dl = None if dloss is None else torch.tensor(dloss, device=dev)
    t = trg.to(dev)
    for call in range(2):                                          # twice in a row: the kernel re-arms its counter words
        buf, v = rows_buf(dev, x, ld)
        rl = torch.full((rows,), SENT, device=dev)
        out = torch.full((2,), NAN, device=dev)
        gb = torch.full((rows, ldg), SENT, dtype=torch.bfloat16, device=dev)
        assert V % 4 == 0 and ld % 4 == 0 and ldg % 4 == 0 and v.data_ptr() % 16 == 0 and gb.data_ptr() % 8 == 0
        assert ops.head_loss_ok(V, ld, ldg) and implied_nv(V, (2, 4, 8, 12)) == want, "this case no longer reaches the path it is for"
        ops.head_loss(v, ld, t, smoothing, pad, wt, factor, dl, rl, out, gb, ldg, counter, rows, V)
        torch.cuda.synchronize()
        assert int(counter.abs().sum()) == 0, "counter words not back at zero"
        k = f"head_loss<{want}>"
        check(k + " logp", what, v, ref[0], yard[0])
        check(k + " rows", what, rl, ref[1], yard[1])
        check(k + " loss", what, out[0], ref[2], yard[2])
        check(k + " scale", what, out[1], torch.as_tensor(ref[3]), torch.as_tensor(yard[3]))
        check(k + " d logits bf16", what, gb[:, :V], ref[4], yard[4], R.column_classes(V, trg, None, pad), bf16=True)
        assert slack_untouched(buf, v, ld) and bool((gb[:, V:] == SENT).all())


HEAD_TABLE = [(4, 2), (52, 2), (1028, 2), (2052, 4), (4100, 8), (8196, 12), (12288, 12)]
PAD_ROWS = [(), (0,), (0, 2, 4)]


@pytest.mark.parametrize("V,want", HEAD_TABLE)
def test_head_loss_every_instantiation(dev, V, want):
    """against the float64 oracle: log-probs in place, row losses, loss, scale and the bf16 gradient; the arguments rotate with
    the pad-row pattern (test_head_loss_arguments crosses them at V = 52)"""
    for n, pad_rows in enumerate(PAD_ROWS):
        run_head_loss(dev, 5, V, want, pad_rows, weight=(None, 0.7, 1.3)[n], factor=(1.0, 0.2, 0.2)[n], dloss=(None, 1.25, None)[n],
                      ld=V + 4 * (n % 2), ldg=pad8(V) + 8 * (n > 0))


@pytest.mark.parametrize("pad_rows", PAD_ROWS)
def test_head_loss_arguments(dev, pad_rows):
    for weight in (None, 0.7):
        for factor in (1.0, 0.2):
            for dloss in (None, 1.25):
                for ld, ldg in ((52, 56), (56, 64)):
                    run_head_loss(dev, 6, 52, 2, pad_rows, weight, factor, dloss, ld, ldg)


def test_head_loss_counts_tokens_over_more_rows_than_threads(dev):
    run_head_loss(dev, 300, 8, 2, (0, 7, 255, 256, 299), 0.7, 0.2, 1.25, 8, 8)


# ------------------------------------------------------------------------------------------------ the token reduce
@pytest.mark.parametrize("weight", [None, 1.3])
@pytest.mark.parametrize("rows", [1, 255, 256, 300])
def test_token_loss_reduce(dev, rows, weight):
    from bmhrl_amd import ops
    g = torch.Generator().manual_seed(rows)
    rl = torch.rand(rows, generator=g) * 8 + 1
    trg = torch.randint(2, 50, (rows,), generator=g)
    trg[torch.rand(rows, generator=g) < 0.3] = 1
    trg[rows - 1] = 2                                              # at least one token, and it sits in the last row
    w = None if weight is None else torch.tensor([weight], device=dev)
    out = torch.full((2,), NAN, device=dev)
    ops.token_loss_reduce(rl.to(dev), trg.to(dev), rows, 1, w, 0.2, out[0:1], out[1:2])
    w64 = None if weight is None else f32(weight)
    ref = R.token_loss(rl.double(), trg, 1, w64, 0.2)
    yard = R.token_loss(rl.to(dev), trg.to(dev), 1, w64, 0.2)
    what = f"rows={rows} weight={weight}"
    check("token_loss_reduce loss", what, out[0], ref[0], yard[0])
    check("token_loss_reduce scale", what, out[1], ref[1], yard[1])


# ------------------------------------------------------------------------------------------------ REINFORCE
@pytest.mark.parametrize("extra", [0, 3])
def test_reinforce_fwd_and_bwd(dev, extra):
    from bmhrl_amd import ops
    c = C.reinforce_case()
    rows, V, ld = c["rows"], c["V"], c["V"] + extra
    act, val, cri = c["action"].to(dev), c["value"].to(dev), c["critic"].to(dev)
    for is_logp in (False, True):
        pred = torch.log(c["probs"]) if is_logp else c["probs"]
        buf, pv = rows_buf(dev, pred, ld)
        rp, rv = torch.full((rows,), SENT, device=dev), torch.full((rows,), SENT, device=dev)
        ops.reinforce_fwd(pv, ld, act, val, cri, rp, rv, rows, V, is_logp=is_logp)
        ref = R.reinforce(pred.double(), is_logp, c["action"], c["value"].double(), c["critic"].double())
        yard = R.reinforce(pred.to(dev), is_logp, act, val, cri)
        what = f"is_logp={is_logp} ld={ld}"
        check("reinforce_fwd policy", what, rp, ref[0], yard[0])
        check("reinforce_fwd value", what, rv, ref[1], yard[1])
        assert slack_untouched(buf, pv, ld)
    buf, pv = rows_buf(dev, c["probs"], ld)
    for gscale in (1.0, 2.5):
        ref = R.reinforce_grad(c["probs"].double(), c["action"], c["value"].double(), c["critic"].double(), gscale)
        yard = R.reinforce_grad(c["probs"].to(dev), act, val, cri, gscale)
        for want_v, want_c in ((True, True), (True, False), (False, True)):
            what = f"gscale={gscale} ld={ld} dvalue={want_v} dcritic={want_c}"
            dp = torch.full((rows, V), SENT, device=dev)
            vc = torch.full((2, rows), SENT, device=dev)           # dvalue | dcritic halves of ONE buffer: a null half keeps SENT
            ops.reinforce_bwd(pv, ld, act, val, cri, torch.tensor([gscale], device=dev), dp, vc[0] if want_v else None,
                              vc[1] if want_c else None, rows, V)
            check("reinforce_bwd d probs", what, dp, ref[0], yard[0])
            ga = torch.gather(dp, 1, act[:, None]).squeeze(1)
            assert float(ga[c["below"]]) == 0.0 and float(ga[c["above"]]) == 0.0
            assert float(ga[c["lower"]]) != 0.0 and float(ga[c["upper"]]) != 0.0, "the two boundary values carry gradient"
            for half, want, r, y, n in ((0, want_v, ref[1], yard[1], "d value"), (1, want_c, ref[2], yard[2], "d critic")):
                if want:
                    check("reinforce_bwd " + n, what, vc[half], r, y)
                else:
                    assert bool((vc[half] == SENT).all()), "the null output's neighbour was written"


# ------------------------------------------------------------------------------------------------ the sampler
@pytest.mark.parametrize("row_offset", [0, 1000])
@pytest.mark.parametrize("V", C.SAMPLER_V)
def test_sample_tokens_is_the_inverse_cdf_pick(dev, V, row_offset):
    """every token is the inverse-CDF pick of its row's uniform, within the fp32 error of the running sums (loss_reference
    sampler_tol); on the decided rows -- at least 90 % -- it IS the float64 pick.  ld in {V, V + 4}, seed_dev null and given
    (the effective seed is seed + the device word)."""
    from bmhrl_amd import ops
    lp, seed, ref_rows = C.sampler_case(V, row_offset)
    rows = C.SAMPLER_ROWS
    chunk = (V + 255) // 256
    assert chunk == {9: 1, 256: 1, 257: 2, 1000: 4, 10172: 40}[V]
    assert sum(1 for r in ref_rows if r[5]) >= 0.9 * rows
    word = torch.tensor([C.SAMPLER_DEV_WORD], dtype=torch.int64, device=dev)
    picks = []
    for ld in (V, V + 4):
        buf, v = rows_buf(dev, lp, ld)
        for seed_dev in (None, word):
            out = torch.full((rows,), -1, dtype=torch.int64, device=dev)
            p = torch.full((rows,), SENT, device=dev)
            ops.sample_tokens(v, ld, out, p, rows, V, False, seed if seed_dev is None else seed - C.SAMPLER_DEV_WORD, seed_dev, row_offset)
            o = out.cpu().tolist()
            worst, wrong = 0.0, []
            for r, (u, pick, cdf, total, tol, decided) in enumerate(ref_rows):
                c = o[r]
                assert 0 <= c < V
                lo = float(cdf[c - 1]) if c else 0.0
                worst = max(worst, (lo - u * total) / tol, (u * total - float(cdf[c])) / tol)
                if decided and c != pick:
                    wrong.append((r, c, pick))
            print(f"sample_tokens | V={V} ld={ld} row_offset={row_offset} seed_dev={'given' if seed_dev is not None else 'null'}: "
                  f"worst excursion past a cdf boundary {max(worst, 0.0):.3f} tol, {len(wrong)} decided rows off the float64 pick")
            w = WORST.setdefault("sample_tokens (sampling)", [0.0, 0.0])
            w[1] = max(w[1], worst)
            assert worst <= 1.0 and not wrong, (worst, wrong)
            want_p = torch.exp(torch.gather(lp.double(), 1, out.cpu()[:, None]).squeeze(1))
            check("sample_tokens p_out", f"V={V} ld={ld}", p, want_p, torch.exp(torch.gather(v, 1, out[:, None]).squeeze(1)))
            picks.append(o)
            assert slack_untouched(buf, v, ld)
    assert all(x == picks[0] for x in picks), "ld or the split of the seed changed a token"


@pytest.mark.parametrize("V", [9, 257, 1000])
def test_sample_tokens_greedy_is_the_first_maximum(dev, V):
    from bmhrl_amd import ops
    lp, want, _ = C.greedy_logp(V)
    rows = lp.shape[0]
    for ld in (V, V + 4):
        buf, v = rows_buf(dev, lp, ld)
        out = torch.full((rows,), -1, dtype=torch.int64, device=dev)
        p = torch.full((rows,), SENT, device=dev)
        ops.sample_tokens(v, ld, out, p, rows, V, True, 0)
        assert out.cpu().tolist() == want
        want_p = torch.exp(torch.gather(lp.double(), 1, torch.tensor(want)[:, None]).squeeze(1))
        check("sample_tokens greedy p_out", f"V={V} ld={ld}", p, want_p, torch.exp(torch.gather(v, 1, out[:, None]).squeeze(1)))


@pytest.mark.parametrize("V", [9, 257])
def test_greedy_pick_of_a_row_without_a_maximum_is_token_0(dev, V):
    """an all-NaN row (a diverged step) and an all -inf row have no entry above -inf: the token is 0, inside [0, V), and p_out =
    exp(logp[0]) still shows the NaN.  The log-probs are a view of a larger buffer (ld = V + 4 and a tail behind the last row).
    Only the token is asserted; it is fed to nothing."""
    from bmhrl_amd import ops
    g = torch.Generator().manual_seed(V)
    lp = torch.log_softmax(torch.randn(3, V, generator=g), -1)
    lp[0] = NAN
    lp[1] = -math.inf
    ld = V + 4
    buf, v = rows_buf(dev, lp, ld, fill=0.0)
    out = torch.full((3,), -1, dtype=torch.int64, device=dev)
    p = torch.full((3,), SENT, device=dev)
    ops.sample_tokens(v, ld, out, p, 3, V, True, 0)
    o = out.cpu().tolist()
    print(f"greedy without a maximum | V={V}: tokens {o}, p_out {p.cpu().tolist()}")
    assert all(0 <= t < V for t in o), "token outside [0, V)"
    assert o[0] == 0 and o[1] == 0 and o[2] == int(lp[2].argmax())
    assert math.isnan(float(p[0])) and float(p[1]) == 0.0
    assert abs(float(p[2]) - math.exp(float(lp[2, o[2]]))) <= 2.0 ** -22
