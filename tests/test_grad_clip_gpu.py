"""Gradient-norm clipping and the device-resident learning rate on the GPU: bmhrl_grad_norm against float64, the _dev Adam
entry points against the existing ones (bit for bit), and the trainer -- eager, captured, with the side-stream experiments
switched on, and with two ranks.  Trainer checks run in child processes with BMHRL_DETERMINISTIC=1 (each under its own
time limit; a child that fails ends the test)."""
import os
import socket
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BLOCK = 4096
# Longest chain of fp32 roundings between the exact sum of squares and the kernel's (csrc/grad_norm.hip): the product
# g * grad_scale enters the square twice (2) + the square (1) + 16 additions per thread + 6 shuffle levels + 3 additions over
# the four waves = 28 on the SUM (the fp64 second stage adds nothing visible); every term is non-negative, so the sum is
# within 28 * 2^-24 relative, the root halves that and adds the root's and the fp32 conversion's rounding: 16 on the NORM.
# The coefficient adds the + 1e-6, the reciprocal and the product: 19.  D bounds all of them (it must not exceed 64).
D = 32
EPS = 2.0 ** -24


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


def _torch_coef(norm_f32: torch.Tensor, max_norm: float) -> torch.Tensor:
    """clip_grad_norm_'s coefficient as torch evaluates it, on a CPU fp32 tensor"""
    return torch.clamp(max_norm / (norm_f32 + 1e-6), max=1.0)


def _table(sizes, dev, placement, gen):
    """the 7-word table of bmhrl_adam_segments for gradients of `sizes`; placement "flat": word 6 = 0, the gradients are
    slices of one bucket (offsets padded to 4 elements); "direct": separate allocations at 4-, 8- and 16-byte alignments.
    Returns (table, n_blocks, flat bucket, [gradient tensors], (vector blocks, scalar blocks) by the header's rule)."""
    offs, n = [], 0
    for s in sizes:
        offs.append(n)
        n += (s + 3) & ~3
    flat = torch.zeros(max(n, 4), device=dev)
    grads, rows, blk, n_vec, n_sca = [], [], 0, 0, 0
    for i, (s, o) in enumerate(zip(sizes, offs)):
        if placement == "flat":
            g = flat[o:o + s]
            ptr = 0
        else:
            shift = (1, 2, 4)[i % 3]                       # elements past a 256-byte aligned allocation: 4, 8, 16 bytes
            g = torch.zeros(s + shift, device=dev)[shift:]
            ptr = g.data_ptr()
            assert ptr % 16 == (4 * shift) % 16
        grads.append(g)
        rows.append([o, 0, 1, s, 0, blk, ptr])
        whole = s // BLOCK
        aligned = g.data_ptr() % 16 == 0
        n_vec += whole if aligned else 0
        n_sca += (s + BLOCK - 1) // BLOCK - (whole if aligned else 0)
        blk += (s + BLOCK - 1) // BLOCK
    return torch.tensor(rows, dtype=torch.int64).to(dev), blk, flat, grads, (n_vec, n_sca)


def _fill(grads, gen, kind):
    for g in grads:
        if kind == "zero":
            g.zero_()
            continue
        mag = 10.0 ** (torch.rand(g.shape, generator=gen) * 9.0 - 6.0)          # 1e-6 ... 1e3
        g.copy_((torch.randn(g.shape, generator=gen) * mag).to(g.device))


def _norm(table, n_seg, n_blk, flat, scale, max_norm, dev, ws_extra=0):
    from bmhrl_amd import ops
    hyper = torch.tensor([0.0, max_norm, -7.0, -7.0, 0, 0, 0, 0], dtype=torch.float32).to(dev)
    ws = torch.full((n_blk + ws_extra,), float("nan"), device=dev)
    ops.grad_norm(table, n_seg, n_blk, flat, scale, ws, hyper)
    return hyper.cpu()


SIZES = [1, 3, 4, 127, 4096, 4097, 10172 * 300, 1024 * 1024]


def _draw_sizes(n_params, gen):
    """sizes from SIZES; at most three of the two large ones per table (memory)"""
    idx = torch.randint(0, len(SIZES), (n_params,), generator=gen).tolist()
    big = 0
    out = []
    for i in idx:
        if i >= 6:
            big += 1
            if big > 3:
                i = i - 6          # 10172*300 -> 1, 1024*1024 -> 3
        out.append(SIZES[i])
    return out


@pytest.mark.parametrize("placement", ["flat", "direct"])
def test_grad_norm_kernel_against_float64(placement):
    dev = _need_gpu()
    gen = torch.Generator().manual_seed(11)
    reached = [0, 0]
    tables = [[s] for s in SIZES] + [[4096, 4096 * 3, 8192 + 5], SIZES] + [_draw_sizes(n, gen) for n in (2, 17, 300)]
    for sizes in tables:
        table, n_blk, flat, grads, (n_vec, n_sca) = _table(sizes, dev, placement, gen)
        reached[0] += n_vec
        reached[1] += n_sca
        for scale in (1.0, 0.125):
            for kind in ("mixed", "zero"):
                _fill(grads, gen, kind)
                ref = sum(float((g.double() * scale).pow(2).sum()) for g in grads) ** 0.5
                max_norm = 0.5 * ref if ref > 0 else 1.0
                h = _norm(table, len(sizes), n_blk, flat, scale, max_norm, dev)
                h2 = _norm(table, len(sizes), n_blk, flat, scale, max_norm, dev, ws_extra=3)
                assert torch.equal(h.view(torch.int32), h2.view(torch.int32))            # run to run: the same bits
                norm, coef = float(h[3]), float(h[2])
                print(f"{placement} n={len(sizes)} scale={scale} {kind}: norm {norm!r} ref {ref!r} rel {abs(norm - ref) / max(ref, 1e-300):.2e}")
                assert abs(norm - ref) <= D * EPS * ref, (sizes[:8], scale, kind, norm, ref)
                assert float(h[0]) == 0.0 and float(h[1]) == torch.tensor(max_norm, dtype=torch.float32).item()
                assert coef == float(_torch_coef(h[3], max_norm))                        # torch's formula on the kernel's norm: exact
                coef64 = min(1.0, max_norm / (ref + 1e-6))
                assert abs(coef - coef64) <= D * EPS * coef64, (coef, coef64)
                if kind == "zero":
                    assert norm == 0.0 and coef == 1.0
                else:
                    assert 0.0 < coef < 0.51                   # (the + 1e-6 shows on the tables with a tiny norm)
        for bad in (float("nan"), float("inf"), float("-inf")):
            _fill(grads, gen, "mixed")
            k = len(grads) // 2
            grads[k][grads[k].numel() // 2] = bad
            h = _norm(table, len(sizes), n_blk, flat, 1.0, 1.0, dev)
            assert not bool(torch.isfinite(h[3])) and bool(torch.isnan(h[2])), (bad, h)
        del table, flat, grads
    assert reached[0] > 0 and reached[1] > 0, reached           # the 16-byte path and the scalar path both ran
    if placement == "direct":
        assert reached[1] > 1000                                # whole blocks at 4- / 8-byte alignment take the scalar path too


def test_grad_norm_refuses_what_it_cannot_handle():
    dev = _need_gpu()
    from bmhrl_amd import _lib, ops
    table, n_blk, flat, grads, _ = _table([4097], dev, "flat", None)
    hyper = torch.zeros(8, device=dev)
    with pytest.raises(_lib.HipError, match="-22"):
        ops.grad_norm(table, 1, n_blk, flat, 1.0, torch.zeros(n_blk - 1, device=dev), hyper)
    with pytest.raises(_lib.HipError, match="-22"):
        ops.grad_norm(table, 1, 0, flat, 1.0, torch.zeros(4, device=dev), hyper)
    with pytest.raises(RuntimeError, match="GPU only"):
        ops.grad_norm(table, 1, n_blk, flat, 1.0, torch.zeros(4), hyper)


def _adam_case(dev, direct):
    """a table built by hand from the header's description: an aligned bf16 shadow (16-byte path), an odd-sized bf16 shadow,
    a split [hi | lo | hi] shadow, an fp32 copy and a parameter without shadow"""
    gen = torch.Generator().manual_seed(5)
    shapes = [(64, 128), (5, 7), (16, 300), (1, 515), (1, 4099)]
    offs, n = [], 0
    for r, c in shapes:
        offs.append(n)
        n += (r * c + 3) & ~3
    st = {k: torch.randn(n, generator=gen).to(dev) for k in ("p", "g", "m")}
    st["v"] = (torch.rand(n, generator=gen) * 1e-2).to(dev)
    part = 304
    shadows = [torch.zeros(64, 128, dtype=torch.bfloat16, device=dev), torch.zeros(5, 8, dtype=torch.bfloat16, device=dev),
               torch.zeros(16, 3 * part, dtype=torch.bfloat16, device=dev), torch.zeros(515, device=dev), None]
    ld = [128, 8, (3 * part) | (part << 32), 0, 0]
    gsep = [st["g"][o:o + r * c].clone() for (r, c), o in zip(shapes, offs)] if direct else None
    rows, blk = [], 0
    for i, ((r, c), o) in enumerate(zip(shapes, offs)):
        rows.append([o, 0 if shadows[i] is None else shadows[i].data_ptr(), r, c, ld[i], blk, gsep[i].data_ptr() if direct else 0])
        blk += (r * c + BLOCK - 1) // BLOCK
    return torch.tensor(rows, dtype=torch.int64).to(dev), len(rows), blk, st, shadows, gsep, n


@pytest.mark.parametrize("direct", [False, True])
@pytest.mark.parametrize("coef,gscale", [(1.0, 1.0), (0.3183, 0.5)])
def test_dev_adam_equals_the_existing_entry_points(direct, coef, gscale):
    dev = _need_gpu()
    from bmhrl_amd import ops
    lr = 3e-3
    f32 = lambda x: torch.tensor(x, dtype=torch.float32)
    eff = float(f32(gscale) * f32(coef))                       # float32(grad_scale) * float32(coef): the ONE factor
    outs = []
    for use_dev in (False, True):
        table, n_seg, n_blk, st, shadows, gsep, n = _adam_case(dev, direct)
        if direct:
            st["g"].fill_(float("nan"))                        # must not be read: word 6 names every gradient
        hyper = torch.tensor([lr, 1.0, coef, 0, 0, 0, 0, 0], dtype=torch.float32).to(dev) if use_dev else None
        for step in (1, 2, 3):
            if use_dev:
                ops.adam_segments(table, n_seg, n_blk, st["p"], st["g"], st["m"], st["v"], 123.0, 0.9, 0.999, 1e-8, 0.01, step, gscale,
                                  hyper=hyper)
            else:
                ops.adam_segments(table, n_seg, n_blk, st["p"], st["g"], st["m"], st["v"], lr, 0.9, 0.999, 1e-8, 0.01, step, eff)
        # and the plain kernel over a copy of the bucket
        q = {k: v.clone() for k, v in st.items()}
        if direct:
            q["g"] = torch.randn(n, generator=torch.Generator().manual_seed(9)).to(dev)
        if use_dev:
            ops.adam_step(q["p"], q["g"], q["m"], q["v"], n, 123.0, 0.9, 0.999, 1e-8, 0.01, 4, gscale, hyper=hyper)
        else:
            ops.adam_step(q["p"], q["g"], q["m"], q["v"], n, lr, 0.9, 0.999, 1e-8, 0.01, 4, eff)
        torch.cuda.synchronize()
        outs.append([st["p"], st["m"], st["v"], q["p"], q["m"], q["v"]] + [s for s in shadows if s is not None])
    for a, b in zip(*outs):
        assert bool(torch.isfinite(a.float()).all()) and float(a.float().abs().sum()) > 0
        assert torch.equal(a, b)
    if coef != 1.0:                                            # the factor does matter: the unscaled update differs
        table, n_seg, n_blk, st, shadows, gsep, n = _adam_case(dev, direct)
        for step in (1, 2, 3):
            ops.adam_segments(table, n_seg, n_blk, st["p"], st["g"], st["m"], st["v"], lr, 0.9, 0.999, 1e-8,
                              0.01, step, gscale)
        assert not torch.equal(st["m"], outs[0][1])


# ------------------------------------------------------------------------------------------------ trainer, child processes
_CHILD = r"""
import os, sys, json, torch
from bmhrl_amd import synthetic as syn
from bmhrl_amd.train import CaptionTrainer
out_path, mode, phase = sys.argv[1], sys.argv[2], sys.argv[3]
dev = torch.device("cuda:0")
b = syn.synthetic_batch(2, 128, 200, 12, 300, seed=2)
fs = {k: b[k].to(dev) for k in ("rgb", "flow", "audio")}
cap = b["captions"].to(dev)
rew = syn.synthetic_rewards(cap.shape[0], cap.shape[1] - 1, seed=5).to(dev)

def make(clip, **kw):
    extra = dict(phase="worker", reward_fn=lambda s, c: rew, value_lr=1e-3) if phase == "worker" else {}
    t = CaptionTrainer(syn.default_cfg(dout_p=0.0), 300, dev, exploration=False, lr=1e-3, grad_clip=clip, **extra, **kw)
    t.agent.train()
    if t.value_net is not None:
        t.value_net.train()
    return t

def grads(o):
    return torch.cat([(torch.zeros(p.numel(), device=dev) if p.grad is None else p.grad.detach().reshape(-1).float()) for p in o.params0])

def snap(o, name):
    return o.in_param_order(getattr(o, name)).detach().cpu().clone()

res = {}
if mode == "eager":
    # unclipped: the first step's gradient, its float64 norm, the first moments, the weights after three steps
    t = make(None)
    assert t.opt.hyper is None
    t.step(fs, cap); torch.cuda.synchronize()
    g = grads(t.opt)
    res["g"] = g.cpu()
    norm64 = float(g.double().pow(2).sum().sqrt())
    res["norm64"] = norm64
    if t.value_net is not None:
        res["v_m_plain"] = snap(t.vopt, "exp_avg")
    for _ in range(2):
        t.step(fs, cap)
    torch.cuda.synchronize()
    res["w_plain"] = snap(t.opt, "flat")
    del t
    # a threshold nothing reaches: the same weights
    t = make(1e30)
    for _ in range(3):
        t.step(fs, cap)
    torch.cuda.synchronize()
    res["w_huge"] = snap(t.opt, "flat")
    res["coef_huge"] = float(t.last_clip_coef)
    del t
    # half the first norm
    t = make(0.5 * norm64)
    t.step(fs, cap); torch.cuda.synchronize()
    res["norm"], res["coef"] = t.last_grad_norm.cpu().clone(), t.last_clip_coef.cpu().clone()
    res["m_clip"] = snap(t.opt, "exp_avg")
    if t.value_net is not None:
        res["v_m_clip"] = snap(t.vopt, "exp_avg")
        res["v_hyper"] = t.vopt.hyper.cpu().clone()
elif mode == "captured":
    c = float(sys.argv[4])
    t1 = make(c)
    l_eager = [float(t1.step(fs, cap)) for _ in range(5)]
    torch.cuda.synchronize()
    res["w_eager"], res["l_eager"] = snap(t1.opt, "flat"), l_eager
    res["norm_eager"] = float(t1.last_grad_norm)
    del t1
    t2 = make(c)
    t2.capture(fs, cap, warmup=1)
    ga = t2.graph_a
    l_graph, norms, coefs = [], [], []
    for _ in range(4):
        l_graph.append(float(t2.replay())); norms.append(float(t2.last_grad_norm)); coefs.append(float(t2.last_clip_coef))
    res["w_graph"], res["l_graph"], res["norms"], res["coefs"] = snap(t2.opt, "flat"), l_graph, norms, coefs
    w0, m0 = snap(t2.opt, "flat"), snap(t2.opt, "exp_avg")
    t2.set_lr(0.0); t2.replay(); torch.cuda.synchronize()
    res["lr0_same_w"] = bool(torch.equal(w0, snap(t2.opt, "flat")))
    res["lr0_same_m"] = bool(torch.equal(m0, snap(t2.opt, "exp_avg")))
    t2.set_lr(1e-4); t2.replay(); torch.cuda.synchronize()
    res["lr1_same_w"] = bool(torch.equal(w0, snap(t2.opt, "flat")))
    res["lr_read_back"] = t2.opt.lr
    t2.set_grad_clip(1e30); t2.replay(); torch.cuda.synchronize()
    res["coef_after"] = float(t2.last_clip_coef)
    res["same_graph"] = t2.graph_a is ga and t2.graph_b is None
    err = None
    t3 = make(None)
    t3.capture(fs, cap, warmup=1)
    try:
        t3.set_lr(1e-5)
    except RuntimeError as e:
        err = str(e)
    res["set_lr_error"] = err
elif mode == "calls":
    # library calls of capture(warmup=1), by entry point, with and without grad_clip
    from bmhrl_amd import _lib
    lib = _lib.load()
    counts = {}
    def wrap(name, fn):
        def f(*a):
            counts[name] = counts.get(name, 0) + 1
            return fn(*a)
        return f
    for name in _lib.PROTOTYPES:
        setattr(lib, name, wrap(name, getattr(lib, name)))
    per = {}
    for label, clip in (("first", None), ("clip", float(sys.argv[4])), ("plain", None)):      # (the first trainer of a process also fills process-wide caches)
        t = make(clip)
        t.step(fs, cap); torch.cuda.synchronize()
        counts.clear()
        t.capture(fs, cap, warmup=1); torch.cuda.synchronize()
        per[label] = dict(counts)
        float(t.replay())
        del t
    res["calls"] = per
elif mode == "experiments":
    c = float(sys.argv[4])
    for label, env in (("plain", {}), ("early", {"BMHRL_EARLY_ADAM": "1"}), ("phased", {"BMHRL_PHASED_ADAM": "1"})):
        for k in ("BMHRL_EARLY_ADAM", "BMHRL_PHASED_ADAM"):
            os.environ.pop(k, None)
        os.environ.update(env)
        import warnings
        with warnings.catch_warnings(record=True) as wlist:
            warnings.simplefilter("always")
            t = make(c)
        t.capture(fs, cap, warmup=1)
        flags = [bool(t._early_ok()), bool(t._phased_one_rank())]
        losses = [float(t.replay()) for _ in range(3)]
        flags += [bool(t._early_ok()), sorted(t._early_done)]
        torch.cuda.synchronize()
        res[label] = {"w": snap(t.opt, "flat"), "losses": losses, "flags": flags, "coef": float(t.last_clip_coef),
                      "warned": sum("grad_clip" in str(w.message) for w in wlist)}
        del t
torch.save(res, out_path)
"""


def _child(tmp_path, name, *args, timeout=600):
    """one child process under its own time limit; any failure ends the test (nothing is started after it)"""
    _need_gpu()
    f = tmp_path / f"{name}.pt"
    env = dict(os.environ, BMHRL_DETERMINISTIC="1", PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    for k in ("BMHRL_EARLY_ADAM", "BMHRL_PHASED_ADAM"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, "-c", _CHILD, str(f)] + [str(a) for a in args], env=env, capture_output=True, text=True,
                       timeout=timeout)
    assert r.returncode == 0, (r.returncode, r.stderr[-3000:])
    return torch.load(f)


@pytest.mark.parametrize("phase", ["warmstart", "worker"])
def test_trainer_eager_clipping(tmp_path, phase):
    """grad_clip = 1e30 changes nothing; grad_clip = half the first norm halves the first moment.  (The first Adam step is
    nearly scale-invariant in the weights, so the moment is what shows the coefficient.)"""
    r = _child(tmp_path, "eager_" + phase, "eager", phase)
    assert r["coef_huge"] == 1.0 and torch.equal(r["w_plain"], r["w_huge"])
    norm, coef, norm64 = float(r["norm"]), float(r["coef"]), r["norm64"]
    print(f"{phase}: norm {norm!r} float64 {norm64!r} rel {abs(norm - norm64) / norm64:.2e} coef {coef!r}")
    assert norm64 > 0 and abs(norm - norm64) <= D * EPS * norm64, (norm, norm64)
    assert coef == float(_torch_coef(r["norm"], 0.5 * norm64)) and abs(coef - 0.5) < 1e-5
    # exp_avg = fl(fl(1 - beta1) * fl(g * coef)): two fp32 roundings away from the exact product
    one_minus_b1 = float(torch.tensor(1.0, dtype=torch.float32) - torch.tensor(0.9, dtype=torch.float32))
    want = r["g"].double() * coef * one_minus_b1
    got = r["m_clip"].double()
    assert float(want.abs().max()) > 0
    bad = (got - want).abs() > 2 * EPS * want.abs() * (1 + 1e-6) + 1e-44
    assert not bool(bad.any()), (int(bad.sum()), float(((got - want).abs() / want.abs().clamp_min(1e-30)).max()))
    if phase == "worker":                                    # the value network is not clipped
        assert torch.equal(r["v_m_plain"], r["v_m_clip"]) and float(r["v_m_clip"].abs().sum()) > 0
        assert float(r["v_hyper"][2]) == 1.0 and float(r["v_hyper"][3]) == 0.0


CLIP = 1e-3          # far below any gradient norm of these steps (asserted: the coefficient is below 1)


@pytest.mark.parametrize("phase", ["warmstart", "worker"])
def test_trainer_captured_clipping_follows_the_block(tmp_path, phase):
    r = _child(tmp_path, "captured_" + phase, "captured", phase, CLIP)
    # one warm-up step + four replays == five eager steps (deterministic mode: exactly)
    assert r["l_eager"][1:] == r["l_graph"], (r["l_eager"], r["l_graph"])
    assert torch.equal(r["w_eager"], r["w_graph"])
    assert all(0 < c < 1 for c in r["coefs"])
    assert len(set(r["norms"])) == 4 and r["norms"][3] == r["norm_eager"]       # recomputed at every replay, not frozen
    assert r["lr0_same_w"] and not r["lr0_same_m"]           # lr 0: the weights stand still, the moments move
    assert not r["lr1_same_w"] and r["lr_read_back"] == 1e-4
    assert r["coef_after"] == 1.0
    assert r["same_graph"]                                   # no recapture in between
    assert r["set_lr_error"] is not None and "lr_on_device" in r["set_lr_error"]


def test_clipped_capture_adds_one_library_call_of_two_kernels(tmp_path):
    """No test counts graph nodes; what is counted here are the library's entry points called by capture(warmup=1) with
    and without grad_clip: bmhrl_grad_norm (two launches, csrc/grad_norm.hip) once per pass, bmhrl_adam_segments_dev in
    place of bmhrl_adam_segments, everything else unchanged.  FlatAdam.clip() issues no torch operation on the GPU."""
    r = _child(tmp_path, "calls", "calls", "warmstart", CLIP)
    plain, clip = r["calls"]["plain"], r["calls"]["clip"]
    passes = clip.pop("bmhrl_grad_norm")
    assert passes == 2                                       # the warm-up step and the captured step
    assert clip.pop("bmhrl_adam_segments_dev") == plain.pop("bmhrl_adam_segments") == passes
    assert "bmhrl_adam_segments" not in clip and "bmhrl_grad_norm" not in plain
    assert clip == plain


def test_side_stream_experiments_are_ignored_with_grad_clip(tmp_path):
    r = _child(tmp_path, "experiments", "experiments", "warmstart", CLIP)
    for label in ("early", "phased"):
        assert r[label]["flags"] == [False, False, False, []], r[label]["flags"]
        assert r[label]["warned"] == 1 and r["plain"]["warned"] == 0
        assert r[label]["losses"] == r["plain"]["losses"] and torch.equal(r[label]["w"], r["plain"]["w"])
    assert 0 < r["plain"]["coef"] < 1


# ------------------------------------------------------------------------------------------------ two ranks
V, TV, TA, L, B_RANK = 60, 160, 200, 8, 2


def _free_port():
    s = socket.socket(); s.bind(("127.0.0.1", 0)); p = s.getsockname()[1]; s.close(); return p


def _cfg():
    from bmhrl_amd import synthetic as syn
    return syn.tiny_cfg(d_model=1024, rl_att_heads=4, dout_p=0.0)


def _batch(seeds, dev):
    from bmhrl_amd import synthetic as syn
    cfg = _cfg()
    parts = [syn.synthetic_batch(B_RANK, TV, TA, L, V, seed=s, d_vid=cfg.d_vid, d_aud=cfg.d_aud, min_len=3) for s in seeds]
    return {k: torch.cat([p[k] for p in parts]).to(dev) for k in ("rgb", "flow", "audio", "captions")}


def _reward(sampled, captions):
    return (sampled % 17).float() / 17.0


def _trainer(phase, dev):
    from bmhrl_amd.train import CaptionTrainer
    extra = dict(phase="worker", reward_fn=_reward) if phase == "worker" else {}
    return CaptionTrainer(_cfg(), V, dev, exploration=False, seed=0, grad_clip=CLIP, **extra)


def _run(tr, b):
    tr.capture({k: b[k] for k in ("rgb", "flow", "audio")}, b["captions"], warmup=1)
    tr.replay()
    torch.cuda.synchronize()


def _rank(rank, world, port, phase, out):
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY="0")
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    dev = torch.device("cuda:0")
    tr = _trainer(phase, dev)
    assert tr._split() and tr.graph is None
    _run(tr, _batch([40 + rank], dev))
    assert tr.graph_b is not None                       # the norm sits in graph_b, behind the last bucket's all-reduce
    out[rank] = (tr.opt.in_param_order(tr.opt.flat).cpu(), tr.opt.hyper.cpu())
    dist.destroy_process_group()


@pytest.mark.parametrize("phase", ["warmstart", "worker"])
def test_two_ranks_clip_like_one_process(phase):
    """pattern and tolerances of tests/test_ddp_gpu.py; the ranks are fresh child processes joined under a time limit"""
    import time
    import torch.multiprocessing as mp
    dev = _need_gpu()
    world, port = 2, _free_port()
    ctx = mp.get_context("spawn")
    out = ctx.Manager().dict()
    procs = mp.spawn(_rank, args=(world, port, phase, out), nprocs=world, join=False)
    deadline = time.time() + 600
    while not procs.join(timeout=5):                    # (raises when a rank failed; the other one is terminated)
        if time.time() > deadline:
            for p in procs.processes:
                p.kill()
            pytest.fail("the ranks did not finish in 600 s")
    (flat0, h0), (flat1, h1) = out[0], out[1]
    assert torch.equal(flat0, flat1)
    assert torch.equal(h0.view(torch.int32), h1.view(torch.int32))            # norm and coefficient: bit for bit
    assert 0 < float(h0[2]) < 1 and float(h0[1]) == torch.tensor(CLIP).item()
    tr = _trainer(phase, dev)
    tr.split_backward = False
    _run(tr, _batch([40, 41], dev))
    h = tr.opt.hyper.cpu()
    print(f"{phase}: ranks' norm {float(h0[3])!r}, one process {float(h[3])!r}")
    assert abs(float(h0[3]) - float(h[3])) <= 3e-2 * float(h[3])              # the gradient tolerance of test_ddp_gpu.py
    assert float((flat0 - tr.opt.in_param_order(tr.opt.flat).cpu()).abs().max()) <= 2.5e-4
