"""Gradient-norm clipping and the device-resident learning rate, host side: the ABI additions, FlatAdam's CPU form against
torch.optim.Adam + clip_grad_norm_, PlateauLR against torch's ReduceLROnPlateau, two gloo ranks, set_lr semantics."""
import os
import socket

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

F32_EPS = 2.0 ** -24          # half an ulp of fp32, relative


def test_new_symbols_exported_and_abi_still_18():
    from bmhrl_amd import build, _lib
    build.build(verbose=False)
    lib = _lib.load()
    for name in ("bmhrl_grad_norm", "bmhrl_adam_segments_dev", "bmhrl_adam_step_dev"):
        assert name in _lib.PROTOTYPES and hasattr(lib, name)
    assert lib.bmhrl_hip_abi_version() == 18
    # refused like the other entry points: null table, no blocks, a workspace smaller than n_blocks, a missing block
    assert lib.bmhrl_grad_norm(None, 1, 1, None, 1.0, None, 1, None, None) == -22
    assert lib.bmhrl_grad_norm(8, 1, 0, 8, 1.0, 8, 1, 8, None) == -22
    assert lib.bmhrl_grad_norm(8, 1, 4, 8, 1.0, 8, 3, 8, None) == -22
    assert lib.bmhrl_adam_step_dev(8, 8, 8, 8, 4, 0.0, 0.9, 0.999, 1e-8, 0.0, 1, None, 1.0, None, None) == -22
    assert lib.bmhrl_adam_segments_dev(8, 1, 1, 8, 8, 8, 8, 0.0, 0.9, 0.999, 1e-8, 0.0, 1, None, 1.0, None, None) == -22


SHAPES = [(5, 3), (7,), (2, 2), (1,), (13, 11), (129,)]      # odd sizes: slices of the bucket are padded to 4 elements


def _run_pair(clip, weight_decay, grad_mag, missing_step=None, steps=5):
    """FlatAdam(grad_clip=clip) against clip_grad_norm_ + torch.optim.Adam on plain copies; returns the two parameter lists
    and the (norm, coef) pairs of every step: (ours, torch's)"""
    from bmhrl_amd.train import FlatAdam
    torch.manual_seed(0)
    ps = [torch.nn.Parameter(torch.randn(*s)) for s in SHAPES]
    ref = [torch.nn.Parameter(p.detach().clone()) for p in ps]
    opt_ref = torch.optim.Adam(ref, lr=1e-2, weight_decay=weight_decay)
    opt = FlatAdam(ps, lr=1e-2, weight_decay=weight_decay, grad_clip=clip)
    seen = []
    for step in range(steps):
        for p, r in zip(ps, ref):
            g = torch.randn_like(p) * grad_mag
            none = step == missing_step and p.dim() == 1 and p.numel() == 7
            p.grad = None if none else g.clone()
            r.grad = None if none else g.clone()
        opt.gather_grads()
        if clip is not None:
            opt.clip()
            with_grad = [r for r in ref if r.grad is not None]
            total = torch.nn.utils.clip_grad_norm_(with_grad, clip)
            coef_ref = torch.clamp(clip / (total + 1e-6), max=1.0)
            seen.append((float(opt.last_grad_norm), float(opt.last_clip_coef), float(total), float(coef_ref)))
        for r in ref:                   # (torch skips a parameter without gradient; FlatAdam gives it a zero gradient)
            if r.grad is None:
                r.grad = torch.zeros_like(r)
        opt.step()
        opt_ref.step()
    return ps, ref, seen, opt


@pytest.mark.parametrize("case", ["above", "missing_grad", "weight_decay"])
def test_flat_adam_cpu_clip_matches_torch(case):
    """gradient norm ~ 18 x grad_mag for these shapes; threshold 1.0 clips every step"""
    wd = 0.1 if case == "weight_decay" else 0.0
    ps, ref, seen, _ = _run_pair(1.0, wd, 1.0, missing_step=1 if case == "missing_grad" else None)
    assert len(seen) == 5
    for norm, coef, norm_ref, coef_ref in seen:
        assert coef < 0.2                                     # the case really clips
        assert abs(norm - norm_ref) <= 4 * F32_EPS * norm_ref, (norm, norm_ref)     # torch sums in fp32, FlatAdam in fp64
        assert abs(coef - coef_ref) <= 8 * F32_EPS * coef_ref, (coef, coef_ref)
    for p, r in zip(ps, ref):
        assert torch.allclose(p, r, atol=1e-6), (p - r).abs().max()      # tolerance of test_flat_adam_cpu_matches_torch_...


def test_flat_adam_cpu_below_threshold_is_the_unclipped_update():
    ps, ref, seen, opt = _run_pair(1e3, 0.0, 1.0)
    assert all(coef == 1.0 for _, coef, _, _ in seen) and all(c == 1.0 for _, _, _, c in seen)
    plain, _, _, _ = _run_pair(None, 0.0, 1.0)
    for p, q, r in zip(ps, plain, ref):
        assert torch.equal(p, q)
        assert torch.allclose(p, r, atol=1e-6)
    assert opt.hyper.shape == (8,) and float(opt.hyper[0]) == pytest.approx(1e-2) and float(opt.hyper[1]) == 1e3
    assert bool((opt.hyper[4:] == 0).all())


def test_flat_adam_defaults_allocate_no_block():
    from bmhrl_amd.train import FlatAdam
    opt = FlatAdam([torch.nn.Parameter(torch.randn(3))], lr=1e-3)
    assert opt.hyper is None and opt.grad_clip is None
    with pytest.raises(RuntimeError, match="without grad_clip"):
        opt.clip()
    with pytest.raises(RuntimeError, match="without grad_clip"):
        opt.set_grad_clip(1.0)
    dev = FlatAdam([torch.nn.Parameter(torch.randn(3))], lr=1e-3, lr_on_device=True)
    assert dev.hyper.tolist() == [pytest.approx(1e-3), float("inf"), 1.0, 0.0, 0.0, 0.0, 0.0, 0.0]


def test_nonfinite_gradient_gives_nan_coefficient_on_the_host_form():
    from bmhrl_amd.train import FlatAdam
    for bad in (float("nan"), float("inf")):
        p = torch.nn.Parameter(torch.randn(6))
        opt = FlatAdam([p], lr=1e-3, grad_clip=1.0)
        p.grad = torch.ones(6)
        p.grad[2] = bad
        opt.gather_grads(); opt.clip()
        assert not bool(torch.isfinite(opt.last_grad_norm)) and bool(torch.isnan(opt.last_clip_coef))


# 60 validation metrics: improvements, plateaus, improvements inside the relative threshold (1e-4: they do not count),
# one outside it, and a tail long enough to run into min_lr
METRICS = ([5.0, 4.0, 3.5, 3.2, 3.1] + [3.1] * 4 + [3.09999, 3.09998, 3.0999] + [3.2] * 3 + [3.0, 2.9] +
           [2.89999, 2.89998, 2.89997, 2.89996] + [2.95] * 6 + [2.5] + [2.6, 2.55, 2.7, 2.51, 2.50001, 2.49999] + [2.8] * 24 + [2.0, 2.1])


@pytest.mark.parametrize("patience,factor,min_lr", [(3, 0.1, 1e-7), (10, 0.1, 0.0), (2, 0.5, 2e-4), (0, 0.3, 1e-6)])
def test_plateau_lr_decides_like_torch(patience, factor, min_lr):
    from bmhrl_amd.train import FlatAdam, PlateauLR
    assert len(METRICS) == 60
    w = torch.nn.Parameter(torch.zeros(1))
    ref_opt = torch.optim.Adam([w], lr=1e-3)
    ref = torch.optim.lr_scheduler.ReduceLROnPlateau(ref_opt, mode="min", factor=factor, patience=patience, threshold=1e-4,
                                                     threshold_mode="rel", cooldown=0, min_lr=min_lr)
    trainer = type("T", (), {})()
    trainer.opt = FlatAdam([torch.nn.Parameter(torch.zeros(1))], lr=1e-3, lr_on_device=True)
    trainer.set_lr = trainer.opt.set_lr
    sched = PlateauLR(trainer, factor=factor, patience=patience, threshold=1e-4, min_lr=min_lr)
    rates = []
    for m in METRICS:
        ref.step(m)
        got = sched.step(m)
        assert got == trainer.opt.lr == ref_opt.param_groups[0]["lr"], (m, got, ref_opt.param_groups[0]["lr"])
        assert float(trainer.opt.hyper[0]) == torch.tensor(got, dtype=torch.float32).item()
        rates.append(got)
    assert len(set(rates)) >= 3                                # the sequence does lower the rate more than once


def test_plateau_lr_runs_into_min_lr():
    from bmhrl_amd.train import FlatAdam, PlateauLR
    trainer = type("T", (), {})()
    trainer.opt = FlatAdam([torch.nn.Parameter(torch.zeros(1))], lr=1e-3, lr_on_device=True)
    trainer.set_lr = trainer.opt.set_lr
    sched = PlateauLR(trainer, factor=0.1, patience=2, min_lr=2e-5)
    rates = [sched.step(m) for m in METRICS]
    assert rates[-1] == 2e-5 and trainer.opt.lr == 2e-5


def _free_port():
    s = socket.socket(); s.bind(("127.0.0.1", 0)); p = s.getsockname()[1]; s.close(); return p


def _clip_params():
    torch.manual_seed(0)
    return [torch.nn.Parameter(torch.randn(6, 4)), torch.nn.Parameter(torch.randn(9)), torch.nn.Parameter(torch.randn(3, 5))]


def _clip_worker(rank, world, port, out):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from bmhrl_amd.train import FlatAdam
    ps = _clip_params()
    opt = FlatAdam(ps, lr=1e-2, grad_clip=0.7)
    words = []
    for step in range(3):
        g = torch.Generator().manual_seed(100 * step + rank)
        for p in ps:
            p.grad = torch.randn(p.shape, generator=g) * (1.0 + rank)      # different local gradients
        opt.gather_grads()
        scale = opt.all_reduce()
        opt.clip(scale)                                                     # norm of the AVERAGED gradient
        words.append(opt.hyper[2:4].clone())
        opt.step(scale)
    out[rank] = (opt.flat.clone(), torch.stack(words))
    dist.destroy_process_group()


def test_two_ranks_clip_the_averaged_gradient_identically():
    world, port = 2, _free_port()
    out = mp.Manager().dict()
    mp.spawn(_clip_worker, args=(world, port, out), nprocs=world, join=True)
    assert torch.equal(out[0][0], out[1][0])
    assert torch.equal(out[0][1].view(torch.int32), out[1][1].view(torch.int32))       # norm and coefficient, bit for bit
    from bmhrl_amd.train import FlatAdam
    ps = _clip_params()
    summed = FlatAdam(ps, lr=1e-2, grad_clip=0.7)          # one process on the SUMMED gradient, scale 1 / world: the ranks' bytes
    qs = _clip_params()
    averaged = FlatAdam(qs, lr=1e-2, grad_clip=0.7)        # ... and on the averaged gradient
    for step in range(3):
        gs = [torch.Generator().manual_seed(100 * step + r) for r in range(world)]
        for p, q in zip(ps, qs):
            p.grad = sum(torch.randn(p.shape, generator=g) * (1.0 + r) for r, g in enumerate(gs))
            q.grad = p.grad / world
        summed.gather_grads(); summed.clip(1.0 / world)
        assert torch.equal(summed.hyper[2:4].view(torch.int32), out[0][1][step].view(torch.int32))
        averaged.gather_grads(); averaged.clip()
        assert torch.equal(averaged.hyper[2:4], summed.hyper[2:4])        # (x 0.5 is exact)
        assert float(summed.last_clip_coef) < 0.5
        summed.step(1.0 / world); averaged.step()
    assert torch.allclose(summed.flat, out[0][0], atol=1e-6)
    assert torch.allclose(averaged.flat, out[0][0], atol=1e-6)


def test_set_lr_before_and_after_a_capture():
    from bmhrl_amd.train import FlatAdam
    opt = FlatAdam([torch.nn.Parameter(torch.randn(3))], lr=1e-3)
    opt.set_lr(5e-4)
    assert opt.lr == 5e-4
    opt.lr = 2e-4                                        # plain assignment keeps working
    assert opt.lr == 2e-4
    opt.captured = True                                  # what CaptionTrainer.capture() sets
    with pytest.raises(RuntimeError, match="lr_on_device"):
        opt.set_lr(1e-4)
    assert opt.lr == 2e-4
    dev = FlatAdam([torch.nn.Parameter(torch.randn(3))], lr=1e-3, lr_on_device=True)
    dev.captured = True
    dev.set_lr(1e-4)
    assert dev.lr == 1e-4 and float(dev.hyper[0]) == torch.tensor(1e-4, dtype=torch.float32).item()
    # the CPU step reads the rate that was set
    p = torch.nn.Parameter(torch.ones(4))
    o = FlatAdam([p], lr=1e-3, lr_on_device=True)
    o.set_lr(0.0)
    p.grad = torch.ones(4)
    o.gather_grads(); o.step()
    assert torch.equal(p.detach(), torch.ones(4)) and float(o.exp_avg.abs().sum()) > 0
