"""The accumulate launch of gradient accumulation on the GPU: bmhrl_accum_segments (ops.accum_segments) against float64 over
the Adam table in two gradient placements, the bytes it must not write, run-to-run bits, the loss word and the refusals."""
import pytest
import torch

pytestmark = pytest.mark.gpu

BLOCK = 4096
EPS = 2.0 ** -23          # one rounding of an fma (2^-24 relative) plus room for the float64 reference's own double rounding
SENTINEL = 0x7FC0DEAD     # a NaN with a payload: the bit pattern of everything a launch must not write


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


# ------------------------------------------------------------------------------------------------ (a) the kernel
SHAPES = [(1, 1), (1, 3), (1, 4), (1, 4095), (1, 4096), (1, 4097), (1, 2 * 4096 + 5), (32, 1024)]


def _case(dev, placement, gen):
    """the 7-word table of bmhrl_adam_segments over SHAPES.  "flat": word 6 = 0, the gradients are slices of one bucket;
    "mixed": every other parameter's gradient is an allocation of its own -- the 32 x 1024 one 16-byte aligned (vector path),
    the 2 * 4096 + 5 one a float past an aligned address (4-byte but not 16-byte aligned: whole blocks on the scalar path)."""
    offs, n = [], 0
    for r, c in SHAPES:
        offs.append(n)
        n += (r * c + 3) & ~3
    flat = torch.randn(n, generator=gen).to(dev)
    own = {}
    rows, blk = [], 0
    for i, ((r, c), o) in enumerate(zip(SHAPES, offs)):
        ptr = 0
        if placement == "mixed" and i in (1, 3, 6, 7):
            shift = 1 if i == 6 else 0
            own[i] = torch.randn(r * c + shift, generator=gen).to(dev)[shift:]
            ptr = own[i].data_ptr()
            assert ptr % 4 == 0 and (ptr % 16 == 0) == (shift == 0)
            flat[o:o + r * c] = float("nan")                   # must not be read: word 6 names this gradient
        rows.append([o, 0, r, c, 0, blk, ptr])
        blk += (r * c + BLOCK - 1) // BLOCK
    grads = [own[i] if i in own else flat[o:o + r * c] for i, ((r, c), o) in enumerate(zip(SHAPES, offs))]
    return torch.tensor(rows, dtype=torch.int64).to(dev), blk, flat, grads, offs, n


def _run_sequence(dev, placement):
    """first (on an accumulator full of NaN), then two adds with the weights read from the device words; returns the
    accumulator and the loss word after every launch, with the float64 references"""
    from bmhrl_amd import ops
    gen = torch.Generator().manual_seed(3)
    table, n_blk, flat, grads, offs, n = _case(dev, placement, gen)
    guard = 64
    acc = torch.full((n + guard,), SENTINEL, dtype=torch.int32, device=dev).view(torch.float32)
    loss_out = torch.full((1,), float("nan"), device=dev)
    steps = []
    prev = None
    prev_loss = 0.0
    for first, w, loss in ((1.0, 0.37, 3.25), (0.0, 0.37, 1.7), (0.0, 1.0, 2.9)):
        ctl = torch.tensor([w, first], dtype=torch.float32).to(dev)
        loss_in = torch.tensor([loss], dtype=torch.float32).to(dev)
        for g in grads:                                        # fresh gradients per launch
            g.copy_(torch.randn(g.shape, generator=gen).to(dev))
        ops.accum_segments(table, len(SHAPES), n_blk, flat, acc, ctl, loss_in, loss_out)
        torch.cuda.synchronize()
        w64 = float(ctl[0].double())
        ref = []
        for i, g in enumerate(grads):
            base = 0.0 if first else prev[i]
            ref.append(w64 * g.double().cpu() + base)
        ref_loss = w64 * float(loss_in.double()) + (0.0 if first else prev_loss)
        out = acc.clone().cpu()
        steps.append((out, ref, float(loss_out), ref_loss))
        prev = [out[o:o + r * c].double() for (r, c), o in zip(SHAPES, offs)]
        prev_loss = float(loss_out.double())
    return steps, offs, n


@pytest.mark.parametrize("placement", ["flat", "mixed"])
def test_accum_kernel_against_float64(placement):
    dev = _need_gpu()
    steps, offs, n = _run_sequence(dev, placement)
    inside = torch.zeros(n + 64, dtype=torch.bool)
    for (r, c), o in zip(SHAPES, offs):
        inside[o:o + r * c] = True
    assert int((~inside).sum()) > 64                           # there IS padding between the slices
    for k, (out, ref, loss, ref_loss) in enumerate(steps):
        # padding and everything outside the slices: never written
        assert bool((out.view(torch.int32)[~inside] == SENTINEL).all()), k
        worst = 0.0
        for (r, c), o, want in zip(SHAPES, offs, ref):
            got = out[o:o + r * c].double()
            assert bool(torch.isfinite(got).all()), (k, r, c)  # the NaN the accumulator started with did not survive
            err = (got - want).abs()
            worst = max(worst, float((err / want.abs().clamp_min(1e-300)).max()))
            assert bool((err <= EPS * want.abs()).all()), (placement, k, r, c, float((err / want.abs().clamp_min(1e-300)).max()))
        print(f"{placement} launch {k}: worst relative error {worst:.3e} (bound {EPS:.3e}); loss {loss!r} ref {ref_loss!r}")
        assert abs(loss - ref_loss) <= EPS * abs(ref_loss), (k, loss, ref_loss)
    again, _, _ = _run_sequence(dev, placement)                # run to run: the same bits
    for (out, _, loss, _), (out2, _, loss2, _) in zip(steps, again):
        assert torch.equal(out.view(torch.int32), out2.view(torch.int32)) and loss == loss2


def test_accum_without_loss_words_and_refusals():
    dev = _need_gpu()
    from bmhrl_amd import _lib, ops
    table = torch.tensor([[0, 0, 1, 4097, 0, 0, 0]], dtype=torch.int64).to(dev)
    g = torch.randn(4100, generator=torch.Generator().manual_seed(1)).to(dev)
    acc = torch.full((4100,), float("inf"), device=dev)
    ctl = torch.tensor([0.0, 1.0], dtype=torch.float32).to(dev)
    ops.accum_segments(table, 1, 2, g, acc, ctl)               # weight 0 on the first micro-batch: zeros, not 0 * inf
    assert float(acc[:4097].abs().sum()) == 0.0 and bool(torch.isinf(acc[4097:]).all())
    lib = _lib.load()
    T, G, A, C = table.data_ptr(), g.data_ptr(), acc.data_ptr(), ctl.data_ptr()
    one = torch.zeros(1, device=dev).data_ptr()
    s = ops.stream()
    for args in ((None, 1, 2, G, A, C, None, None), (T, 1, 2, None, A, C, None, None), (T, 1, 2, G, None, C, None, None),
                 (T, 1, 2, G, A, None, None, None), (T, 0, 2, G, A, C, None, None), (T, 1, 0, G, A, C, None, None),
                 (T, -1, 2, G, A, C, None, None), (T, 1, 2, G, A, C, one, None), (T, 1, 2, G, A, C, None, one)):
        assert lib.bmhrl_accum_segments(*args, s) == -22, args
    with pytest.raises(RuntimeError, match="GPU only"):
        ops.accum_segments(table, 1, 2, g, acc, torch.zeros(2))
    torch.cuda.synchronize()
