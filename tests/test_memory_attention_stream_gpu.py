"""The LDS-ring streams of csrc/memory_attention.hip (both passes, forward and backward) at the shapes where they can go
wrong: one unit, the key-tile boundary, partial units in dm and in Sk, waves with unequal tile counts, the shortest ring
(dm 1024 with Sk 896), the step's shapes with and without the XCD map.  Against float64 torch from the bf16-rounded inputs;
every operand sits inside NaN so that a read outside it poisons a result, every output inside NaN so that a write outside
its documented extent shows, and ten consecutive calls must agree bit for bit (a missing wait shows as a difference)."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

GUARD = 4096          # elements of NaN on either side of an operand; rows of NaN on either side of an output


def rel_err(a, b):
    a, b = a.double(), b.double()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))


def in_nan(n, dev):
    """n bf16 elements in the middle of a NaN-filled allocation (16-byte aligned)"""
    big = torch.full((n + 2 * GUARD,), float("nan"), dtype=torch.bfloat16, device=dev)
    return big, big[GUARD:GUARD + n]


def only_nan_outside(buf, inside):
    """every element of `inside` finite, every other element of the allocation still the NaN sentinel"""
    nan = torch.isnan(buf)
    return bool(torch.isfinite(buf[inside]).all()) and bool(nan[~inside].all())


@pytest.mark.parametrize("B,H,L,Sk,dm,masked", [
    (1, 1, 1, 1, 32, False),                                                   # one query, one key, one unit
    (1, 2, 30, 31, 64, True), (1, 2, 30, 32, 64, True), (1, 2, 30, 33, 64, True),   # the key-tile boundary
    (1, 3, 7, 250, 96, True),                                                  # dm % 64 != 0; Sk % 8 != 0, % 16 != 0
    (1, 1, 30, 264, 128, True),                                                # nine key tiles: wave 0 has two
    (2, 1, 32, 896, 1024, True),                                               # longest rows, shortest ring
    (4, 4, 30, 256, 1024, True), (4, 4, 30, 800, 128, True),                   # the step's shapes, B2 = 8: XCD map
    (3, 4, 30, 256, 1024, True),                                               # B2 = 6: plain map
])
def test_memory_attention_streams(B, H, L, Sk, dm, masked):
    from bmhrl_amd import ops
    dev = torch.device("cuda:0")
    g = torch.Generator(device="cpu").manual_seed(B * 1000 + Sk + dm)
    B2, Skp, ldt = 2 * B, (Sk + 7) & ~7, (Sk + 15) & ~15
    assert ops.memory_attention_ok(L, Sk, dm)
    mem = torch.randn(B, Sk, dm, generator=g).to(dev)
    y_all, y = in_nan(B * Sk * dm, dev)
    yt_all, yt = in_nan(B * dm * ldt, dev)
    ops.cast_memory(mem, y, yt, B, Sk, dm, ldt)
    assert torch.equal(y.view(B, Sk, dm), mem.bfloat16()) and torch.equal(yt.view(B, dm, ldt)[:, :, :Sk], mem.bfloat16().transpose(1, 2))
    assert float(yt.view(B, dm, ldt)[:, :, Sk:].float().abs().sum()) == 0.0
    assert bool(torch.isnan(y_all[:GUARD]).all() and torch.isnan(y_all[-GUARD:]).all())
    assert bool(torch.isnan(yt_all[:GUARD]).all() and torch.isnan(yt_all[-GUARD:]).all())
    scale = 1.0 / math.sqrt(dm / 4)
    ldq = 2 * H * dm
    QD = torch.zeros(B2 * L, ldq, dtype=torch.bfloat16, device=dev)
    Q = (torch.randn(B2, L, H, dm, generator=g) * 0.4).to(dev).bfloat16()
    dC = (torch.randn(B2, L, H, dm, generator=g) * 0.4).to(dev).bfloat16()
    QD.view(B2, L, 2, H, dm)[:, :, 1] = Q
    QD.view(B2, L, 2, H, dm)[:, :, 0] = dC
    mask = None
    if masked:
        mask = torch.rand(B2, 1, Sk, generator=g) > 0.25
        mask[:, :, 0] = True
        mask[1] = False                                  # a fully masked sample
        mask = mask.to(dev)
    # outputs: NaN rows before and after, NaN columns past the rows' extents
    R, ldp, ldy = B2 * L, 2 * H * Skp + 8, H * dm + 8
    PD_all = torch.full((R + 2 * 40, ldp), float("nan"), dtype=torch.bfloat16, device=dev)
    Cx_all, dQ_all = (torch.full((R + 2 * 40, ldy), float("nan"), dtype=torch.bfloat16, device=dev) for _ in range(2))
    PD, Cx, dQ = PD_all[40:40 + R], Cx_all[40:40 + R], dQ_all[40:40 + R]
    in_p, in_ds, in_y = (torch.zeros_like(t, dtype=torch.bool) for t in (PD_all, PD_all, Cx_all))
    in_p[40:40 + R, :H * Skp] = True
    in_ds[40:40 + R, H * Skp:2 * H * Skp] = True
    in_y[40:40 + R, :H * dm] = True

    def fwd():
        ops.memory_attention(False, QD, H * dm, ldq, y, yt, ldt, PD, ldp, H * Skp, Cx, ldy, mask, Sk, B, B2, H, L, Sk, dm, scale)

    def bwd():
        ops.memory_attention(True, QD, 0, ldq, y, yt, ldt, PD, ldp, H * Skp, dQ, ldy, mask, Sk, B, B2, H, L, Sk, dm, scale)

    fwd()
    assert only_nan_outside(PD_all, in_p) and only_nan_outside(Cx_all, in_y)          # (dS slot: still the sentinel)
    Pv = lambda: PD[:, :2 * H * Skp].view(B2, L, 2, H, Skp)
    memf = mem.bfloat16().double().repeat(2, 1, 1)                                   # sample b2 reads memory b2 % B
    s = torch.einsum("blhd,bkd->blhk", Q.double(), memf) * scale
    if mask is not None:
        s = s.masked_fill(~mask.view(B2, 1, 1, Sk), -1e9)
    p_ref = torch.softmax(s, -1)
    P = Pv()[:, :, 0, :, :Sk]
    e_p = rel_err(P, p_ref)
    e_c = rel_err(Cx[:, :H * dm].view(B2, L, H, dm), torch.einsum("blhk,bkd->blhd", p_ref, memf))
    print(f"P {e_p:.2e} context {e_c:.2e}")
    assert e_p < 1e-2 and e_c < 1e-2
    assert float(Pv()[:, :, 0, :, Sk:].float().abs().sum()) == 0.0
    first = (PD_all.clone(), Cx_all.clone())
    for _ in range(9):
        fwd()
        assert torch.equal(PD_all.view(torch.int16), first[0].view(torch.int16)) and torch.equal(Cx_all.view(torch.int16), first[1].view(torch.int16))

    # backward: P as stored is its input; dS = scale P (dP - sum_k P dP), 0 at masked keys; dQ' = dS mem
    bwd()
    assert only_nan_outside(PD_all, in_p | in_ds) and only_nan_outside(dQ_all, in_y)
    assert torch.equal(Pv()[:, :, 0].contiguous().view(torch.int16), first[0][40:40 + R, :2 * H * Skp].view(B2, L, 2, H, Skp)[:, :, 0].contiguous().view(torch.int16))
    dP = torch.einsum("blhd,bkd->blhk", dC.double(), memf)
    Pf = P.double()
    dS_ref = scale * Pf * (dP - (Pf * dP).sum(-1, keepdim=True))
    if mask is not None:
        dS_ref = dS_ref.masked_fill(~mask.view(B2, 1, 1, Sk), 0.0)
    dS = Pv()[:, :, 1, :, :Sk]
    e_s = rel_err(dS, dS_ref)
    e_q = rel_err(dQ[:, :H * dm].view(B2, L, H, dm), torch.einsum("blhk,bkd->blhd", dS_ref, memf))
    print(f"dS {e_s:.2e} dQ' {e_q:.2e}")
    assert e_s < 1.5e-2 and e_q < 1e-2
    assert float(Pv()[:, :, 1, :, Sk:].float().abs().sum()) == 0.0
    if mask is not None:
        assert float(dS.float().masked_fill(mask.view(B2, 1, 1, Sk), 0.0).abs().sum()) == 0.0
        assert float(dS[1].float().abs().max()) == 0.0 and rel_err(P[1], torch.full_like(P[1].float(), 1.0 / Sk)) < 1e-2
    first = (PD_all.clone(), dQ_all.clone())
    for _ in range(9):
        bwd()
        assert torch.equal(PD_all.view(torch.int16), first[0].view(torch.int16)) and torch.equal(dQ_all.view(torch.int16), first[1].view(torch.int16))
