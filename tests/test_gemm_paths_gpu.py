"""Every main loop, tile, K split and epilogue store path of bmhrl_gemm against a float64 restatement of the header's
contract (tests/gemm_reference.py), element by element.

Operands live in buffers whose padding (columns K .. lda, or M / N .. lda when transposed) and gaps between batch entries
are NaN; outputs start as a sentinel that must survive everywhere outside each batch entry's (M, N) region.  Each case
records the plan bmhrl_gemm_plan reports for it; test_paths_covered asserts that the cases reach every path.  The
tuning switches and BMHRL_DETERMINISTIC are read once per process, so the paths behind them run in child processes."""
import json
import os
import subprocess
import sys
import zlib

import pytest
import torch

from tests import gemm_reference as gr

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENT = -768.0                       # output sentinel (exact in fp32 and bf16)
NAN_BF16 = float("nan")


def pad8(n):
    return (n + 7) & ~7


def pad4(n):
    return (n + 3) & ~3


def case(name, M, N, K, at=False, bt=False, **kw):
    c = dict(name=name, M=M, N=N, K=K, at=at, bt=bt, batch=(1, 1), epi=0, f32=True, bf16=False, alpha=1.0, bias=False,
             per_head=False, relu=False, mask=None, p=0.0, drop_strides=(0, 0, 0), seed_dev=None, residual=False,
             accumulate=False, colsum=False, split=False, ws=False, ldc_pad=4, c_off=0, ldcb_pad=8, aux_off=0, ldaux_pad=8,
             expect={})
    c.update(kw)
    return c


L, P, D, R = 0, 1, 2, 3   # epilogues
CASES = []
# -- the four layouts x both main loops x both default tiles, with tails in M, N and K (M, N in {1, 3, 7}: register loop)
for at in (False, True):
    for bt in (False, True):
        t = f"{'T' if at else 'N'}{'T' if bt else 'N'}"
        CASES += [
            case(f"{t}_m1", 1, 7, 300, at, bt, ldc_pad=1, expect=dict(loop=0, tile=0)),
            case(f"{t}_m3n3", 3, 3, 203, at, bt, bf16=True, expect=dict(loop=0, tile=0)),
            case(f"{t}_m7", 7, 70, 64, at, bt, bias=True, expect=dict(loop=0, tile=0)),
            case(f"{t}_n7", 70, 7, 64, at, bt, bias=True, expect=dict(loop=0, tile=0)),
            case(f"{t}_reg64_k203", 65, 130, 203, at, bt, bf16=True, expect=dict(loop=0, tile=0, vec_ok=1)),
            case(f"{t}_glds64", 130, 72, 192, at, bt, alpha=0.5, expect=dict(loop=1, tile=0, stages=4)),
            case(f"{t}_reg128", 4100, 1030, 203, at, bt, expect=dict(loop=0, tile=1)),
            case(f"{t}_glds128", 4100, 1030, 192, at, bt, bias=True, expect=dict(loop=1, tile=1, stages=2)),
        ]
CASES += [
    # two-stage direct-to-LDS ring on 64 x 64 tiles (more than 448 of them)
    case("glds64_2stage", 1030, 2050, 128, bt=True, expect=dict(loop=1, tile=0, stages=2)),
    # K splits (the vocabulary head's d cat[x, goal]): fp32 atomics into a zeroed C, and the ordered form with accumulate
    case("split_atomic", 480, 364, 10176, bt=True, split=True, alpha=0.5, bias=True, residual=True,
         expect=dict(loop=1, split_form=1)),
    case("split_atomic_reg", 480, 364, 10172, bt=True, split=True, bias=True, residual=True, expect=dict(loop=0, split_form=1)),
    case("split_ordered", 480, 364, 10176, bt=True, split=True, ws=True, alpha=0.5, bias=True, residual=True, accumulate=True,
         expect=dict(loop=1, split_form=2)),
    case("split_ordered_reg_batched", 300, 130, 4100, at=True, bt=True, batch=(1, 2), split=True, ws=True, accumulate=True,
         expect=dict(loop=0, split_form=2)),
    # LINEAR on its three store paths
    case("lin_fast", 200, 300, 1024, f32=False, bf16=True, bias=True, relu=True, p=0.25, expect=dict(epi_path=0)),
    case("lin_fast_reg", 5, 300, 300, f32=False, bf16=True, bias=True, p=0.1, expect=dict(loop=0, epi_path=0)),
    case("lin_vec", 200, 300, 1024, bf16=True, ldcb_pad=4, bias=True, relu=True, mask="mn", p=0.25, residual=True, alpha=0.75,
         expect=dict(epi_path=2, vec_ok=1)),
    case("lin_vec_accumulate", 200, 300, 256, bias=True, residual=True, accumulate=True, expect=dict(epi_path=2, vec_ok=1)),
    case("lin_scalar_ldc", 200, 300, 1024, ldc_pad=1, bias=True, mask="mn", p=0.25, residual=True, expect=dict(vec_ok=0)),
    case("lin_scalar_off", 70, 200, 320, c_off=1, bias=True, relu=True, accumulate=True, expect=dict(vec_ok=0)),
    case("lin_scalar_bf16", 70, 203, 256, f32=False, bf16=True, ldcb_pad=1, bias=True, relu=True, p=0.5, expect=dict(vec_ok=0)),
    case("lin_keymask", 30, 200, 256, bias=True, mask="key", expect=dict(vec_ok=1)),
    # PROB: fast (key mask), generic vector (per-(m, n) mask), generic scalar (odd ldcb)
    case("prob_fast", 30, 200, 256, bt=True, epi=P, f32=False, bf16=True, mask="key", alpha=0.0625, expect=dict(epi_path=1)),
    case("prob_fast_nomask", 70, 130, 320, epi=P, f32=False, bf16=True, alpha=0.0625, expect=dict(epi_path=1)),
    case("prob_vec", 30, 200, 256, bt=True, epi=P, bf16=True, mask="mn", alpha=0.0625, expect=dict(epi_path=2, vec_ok=1)),
    case("prob_scalar", 30, 203, 256, bt=True, epi=P, f32=False, bf16=True, ldcb_pad=1, mask="key", alpha=0.0625,
         expect=dict(epi_path=2, vec_ok=0)),
    # DSCORE: fast, generic vector (fp32 out + per-(m, n) mask), scalar (aux at a 4-byte offset)
    case("dscore_fast", 30, 200, 256, epi=D, f32=False, bf16=True, mask="key", alpha=0.0625, expect=dict(epi_path=1)),
    case("dscore_vec", 30, 200, 256, epi=D, bf16=True, mask="mn", alpha=0.0625, expect=dict(epi_path=2, vec_ok=1)),
    case("dscore_scalar", 30, 200, 256, epi=D, f32=False, bf16=True, aux_off=2, mask="key", alpha=0.0625,
         expect=dict(epi_path=2, vec_ok=0)),
    # RELU_BWD (no fast path): vector and scalar, both loops
    case("relubwd_vec", 200, 300, 1024, epi=R, bf16=True, ldcb_pad=4, alpha=1.25, colsum=True, expect=dict(epi_path=2, vec_ok=1)),
    case("relubwd_scalar", 70, 130, 203, epi=R, ldc_pad=1, alpha=1.25, expect=dict(loop=0, vec_ok=0)),
    # batched problems with per-head bias / colsum slices, residual strides and explicit dropout ids
    case("batched_vec", 64, 96, 128, bt=True, batch=(2, 3), bf16=True, ldcb_pad=4, bias=True, per_head=True, colsum=True,
         residual=True, mask="mn", p=0.2, drop_strides=(100003, 20011, 307), relu=True, expect=dict(vec_ok=1)),
    case("batched_scalar", 30, 97, 72, at=True, batch=(3, 2), ldc_pad=1, bias=True, per_head=True, colsum=True,
         residual=True, p=0.3, drop_strides=(50021, 9001, 211), expect=dict(loop=0, vec_ok=0)),
    case("batched_fast", 33, 72, 256, bt=True, batch=(2, 2), f32=False, bf16=True, bias=True, per_head=True, p=0.3,
         drop_strides=(9000, 3000, 80), expect=dict(epi_path=0)),
    case("batched_prob", 30, 130, 256, bt=True, batch=(2, 4), epi=P, f32=False, bf16=True, mask="key", alpha=0.0625,
         expect=dict(epi_path=1)),
    case("batched_dscore", 30, 130, 256, batch=(2, 4), epi=D, f32=False, bf16=True, mask="key", alpha=0.0625,
         expect=dict(epi_path=1)),
    case("colsum_plain", 300, 200, 256, colsum=True, expect=dict(vec_ok=1)),
]
# the beam decoder's token steps (decode.py: M = B * beam rows against the 1024-wide model): Q projection (bf16 out + bias)
# and output projection (fp32 out + bias + residual)
for Bn in (1, 3, 16):
    for beam in (1, 4):
        M = Bn * beam
        CASES += [
            case(f"beam_q_{Bn}x{beam}", M, 1024, 300, f32=False, bf16=True, ldcb_pad=0, bias=True, expect=dict(epi_path=0)),
            case(f"beam_o_{Bn}x{beam}", M, 300, 1024, ldc_pad=0, bias=True, residual=True,
                 expect=dict(loop=0 if M < 8 else 1)),
        ]
BY_NAME = {c["name"]: c for c in CASES}
assert len(BY_NAME) == len(CASES)


# ---- operands
def _strided_buffer(shape4, ld, dtype, fill, dev, gap, align=8):
    """flat buffer holding a [b1, b2, rows, cols] view with leading dim ld, a gap between batch entries; returns (buf,
    view, (sb1, sb2))"""
    b1, b2, rows, cols = shape4
    sb2 = ((rows * ld + gap + align - 1) // align) * align
    sb1 = ((b2 * sb2 + gap + align - 1) // align) * align
    buf = torch.full((b1 * sb1 + 64,), fill, dtype=dtype, device=dev)
    view = buf.as_strided((b1, b2, rows, cols), (sb1, sb2, ld, 1))
    return buf, view, (sb1, sb2)


def make(c, dev):
    """allocate and fill the case's operands; returns the launch context (descriptor inputs, reference inputs)"""
    from bmhrl_amd import ops
    M, N, K, (b1, b2) = c["M"], c["N"], c["K"], c["batch"]
    g = torch.Generator(device="cpu").manual_seed(zlib.crc32(c["name"].encode()))
    A = torch.randn(b1, b2, M, K, generator=g).to(torch.bfloat16).to(dev)
    Bm = torch.randn(b1, b2, K, N, generator=g).to(torch.bfloat16).to(dev)
    x = dict(case=c, A=A, B=Bm)
    a_rows, a_cols = (K, M) if c["at"] else (M, K)
    lda = pad8(a_cols) + 8
    x["Abuf"], av, x["a_sb"] = _strided_buffer((b1, b2, a_rows, a_cols), lda, torch.bfloat16, NAN_BF16, dev, 24)
    av.copy_(A.transpose(-1, -2) if c["at"] else A)
    b_rows, b_cols = (K, N) if c["bt"] else (N, K)
    ldb = pad8(b_cols) + 16
    x["Bbuf"], bv, x["b_sb"] = _strided_buffer((b1, b2, b_rows, b_cols), ldb, torch.bfloat16, NAN_BF16, dev, 40)
    bv.copy_(Bm if c["bt"] else Bm.transpose(-1, -2))
    x["lda"], x["ldb"] = lda, ldb
    if c["f32"]:
        ldc = pad4(N) + c["ldc_pad"] if c["ldc_pad"] != 1 else N + (1 if N % 2 == 0 else 2)
        x["ldc"] = ldc
        x["Cbuf"], cv, x["c_sb"] = _strided_buffer((b1, b2, M, N), ldc, torch.float32, SENT, dev, 12,
                                                   align=4 if c["ldc_pad"] != 1 else 1)
        x["c_off"] = c["c_off"]
        if c["c_off"]:
            cv = x["Cbuf"][c["c_off"]:].as_strided((b1, b2, M, N), (x["c_sb"][0], x["c_sb"][1], ldc, 1))
        x["Cview"] = cv
        if c["split"] and not c["ws"]:
            cv.zero_()                               # (allow_split_k: C is zero-initialised)
        if c["accumulate"]:
            cv.copy_(torch.randn(b1, b2, M, N, generator=g).to(dev))
        x["C_old"] = cv.double().clone()
    if c["bf16"]:
        ldcb = pad8(N) + c["ldcb_pad"] if c["ldcb_pad"] != 1 else N + (1 if N % 2 == 0 else 2)
        x["ldcb"] = ldcb
        x["Cbbuf"], cbv, x["cb_sb"] = _strided_buffer((b1, b2, M, N), ldcb, torch.bfloat16, SENT, dev, 16,
                                                      align=8 if c["ldcb_pad"] in (0, 8) else (4 if c["ldcb_pad"] == 4 else 1))
        x["Cbview"] = cbv
    if c["bias"]:
        if c["per_head"]:
            x["biasbuf"], bview, x["bias_sb"] = _strided_buffer((b1, b2, 1, N), pad4(N), torch.float32, float("nan"), dev, 4, 4)
            bview.copy_(torch.randn(b1, b2, 1, N, generator=g).to(dev))
        else:                                         # one bias for every batch entry
            x["biasbuf"] = torch.full((pad4(N) + 8,), float("nan"), device=dev)
            x["biasbuf"][:N] = torch.randn(N, generator=g).to(dev)
            bview = x["biasbuf"][:N].view(1, 1, 1, N).expand(b1, b2, 1, N)
            x["bias_sb"] = (0, 0)
        x["bias"] = bview.double()
    if c["residual"]:
        ldr = pad4(N) + 4
        x["ldr"] = ldr
        x["Rbuf"], rv, x["r_sb"] = _strided_buffer((b1, b2, M, N), ldr, torch.float32, float("nan"), dev, 8, 4)
        rv.copy_(torch.randn(b1, b2, M, N, generator=g).to(dev))
        x["res"] = rv.double()
    if c["mask"] is not None:
        sm = 0 if c["mask"] == "key" else N + 5
        rows = 1 if sm == 0 else M
        msb1 = rows * max(sm, N) + 11
        x["maskbuf"] = torch.full((b1 * msb1 + 64,), 255, dtype=torch.uint8, device=dev)
        keep = (torch.rand(b1, rows, N, generator=g) > 0.2).to(torch.uint8)
        keep[:, :, 0] = 1                             # (no fully masked PROB row: rowvec2 stays > 0)
        mv = x["maskbuf"].as_strided((b1, rows, N), (msb1, sm if sm else 0, 1))
        mv.copy_(keep.to(dev))
        x["mask_sb1"], x["mask_sm"] = msb1, sm
        x["mask"] = (keep.to(dev) != 0).view(b1, 1, rows, N).expand(b1, b2, M, N)
    if c["colsum"]:
        x["csbuf"], csv, x["cs_sb"] = _strided_buffer((b1, b2, 1, N), pad4(N), torch.float32, SENT, dev, 4, 4)
        csv.copy_(torch.randn(b1, b2, 1, N, generator=g).to(dev))
        x["csview"] = csv
        x["cs_old"] = csv.double().clone()
    acc = A.double() @ Bm.double()
    absacc = A.double().abs() @ Bm.double().abs()
    x["acc"], x["absacc"] = acc, absacc
    if c["epi"] in (P, D):
        # row vectors [b1, b2, M] with their own strides: the row max / row sum of the masked scores (PROB), delta (DSCORE)
        xs = c["alpha"] * acc
        if c["mask"] is not None:
            xs = torch.where(x["mask"], xs, torch.full_like(xs, gr.NEG_MASK))
        rvm = xs.amax(-1)
        x["rvbuf"], rvv, x["rv_sb"] = _strided_buffer((b1, b2, 1, M), M + 3, torch.float32, float("nan"), dev, 3, 1)
        x["rv2buf"] = torch.full_like(x["rvbuf"], float("nan"))
        rv2v = x["rv2buf"].as_strided((b1, b2, 1, M), (x["rv_sb"][0], x["rv_sb"][1], M + 3, 1))
        if c["epi"] == P:
            rvv.copy_(rvm.float().view(b1, b2, 1, M))
            rv2v.copy_(torch.exp(xs - rvv.double().view(b1, b2, M, 1)).sum(-1).float().view(b1, b2, 1, M))
        else:
            rvv.copy_(torch.randn(b1, b2, 1, M, generator=g).to(dev) * 3)
        x["rowvec"] = rvv.double().view(b1, b2, M, 1)
        x["rowvec2"] = rv2v.double().view(b1, b2, M, 1)
    if c["epi"] in (D, R):
        ldaux = pad8(N) + c["ldaux_pad"]
        x["ldaux"] = ldaux
        x["auxbuf"], auxv, x["aux_sb"] = _strided_buffer((b1, b2, M, N), ldaux, torch.bfloat16, NAN_BF16, dev, 8)
        vals = torch.rand(b1, b2, M, N, generator=g) if c["epi"] == D else torch.randn(b1, b2, M, N, generator=g)
        x["aux_off"] = c["aux_off"]
        if c["aux_off"]:
            auxv = x["auxbuf"][c["aux_off"]:].as_strided((b1, b2, M, N), (x["aux_sb"][0], x["aux_sb"][1], ldaux, 1))
        auxv.copy_(vals.to(torch.bfloat16).to(dev))
        x["aux"] = auxv.double()
    if c["ws"]:
        n = ops.gemm_splits(M, N, K, b1 * b2)
        x["wsbuf"] = torch.full((n * b1 * b2 * M * N,), float("nan"), device=dev)
    if c["p"] > 0 and c["seed_dev"] is not None:
        x["seed_dev"] = torch.tensor([c["seed_dev"]], dtype=torch.int64, device=dev)
    return x


def descriptor(x):
    from bmhrl_amd import ops
    c = x["case"]
    kw = dict(lda=x["lda"], ldb=x["ldb"], a_trans=c["at"], b_trans=c["bt"], batch=c["batch"], a_strides=x["a_sb"],
              b_strides=x["b_sb"], epilogue=c["epi"], alpha=c["alpha"], relu=c["relu"], accumulate=c["accumulate"],
              allow_split_k=c["split"], dropout_p=c["p"], seed=c.get("seed", 1234567), drop_strides=c["drop_strides"])
    if c["f32"]:
        kw.update(C_f32=x["Cbuf"], ldc=x["ldc"], c_strides=x["c_sb"], c_off=x["c_off"])
    if c["bf16"]:
        kw.update(C_bf16=x["Cbbuf"], ldcb=x["ldcb"], cb_strides=x["cb_sb"])
    if c["bias"]:
        kw.update(bias=x["biasbuf"], bias_sb1=x["bias_sb"][0], bias_sb2=x["bias_sb"][1])
    if c["residual"]:
        kw.update(residual=x["Rbuf"], ldr=x["ldr"], r_strides=x["r_sb"])
    if c["mask"] is not None:
        kw.update(mask=x["maskbuf"], mask_sb1=x["mask_sb1"], mask_sm=x["mask_sm"])
    if c["colsum"]:
        kw.update(colsum=x["csbuf"], colsum_sb1=x["cs_sb"][0], colsum_sb2=x["cs_sb"][1])
    if c["epi"] in (P, D):
        kw.update(rowvec=x["rvbuf"], rv_strides=x["rv_sb"])
    if c["epi"] == P:
        kw.update(rowvec2=x["rv2buf"])
    if c["epi"] in (D, R):
        kw.update(aux=x["auxbuf"], ldaux=x["ldaux"], aux_strides=x["aux_sb"], aux_off=x["aux_off"])
    if c["ws"]:
        kw.update(split_ws=x["wsbuf"])
    if "seed_dev" in x:
        kw.update(seed_dev=x["seed_dev"])
    return ops.gemm_desc(x["Abuf"], x["Bbuf"], c["M"], c["N"], c["K"], **kw)


# ---- reference and checks
def reference(x, seed_add=0):
    """(R, S) of the case's output: value and bound magnitude (PROB: the bound relative to R)"""
    c = x["case"]
    (b1, b2), M, N = c["batch"], c["M"], c["N"]
    acc, absacc = x["acc"], x["absacc"]
    mask = x.get("mask")
    if c["epi"] == L:
        keep, scale = None, 1.0
        if c["p"] > 0:
            seed = (c.get("seed", 1234567) + seed_add) & 0xFFFFFFFFFFFFFFFF
            keep = torch.from_numpy(gr.keep_mask(c["p"], seed, M, N, b1, b2, c["drop_strides"])).to(acc.device)
            scale = gr.dropout_scale(c["p"])
        return gr.linear_ref(acc, absacc, alpha=c["alpha"], bias=x.get("bias"), relu=c["relu"], mask=mask, keep=keep, scale=scale,
                             residual=x.get("res"), old=x["C_old"] if c["accumulate"] else None)
    if c["epi"] == P:
        return gr.prob_ref(acc, absacc, alpha=c["alpha"], rowvec=x["rowvec"], rowvec2=x["rowvec2"], mask=mask)
    if c["epi"] == D:
        return gr.dscore_ref(acc, absacc, alpha=c["alpha"], rowvec=x["rowvec"], aux=x["aux"], mask=mask)
    return gr.relu_bwd_ref(acc, absacc, alpha=c["alpha"], aux=x["aux"])


def _region(buf, view):
    inside = torch.zeros(buf.numel(), dtype=torch.bool, device=buf.device)
    off = view.storage_offset() - buf.storage_offset()
    inside[off:].as_strided(view.shape, view.stride()).fill_(True)
    return inside


def _report(what, ok, out, R, bound):
    if bool(ok.all()):
        return
    bad = (~ok).nonzero()
    i = tuple(bad[0].tolist())
    raise AssertionError(f"{what}: {bad.shape[0]} of {ok.numel()} elements outside the bound; first at {i}: "
                         f"got {float(out[i])!r}, want {float(R[i])!r} +- {float(bound[i])!r}")


def check(x, seed_add=0, det=False):
    c = x["case"]
    R, S = reference(x, seed_add)
    if c["epi"] == P:
        bound32 = R * S + 1e-30
        boundb = R * S * 1.01 + gr.BF16_U * R + 1e-30
    else:
        bound32 = gr.TAU * S
        boundb = gr.TAU * S * 1.01 + gr.BF16_U * R.abs()
    name = c["name"]
    if c["f32"]:
        out = x["Cview"].double()
        _report(f"{name} fp32", gr.within(out, R, bound32), out, R, bound32)
        assert torch.equal(x["Cbuf"][~_region(x["Cbuf"], x["Cview"])],
                           torch.full_like(x["Cbuf"], SENT)[~_region(x["Cbuf"], x["Cview"])]), f"{name}: fp32 store outside (M, N)"
    if c["bf16"]:
        out = x["Cbview"].double()
        _report(f"{name} bf16", gr.within(out, R, boundb), out, R, boundb)
        outside = ~_region(x["Cbbuf"], x["Cbview"])
        assert bool((x["Cbbuf"][outside].float() == SENT).all()), f"{name}: bf16 store outside (M, N)"
    if c["colsum"]:
        M = c["M"]
        want = x["cs_old"] + R.sum(-2, keepdim=True)
        bnd = bound32.sum(-2, keepdim=True) + M * 2.0 ** -24 * (R.abs().sum(-2, keepdim=True) + x["cs_old"].abs())
        if det and c["bf16"]:
            # (the ordered pass sums the STORED output, the bf16 one when there is one: one bf16 rounding per term)
            bnd = bnd + gr.BF16_U * R.abs().sum(-2, keepdim=True)
        out = x["csview"].double()
        _report(f"{name} colsum", gr.within(out, want, bnd), out, want, bnd)
        outside = ~_region(x["csbuf"], x["csview"])
        assert bool((x["csbuf"][outside] == SENT).all()), f"{name}: colsum store outside [0, N)"


PLANS = {}


def run(c, dev, det=False):
    from bmhrl_amd import ops, _lib
    import ctypes as C
    x = make(c, dev)
    d = descriptor(x)
    plan = ops.gemm_plan(d)
    PLANS[c["name"]] = plan
    for k, v in c["expect"].items():
        assert plan[k] == v, f"{c['name']}: plan {plan} expected {k} = {v}"
    _lib.check(_lib.load().bmhrl_gemm(C.byref(d), ops.stream()), "bmhrl_gemm")
    torch.cuda.synchronize()
    check(x, det=det)
    return x, plan


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from bmhrl_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


@pytest.mark.parametrize("name", [c["name"] for c in CASES])
def test_gemm_path(dev, name):
    run(BY_NAME[name], dev)


def test_accumulate_refusals(dev):
    """accumulate goes with the fp32 output alone (not Cb, not colsum) and, split, with the ordered form only: the atomic
    form (no or too small a workspace) is refused with -22 instead of adding atomics into a live C"""
    import ctypes as C
    from bmhrl_amd import _lib, ops
    for kw in (dict(bf16=True), dict(colsum=True)):
        x = make(case("refuse", 64, 64, 64, accumulate=True, **kw), dev)
        assert _lib.load().bmhrl_gemm(C.byref(descriptor(x)), ops.stream()) == -22
    x = make(case("refuse_split", 480, 364, 10176, bt=True, split=True, accumulate=True), dev)
    d = descriptor(x)
    small = torch.zeros(8, device=dev)
    d.split_ws, d.split_ws_elems = small.data_ptr(), 8
    assert _lib.load().bmhrl_gemm(C.byref(d), ops.stream()) == -22
    torch.cuda.synchronize()
    assert bool((x["Cview"] == x["C_old"].float()).all())      # untouched


def test_seed_dev_changes_the_mask(dev):
    """seed_dev[0] is added to the seed at run time: two launches with different device words give two different keep
    masks, each exactly the one the header's element id and dropout_bits give"""
    from bmhrl_amd import _lib, ops
    import ctypes as C
    for fast in (False, True):
        c = case(f"seed_dev_{fast}", 96, 136, 128, f32=not fast, bf16=fast, bias=True, p=0.4, seed=99, seed_dev=5,
                 expect=dict(epi_path=0 if fast else 2))
        x = make(c, dev)
        outs = []
        for word in (5, 5 + (1 << 33)):
            x["seed_dev"].fill_(word)
            d = descriptor(x)
            assert ops.gemm_plan(d)["epi_path"] == (0 if fast else 2)
            _lib.check(_lib.load().bmhrl_gemm(C.byref(d), ops.stream()), "bmhrl_gemm")
            torch.cuda.synchronize()
            check(x, seed_add=word)
            outs.append((x["Cbview"] if fast else x["Cview"]).clone())
        assert not torch.equal(outs[0] == 0, outs[1] == 0)


GROUPS = [
    # (problems, expected gemm_group_kernel launches): caption-side weight gradients (K = B L, register loop, 64 x 64)
    ([dict(M=64, N=300, K=300)], 0),
    ([dict(M=64, N=300, K=300), dict(M=300, N=300, K=300, bias=True, relu=True)], 1),
    ([dict(M=64, N=300, K=300), dict(M=7, N=33, K=100, colsum=True), dict(M=130, N=70, K=203, p=0.3, bias=True)], 1),
    ([dict(M=64, N=300, K=300), dict(M=300, N=64, K=300, split=True), dict(M=480, N=364, K=10172, split=True),
      dict(M=3, N=1030, K=300, ldc_pad=1, residual=True)], 1),
    ([dict(M=64, N=300, K=300), dict(M=300, N=300, K=300), dict(M=130, N=70, K=203), dict(M=64, N=64, K=300),
      dict(M=5, N=9, K=11, bias=True)], 1),
    # a mix that falls back to one by one: a direct-to-LDS problem among them
    ([dict(M=64, N=300, K=300), dict(M=64, N=300, K=256, bias=True)], 0),
]


@pytest.mark.parametrize("gi", range(len(GROUPS)))
def test_gemm_group(dev, gi):
    from bmhrl_amd import _lib, ops
    probs, launches = GROUPS[gi]
    xs = [make(case(f"group{gi}_{i}", at=True, bt=True, **p), dev) for i, p in enumerate(probs)]
    ds = [descriptor(x) for x in xs]
    assert ops.gemm_group_plan(ds) == launches
    PLANS[f"group{gi}"] = dict(group_launches=launches, n=len(ds))
    arr = (_lib.GemmDesc * len(ds))(*ds)
    _lib.check(_lib.load().bmhrl_gemm_group(arr, len(ds), ops.stream()), "bmhrl_gemm_group")
    torch.cuda.synchronize()
    for x in xs:
        check(x)


# paths the default process must reach (the tuning switches' paths: the child tests below)
REQUIRED = {
    "loop": {0, 1}, "tile": {0, 1}, "stages": {2, 4}, "split_form": {0, 1, 2}, "epi_path": {0, 1, 2}, "vec_ok": {0, 1},
}


def test_paths_covered(dev):
    """the union of the cases' plans covers every path; a case whose plan was not recorded (deselected) is planned here"""
    from bmhrl_amd import ops
    for c in CASES:
        if c["name"] not in PLANS:
            PLANS[c["name"]] = ops.gemm_plan(descriptor(make(c, dev)))
    plans = [PLANS[c["name"]] for c in CASES]
    missing = []
    for field, values in REQUIRED.items():
        got = {p[field] for p in plans}
        missing += [f"{field}={v}" for v in sorted(values - got)]
    # every layout on both loops and both default tiles
    combos = {(c["at"], c["bt"], PLANS[c["name"]]["loop"], PLANS[c["name"]]["tile"]) for c in CASES}
    missing += [f"layout {at:d}{bt:d} loop {lp} tile {tl}" for at in (0, 1) for bt in (0, 1) for lp in (0, 1) for tl in (0, 1)
                if (bool(at), bool(bt), lp, tl) not in combos]
    # every epilogue kind on each store path it has
    kinds = {(c["epi"], PLANS[c["name"]]["epi_path"], PLANS[c["name"]]["vec_ok"]) for c in CASES}
    want = [(L, 0, 1), (L, 2, 1), (L, 2, 0), (P, 1, 1), (P, 2, 1), (P, 2, 0), (D, 1, 1), (D, 2, 1), (D, 2, 0), (R, 2, 1), (R, 2, 0)]
    missing += [f"epilogue {e} path {pth} vec_ok {v}" for e, pth, v in want if (e, pth, v) not in kinds]
    # M, N below 8 and the beam decoder's row counts
    ms = {c["M"] for c in CASES}
    missing += [f"M={m}" for m in (1, 3, 4, 7, 12, 16, 64) if m not in ms]
    missing += [f"N={n}" for n in (3, 7) if n not in {c["N"] for c in CASES}]
    assert not missing, f"paths no case reaches: {missing}"


# ---- paths behind switches read once per process: fresh child processes
CHILDREN = {
    "w8": (dict(BMHRL_GEMM_W8="2"),
           [case(f"w8_{int(at)}{int(bt)}", 4100, 1030, 192, at, bt, bias=True, expect=dict(loop=2, tile=1, stages=3))
            for at in (False, True) for bt in (False, True)]
           + [case("w8_bf16", 2048, 2048, 256, f32=False, bf16=True, bias=True, p=0.1, expect=dict(loop=2, epi_path=0))]),
    "tile3_xcd": (dict(BMHRL_GEMM_TILE="3", BMHRL_GEMM_XCD="1"),
                  [case(f"t3_{int(at)}{int(bt)}", 1000, 1000, 128, at, bt, bias=True, expect=dict(loop=1, tile=2))
                   for at in (False, True) for bt in (False, True)]
                  + [case("t3_reg", 130, 70, 203, bt=True, expect=dict(loop=0, tile=2)),
                     case("t3_prob", 30, 200, 256, bt=True, epi=P, f32=False, bf16=True, mask="key", alpha=0.0625,
                          expect=dict(tile=2, epi_path=1))]),
    "noglds_bigsplit": (dict(BMHRL_GEMM_NOGLDS="1", BMHRL_GEMM_BIGSPLIT="1"),
                        [case("nb_atomic", 480, 364, 10176, bt=True, split=True, bias=True, residual=True,
                              expect=dict(loop=0, tile=1, split_form=1)),
                         case("nb_ordered", 480, 364, 10176, bt=True, split=True, ws=True, accumulate=True,
                              expect=dict(loop=0, tile=1, split_form=2)),
                         case("nb_layouts", 130, 72, 192, True, True, expect=dict(loop=0))]),
    "deterministic": (dict(BMHRL_DETERMINISTIC="1"),
                      [case("det_split", 480, 364, 10176, bt=True, split=True, bias=True, expect=dict(splits=1, split_form=0)),
                       case("det_colsum", 200, 300, 1024, bf16=True, ldcb_pad=4, epi=R, colsum=True,
                            expect=dict(ordered_colsum=1)),
                       case("det_colsum_batched", 64, 96, 128, bt=True, batch=(2, 3), bias=True, per_head=True, colsum=True,
                            residual=True, p=0.2, drop_strides=(100003, 20011, 307), expect=dict(ordered_colsum=1))]),
}


def child(which, out_path):
    """run one child's cases (the parent started this process with the child's environment); two launches of each must be
    bit-identical under BMHRL_DETERMINISTIC"""
    from bmhrl_amd import _lib, ops
    import ctypes as C
    env, cases = CHILDREN[which]
    for k, v in env.items():
        assert os.environ.get(k) == v, f"child {which} started without {k}={v}"
    dev = torch.device("cuda:0")
    _lib.load()
    det = which == "deterministic"
    assert bool(_lib.load().bmhrl_deterministic_enabled()) == det
    plans = {}
    for c in cases:
        x, plans[c["name"]] = run(c, dev, det=det)
        if det:
            first = [x[k].clone() for k in ("Cbuf", "Cbbuf", "csbuf") if k in x]
            x2 = make(c, dev)
            _lib.check(_lib.load().bmhrl_gemm(C.byref(descriptor(x2)), ops.stream()), "bmhrl_gemm")
            torch.cuda.synchronize()
            second = [x2[k] for k in ("Cbuf", "Cbbuf", "csbuf") if k in x2]
            for a, b in zip(first, second):
                assert torch.equal(a.view(torch.int16) if a.dtype == torch.bfloat16 else a.view(torch.int32),
                                   b.view(torch.int16) if b.dtype == torch.bfloat16 else b.view(torch.int32)), c["name"]
    with open(out_path, "w") as f:
        json.dump(plans, f)


_CHILD = "import sys; sys.path.insert(0, sys.argv[1]); from tests.test_gemm_paths_gpu import child; child(sys.argv[2], sys.argv[3])"


@pytest.mark.parametrize("which", list(CHILDREN))
def test_switch_paths_in_child(dev, tmp_path, which):
    env_add, cases = CHILDREN[which]
    env = {k: v for k, v in os.environ.items() if not (k.startswith("BMHRL_GEMM_") or k == "BMHRL_DETERMINISTIC")}
    env.update(env_add)
    out = tmp_path / f"{which}.json"
    r = subprocess.run([sys.executable, "-c", _CHILD, ROOT, which, str(out)], env=env, cwd=ROOT, capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, f"child {which} exited {r.returncode}:\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}"
    plans = json.loads(out.read_text())
    assert sorted(plans) == sorted(c["name"] for c in cases)
    for c in cases:
        for k, v in c["expect"].items():
            assert plans[c["name"]][k] == v, (c["name"], k, plans[c["name"]])
