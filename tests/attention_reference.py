"""Plain float64 restatement of the fused attention contract (include/bmhrl_hip.h), its per-element error bounds, an emulation
of the roundings the kernels are documented to do, and the inputs / case tables of tests/test_attention_paths_gpu.py.

Shared by tests/test_attention_paths_gpu.py (every fused forward and backward kernel against this reference) and
tests/test_attention_reference_cpu.py (which shows on the CPU that the bounds are tight enough: a correct emulation of the
kernels' roundings stays within HALF of them, and deliberately wrong ones break them).  Everything here is torch float64 on
the CPU; nothing restates a kernel -- only what the header promises:

    S = scale * Q K^T, masked_fill(mask == 0, -1e9);  P = softmax(S);  O = P V          (a fully masked row is uniform)
    shared form (head dimension 128): K = V = X (B, Sk, 128) for every head, Q = Qp (B, Sq, H, 128)
    backward of the shared form (top of csrc/attention_bwd.h):
        dP = dCx X^T;  delta = rowsum(dCx * Cx);  dS = P (dP - delta) scale, 0 at masked keys
        dQp = dS X;    dX = sum_h (P^T dCx + dS^T Qp)

Error bounds (u = 2^-9 for bf16 operands, 2^-11 for fp16; P / dS are rounded to the operand type before the second product,
O / dQp are rounded once, dX is fp32):

    bound_O  = u |O|  + 2u sum_k P[k] |V[k,d]|      + 2^-20 max_k |V[k,d]|                      (keys with P > 0)
    bound_dQ = u |dQ| + 2u sum_k |dS[k]| |X[k,d]|   + (2^-20 max_k |dS[k]| + c) max_k |X[k,d]|
    bound_dX = 2u sum_{h,q} (P |dCx| + |dS| |Qp|)   + 2^-20 (max P max |dCx[.,d]| + max |dS| max |Qp[.,d]|) + c sum_{h,q} P |Qp|
    c = dk 2^-24 scale max |dCx| max |X|: the fp32 error of dP - delta where the two cancel (see backward())

(u = 2^-9 is half of the largest round-to-nearest error of bf16, 2^-8: one rounding of a result with a single dominant term can
use u |O| + 2u |O| up to two thirds.  That is why the inputs below avoid rows that put arbitrary weights on a few keys.)
The 2u terms cover the rounding of P (dS) in the product (and in the row sum, should a kernel sum the rounded values); the
2^-20 floors cover fp32 accumulation over at most 10 112 keys (10 112 * 2^-24 < 2^-10 of the largest term, and the
roundings do not all point one way).

Inputs (make_inputs): a bound of a few u of sum_k P |V| only means something when that sum is not much larger than what an
error moves.  So values carry a signature -- key k holds (-1)^k * mag(k) * (a +-1 pattern of its pair of keys), patterns of
different pairs orthogonal (Sylvester-Hadamard rows) -- and the query rows of a case mix: rows that attend sharply (more than
15 nats) to the first, the last and a middle valid key, uniform and near-uniform rows, and "staircase" rows whose score
rises at the last key of every 32-key tile, by 0.2 nats (the running maximum moves, no rescale) or by 16 nats (a lazy
rescale in every tile).  Scores come from matched filters on the key patterns, so they are exact in fp32 up to a few ulps.
"""
from __future__ import annotations

import functools
import math

import numpy as np
import torch

try:
    from . import gemm_reference as gref
except ImportError:      # (imported as a top-level module)
    import gemm_reference as gref

NEG_MASK = -1e9
F64 = torch.float64
UNIT = {torch.bfloat16: 2.0 ** -9, torch.float16: 2.0 ** -11}
FLOOR = 2.0 ** -20
LAG_MAX = 8 * math.log(2.0)          # the online kernels keep a running maximum that lags by less than 2^8
# Statistics: lse = row_max + log(row_sum).  tests/test_attention_reference_cpu.py evaluates the same quantity in plain torch
# fp32 on every table case; its largest deviation from float64 is LSE_FP32_DEV (asserted there), the GPU tolerance 8 times
# that (hardware exp2 / log2, another summation order).
LSE_FP32_DEV = 1.6e-4
LSE_TOL = 8 * LSE_FP32_DEV


def rnd(x: torch.Tensor, dtype) -> torch.Tensor:
    """round to the operand type and back (round to nearest even, as the kernels' conversions)"""
    return x.to(dtype).to(F64)


# ------------------------------------------------------------------------------------------------------------ reference
def _kv(V: torch.Tensor, H: int) -> torch.Tensor:
    """(B, Sk, Hv, dk) with Hv == H (head split) or 1 (shared) -> (B, H, Sk, dk) view"""
    return V.permute(0, 2, 1, 3).expand(-1, H, -1, -1)


def keep_of(mask, B, Sq, Sk) -> torch.Tensor:
    """bool (B, Sq or 1, Sk): True where the key takes part; mask None, (B, Sk) or (B, Sq, Sk), nonzero = keep"""
    if mask is None:
        return torch.ones(B, 1, Sk, dtype=torch.bool)
    m = mask != 0
    return m[:, None, :] if m.dim() == 2 else m


def scores(Q, K, mask, scale):
    """Q (B, Sq, H, dk), K (B, Sk, Hk, dk) float64 -> masked scaled scores (B, H, Sq, Sk) and keep (B, 1, Sq or 1, Sk)"""
    B, Sq, H, _ = Q.shape
    Sk = K.shape[1]
    s = torch.einsum("bqhd,bhkd->bhqk", Q, _kv(K, H)) * scale
    keep = keep_of(mask, B, Sq, Sk)[:, None]
    return s.masked_fill(~keep, NEG_MASK), keep


def forward(Q, K, V, mask, scale, dtype=torch.bfloat16):
    """float64 reference of one attention.  Returns a dict: O (B, Sq, H, dk), lse / max (B, H, Sq), P (B, H, Sq, Sk), s, keep,
    bound (as O) and full (B, 1, Sq or 1): rows whose keys are all masked"""
    H = Q.shape[2]
    s, keep = scores(Q, K, mask, scale)
    mx = s.max(-1).values
    e = torch.exp(s - mx[..., None])
    l = e.sum(-1)
    P = e / l[..., None]
    Vh = _kv(V, H)
    O = torch.einsum("bhqk,bhkd->bqhd", P, Vh)
    u = UNIT[dtype]
    absacc = torch.einsum("bhqk,bhkd->bqhd", P, Vh.abs())
    # the floor: largest |V| among the keys the row can see (all of them for a fully masked row)
    full = ~keep.any(-1)                                          # (B, 1, Sq or 1)
    seen = keep | full[..., None]                                 # (B, 1, Sq or 1, Sk)
    if seen.shape[2] == 1:
        vmax = (Vh.abs() * seen[:, :, 0, :, None]).amax(2)[:, None]                                  # (B, 1, H, dk)
    else:
        vmax = torch.stack([(Vh[b].abs()[:, None] * seen[b].expand(H, -1, -1)[..., None]).amax(2).permute(1, 0, 2)
                            for b in range(Q.shape[0])])                                             # (B, Sq, H, dk)
    bound = u * O.abs() + 2 * u * absacc + FLOOR * vmax
    return dict(O=O, lse=mx + torch.log(l), max=mx, P=P, s=s, keep=keep, bound=bound, full=full)


def emulate_forward(Q, K, V, mask, scale, dtype=torch.bfloat16, mutate=None):
    """the same attention with P rounded to the operand type before the value product (the row sum adds the unrounded
    exponentials, as the kernels do) and the output rounded once.  `mutate(e, s, keep)` may return changed exponentials e
    (B, H, Sq, Sk): the wrong kernels of the mutation checks."""
    H = Q.shape[2]
    s, keep = scores(Q, K, mask, scale)
    e = torch.exp(s - s.max(-1, keepdim=True).values)
    if mutate is not None:
        e = mutate(e, s, keep)
    num = torch.einsum("bhqk,bhkd->bqhd", rnd(e, dtype), _kv(V, H))
    return rnd(num / e.sum(-1).permute(0, 2, 1)[..., None], dtype)


def backward(Qp, X, dCx, mask, scale, dtype=torch.bfloat16):
    """float64 backward of the shared form.  Qp, dCx (B, Sq, H, dk), X (B, Sk, dk), key mask (B, Sk) or None."""
    B, Sq, H, _ = Qp.shape
    f = forward(Qp, X[:, :, None], X[:, :, None], mask, scale, dtype)
    P, keep = f["P"], f["keep"]
    dP = torch.einsum("bqhd,bkd->bhqk", dCx, X)
    delta = (dCx * f["O"]).sum(-1).permute(0, 2, 1)                 # (B, H, Sq)
    dS = (P * (dP - delta[..., None]) * scale).masked_fill(~keep, 0.0)
    dQ = torch.einsum("bhqk,bkd->bqhd", dS, X)
    dX = torch.einsum("bhqk,bqhd->bkd", P, dCx) + torch.einsum("bhqk,bqhd->bkd", dS, Qp)
    u = UNIT[dtype]
    # floors.  fp32 accumulation: FLOOR times the largest term of the sum.  And dP - delta is a difference of two fp32 sums of
    # dk products no larger than max|dCx| max|X|, each carrying up to dk 2^-24 of that: where the difference cancels (a sharp
    # row: dP = delta at its key) what is left of dS is that absolute error, times P <= 1 and scale.
    dk = X.shape[-1]
    cancel = dk * 2.0 ** -24 * scale * dCx.abs().amax((1, 2, 3)) * X.abs().amax((1, 2))                    # (B)
    xmax = X.abs().amax(1)                                                                                # (B, dk)
    bound_dQ = (u * dQ.abs() + 2 * u * torch.einsum("bhqk,bkd->bqhd", dS.abs(), X.abs())
                + (FLOOR * dS.abs().amax(-1).permute(0, 2, 1)[..., None] + cancel[:, None, None, None]) * xmax[:, None, None, :])
    bound_dX = (2 * u * (torch.einsum("bhqk,bqhd->bkd", P, dCx.abs()) + torch.einsum("bhqk,bqhd->bkd", dS.abs(), Qp.abs()))
                + FLOOR * (P.amax((1, 2, 3))[:, None, None] * dCx.abs().amax((1, 2))[:, None, :]
                           + dS.abs().amax((1, 2, 3))[:, None, None] * Qp.abs().amax((1, 2))[:, None, :])
                + cancel[:, None, None] * torch.einsum("bhqk,bqhd->bkd", P, Qp.abs()))
    f.update(dP=dP, delta=delta, dS=dS, dQ=dQ, dX=dX, bound_dQ=bound_dQ, bound_dX=bound_dX)
    return f


def emulate_backward(Qp, X, dCx, mask, scale, dtype=torch.bfloat16, mutate_ds=None, delta_perm=None):
    """backward with P and dS rounded to the operand type before their products, dQp rounded once, dX float64.
    mutate_ds(dS, P, dP, delta, keep) / delta_perm (a permutation of the heads delta is read from): the mutation checks."""
    f = forward(Qp, X[:, :, None], X[:, :, None], mask, scale, dtype)
    P, keep = f["P"], f["keep"]
    dP = torch.einsum("bqhd,bkd->bhqk", dCx, X)
    delta = (dCx * f["O"]).sum(-1).permute(0, 2, 1)
    if delta_perm is not None:
        delta = delta[:, delta_perm]
    dS = (P * (dP - delta[..., None]) * scale).masked_fill(~keep, 0.0)
    if mutate_ds is not None:
        dS = mutate_ds(dS, P, dP, delta, keep)
    dSr, Pr = rnd(dS, dtype), rnd(P, dtype)
    dQ = rnd(torch.einsum("bhqk,bkd->bqhd", dSr, X), dtype)
    dX = torch.einsum("bhqk,bqhd->bkd", Pr, dCx) + torch.einsum("bhqk,bqhd->bkd", dSr, Qp)
    return dQ, dX


def lagged_statistics(s: torch.Tensor):
    """(row_max, row_sum) as fp32 tensors with P = exp(s - row_max) / row_sum: the exact maximum, lowered by 2.5 on every
    third row (the forward kernels may leave a lagging maximum); the sum is formed against the fp32-rounded maximum.
    Fully masked rows keep the exact fill value."""
    m = s.max(-1).values.clone()
    lag = torch.zeros_like(m)
    lag[..., ::3] = 2.5
    m = torch.where(m <= NEG_MASK, m, m - lag).float().double()
    l = torch.exp(s - m[..., None]).sum(-1)
    return m.float().contiguous(), l.float().contiguous()


def dropout_keep(p: float, seed: int, B: int, Sq: int, H: int, dk: int) -> torch.Tensor:
    """bool (B, Sq, H, dk): output dropout keeps the element.  The attention kernels number the elements
    (b * Sq + q) * H * dk + h * dk + d and call the GEMM epilogues' dropout_scale(p, seed, element): gemm_reference's."""
    return torch.from_numpy(gref.keep_mask(p, seed, B * Sq, H * dk, 1, 1, (0, 0, 0)).reshape(B, Sq, H, dk))


def within(out: torch.Tensor, ref: torch.Tensor, bound: torch.Tensor, frac: float = 1.0):
    """(ok, worst ratio |out - ref| / bound, its index)"""
    err = (out.double() - ref).abs()
    ratio = torch.where(err == 0, torch.zeros_like(err), err / bound)          # (an exact element passes a zero bound)
    ratio = torch.where(torch.isnan(ratio), torch.full_like(ratio, float("inf")), ratio)
    w = int(ratio.argmax())
    return bool(ratio.max() <= frac), float(ratio.max()), np.unravel_index(w, tuple(ratio.shape))


# --------------------------------------------------------------------------------------------------------------- inputs
@functools.lru_cache(maxsize=None)
def hadamard(n: int) -> torch.Tensor:
    h = torch.ones(1, 1, dtype=F64)
    while h.shape[0] < n:
        h = torch.cat([torch.cat([h, h], 1), torch.cat([h, -h], 1)], 0)
    return h


def signature(Sk: int, dk: int, shift: int, seed: int) -> torch.Tensor:
    """(Sk, dk) float64, exactly representable in bf16 and fp16: key k holds (-1)^k * mag(k) * pattern(k // 2), the patterns of
    the pairs of one block of dk pairs are rows of a Hadamard matrix (exactly orthogonal), blocks differ by a random sign
    vector.  Neighbouring keys cancel up to their magnitudes, so sum_k P V stays small beside sum_k P |V| on every row that
    spreads over many keys, and every key differs from every other in its pattern or its magnitude."""
    k = torch.arange(Sk)
    pair = k // 2 + shift
    mag = 1.0 + ((5 * pair + 3 * (k & 1)) % 8).double() / 32
    g = torch.Generator().manual_seed(1000 + seed)
    nblk = int(pair.max()) // dk + 1
    bs = torch.where(torch.rand(nblk, dk, generator=g) < 0.5, -1.0, 1.0).double()
    bs[0] = 1.0
    sgn = torch.where(k % 2 == 0, 1.0, -1.0).double()
    return (sgn * mag)[:, None] * hadamard(dk)[pair % dk] * bs[pair // dk]


SHARP = 32.0        # nats a sharp row's key lies above every other
ROW_KINDS = ("first", "last", "mid", "uniform", "stairs_small", "stairs_big")


def _targets(kind: str, valid: torch.Tensor, dk: int):
    """[(key, nats)]: the keys a query row of this kind is matched to"""
    idx = torch.nonzero(valid).flatten()
    if len(idx) == 0 or kind == "uniform":
        return []
    first, last = int(idx[0]), int(idx[-1])
    if kind == "first":
        return [(first, SHARP)]
    if kind == "last":
        return [(last, SHARP)]
    if kind == "mid":
        want = 31 if last > 31 else last // 2
        return [(int(idx[(idx - want).abs().argmin()]), SHARP)]
    # staircase: the last valid key of every 32-key tile of the last block of 2 dk keys (one block: exactly orthogonal keys)
    blk0 = (last // (2 * dk)) * 2 * dk
    reps = []
    for t0 in range(blk0, last + 1, 32):
        in_tile = idx[(idx >= t0) & (idx < t0 + 32)]
        if len(in_tile):
            reps.append(int(in_tile[-1]))
    # (keys of other blocks are only nearly orthogonal: fewer steps keep their cross-talk far below the top step)
    reps = reps[-8:] if last < 2 * dk else reps[-4:]
    if kind == "stairs_small":
        if len(idx) < 64:
            return []                     # too few keys for a spread row: uniform
        return [(k, 0.2 * (i + 1)) for i, k in enumerate(reps)]
    return [(k, 16.0 * (i + 1)) for i, k in enumerate(reps)]


def make_queries(Kh: torch.Tensor, keep: torch.Tensor, Sq: int, scale: float, seed: int, backward: bool = False):
    """Kh (B, H, Sk, dk) clean keys, keep (B, Sq or 1, Sk) -> Q (B, Sq, H, dk) float64: row (b, q, h) is of kind
    ROW_KINDS[(b + q + h) % 6]; uniform rows are zero, or small noise when at least 64 keys are valid.

    backward: also returns dCx (B, Sq, H, dk).  A gradient is a sum over few terms wherever few keys carry weight, and no
    bound of a few u of that sum can hold a correctly rounded result to half of itself there.  So the "last" and
    "stairs_big" rows, and every spread row of a batch row with fewer than 160 valid keys, become "pair" rows: matched to
    two orthogonal keys of magnitude 1 with equal weight, dCx a multiple of the first key's pattern.  Then P = 1/2 at both,
    dS = +-a dk scale / 4 and dQp = dS (X1 - X2) are exact in the operand type, and not trivial.  The other rows get i.i.d.
    normal dCx."""
    B, H, Sk, dk = Kh.shape
    g = torch.Generator().manual_seed(2000 + seed)
    Q = torch.zeros(B, Sq, H, dk, dtype=F64)
    noise = torch.randn(B, Sq, H, dk, generator=g, dtype=F64) * (0.3 / (scale * math.sqrt(dk) * 1.1))
    dCx = torch.randn(B, Sq, H, dk, generator=g, dtype=F64) if backward else None
    for b in range(B):
        cache = {}
        for q in range(Sq):
            valid = keep[b, q if keep.shape[1] > 1 else 0]
            vkey = q if keep.shape[1] > 1 else 0
            nvalid = int(valid.sum())
            for h in range(H):
                kind = ROW_KINDS[(b + q + h) % len(ROW_KINDS)]
                if backward and (kind in ("last", "stairs_big") or (kind in ("uniform", "stairs_small") and nvalid < 160)):
                    if (h, "pair") not in cache:      # valid keys of magnitude 1 in the first block of 2 dk keys, one per pair
                        ok = valid[:2 * dk] & (Kh[b, h, :2 * dk, 0].abs() == 1.0)
                        cache[(h, "pair")] = [int(k) for k in torch.nonzero(ok).flatten()]
                    cand = cache[(h, "pair")]
                    if len(cand) >= 2:
                        i1 = (3 * q + h) % len(cand)
                        k1, k2 = cand[i1], cand[(i1 + 1 + q % 3) % len(cand)]
                        if k1 // 2 == k2 // 2 or k1 == k2:
                            k2 = cand[(i1 + 2 + q % 3) % len(cand)]
                        if k1 // 2 != k2 // 2:
                            Q[b, q, h] = (Kh[b, h, k1] + Kh[b, h, k2]) * (SHARP / (scale * dk))
                            dCx[b, q, h] = Kh[b, h, k1] * (0.5, 1.0, 2.0)[q % 3]
                            continue
                    kind = "first"
                if (vkey, kind) not in cache:
                    cache[(vkey, kind)] = _targets(kind, valid, dk)
                tg = cache[(vkey, kind)]
                if not tg:
                    if kind == "uniform" and nvalid >= 64 and q % 2 == 1:
                        Q[b, q, h] = noise[b, q, h]
                    continue
                for key, nats in tg:
                    row = Kh[b, h, key]
                    Q[b, q, h] += row * (nats / (scale * float(row @ row)))
    return (Q, dCx) if backward else Q


GARBAGE = 1.0e4


def key_mask(name: str, B: int, Sk: int):
    """uint8 (B, Sk) or None"""
    if name == "none":
        return None
    m = torch.ones(B, Sk, dtype=torch.uint8)
    if name == "tail":
        m[0, Sk - max(1, Sk // 3):] = 0
    elif name == "first":
        m[:, 0] = 0
    elif name == "only0":
        m[0, 1:] = 0
    elif name == "onlylast":
        m[0, :Sk - 1] = 0
    elif name == "tile":            # a whole key tile (of every kernel: 32, 64 or 128 keys) masked between valid ones
        w = 128 if Sk > 256 else (64 if Sk > 128 else 32)
        m[:, w:2 * w] = 0
    elif name == "tile_b0":         # the same in batch row 0 only, behind it one more valid tile and a masked tail
        m[0, 32:64] = 0
        m[0, 97:] = 0
    elif name == "hole256":
        m[:, 250:min(262, Sk - 1)] = 0      # across the ballot word edge at key 256; the last key stays valid
    elif name == "fullrow":
        m[B - 1] = 0
        m[0, Sk - max(1, Sk // 4):] = 0
    elif name == "split":           # the pair form: key split 1 (keys 32 .. 63 of every 128) sees only masked tiles
        for k0 in range(32, Sk, 128):
            m[:, k0:k0 + 32] = 0
    else:
        raise ValueError(name)
    return m


def query_mask(name: str, B: int, Sq: int, Sk: int) -> torch.Tensor:
    """uint8 (B, Sq, Sk)"""
    if name == "causal":
        return torch.tril(torch.ones(Sq, Sk, dtype=torch.uint8)).repeat(B, 1, 1).contiguous()
    if name == "somerows":           # every fifth query row fully masked, the others see a window that moves with the row
        m = torch.ones(B, Sq, Sk, dtype=torch.uint8)
        for q in range(Sq):
            if q % 5 == 0:
                m[:, q] = 0
            else:
                m[:, q, (7 * q) % Sk:((7 * q) % Sk) + max(1, Sk // 5)] = 0
        return m
    raise ValueError(name)


QMASKS = ("causal", "somerows")


@functools.lru_cache(maxsize=None)
def make_inputs(form: str, B: int, H: int, Sq: int, Sk: int, mask_name: str, dtype=torch.bfloat16, backward: bool = False):
    """inputs of a case, float64 tensors holding values of `dtype`:
    form "split": Q (B, Sq, H, 256), K, V (B, Sk, H, 256); form "shared": Q = Qp (B, Sq, H, 128), X (B, Sk, 128).
    K / V / X carry +-GARBAGE at the masked keys of every batch row that is not fully masked (clean: the same with zeros
    there).  backward: also dCx (B, Sq, H, dk), see make_queries."""
    dk = 256 if form == "split" else 128
    scale = 1.0 / 16
    seed = (B * 131 + H * 17 + Sq * 7 + Sk) % 9973
    mask = query_mask(mask_name, B, Sq, Sk) if mask_name in QMASKS else key_mask(mask_name, B, Sk)
    keep = keep_of(mask, B, Sq, Sk)
    Hk = H if form == "split" else 1
    K = torch.stack([torch.stack([signature(Sk, dk, 3 * b + 11 * h + 64, seed) for h in range(Hk)], 1) for b in range(B)])
    if form == "split":
        V = torch.stack([torch.stack([signature(Sk, dk, 3 * b + 7 * h, seed + 1) for h in range(Hk)], 1) for b in range(B)])
    else:
        V = K
    Q = make_queries(_kv(K, H), keep, Sq, scale, seed, backward)
    Q, dCx = Q if backward else (Q, None)
    Q = rnd(Q, dtype)
    # masked keys: finite garbage where no query row of the batch row can see the key and the batch row is not fully masked
    unseen = ~keep.any(1) & keep.any(1).any(-1, keepdim=True)              # (B, Sk)
    g = torch.Generator().manual_seed(3000 + seed)
    junk = GARBAGE * torch.where(torch.rand(B, Sk, Hk, dk, generator=g) < 0.5, -1.0, 1.0).double()
    sel = unseen[:, :, None, None]
    out = dict(form=form, dk=dk, scale=scale, mask=mask, Q=Q, Kc=K, Vc=V,      # (Kc / Vc: the signature at every key)
               K=torch.where(sel, junk, K), V=torch.where(sel, -junk, V) if form == "split" else None,
               K0=torch.where(sel, torch.zeros_like(K), K), V0=torch.where(sel, torch.zeros_like(V), V) if form == "split" else None)
    if backward:
        out["dCx"] = rnd(dCx, dtype)
    return out


def kv_of(inp, clean: bool = True):
    """(K, V) as (B, Sk, Hk, dk); the shared form's X serves as both"""
    K = inp["K0"] if clean else inp["K"]
    if inp["form"] == "shared":
        return K, K
    return K, (inp["V0"] if clean else inp["V"])


@functools.lru_cache(maxsize=None)
def reference(form, B, H, Sq, Sk, mask_name, dtype=torch.bfloat16, backward_pass=False):
    """float64 reference of a case (computed once per process and shared; callers must not modify it)"""
    inp = make_inputs(form, B, H, Sq, Sk, mask_name, dtype, backward_pass)
    K, V = kv_of(inp)
    if backward_pass:
        return backward(inp["Q"], K[:, :, 0], inp["dCx"], inp["mask"], inp["scale"], dtype)
    return forward(inp["Q"], K, V, inp["mask"], inp["scale"], dtype)


# ---------------------------------------------------------------------------------------------------------------- tables
# (name, B, H, Sq, Sk, mask, dtype, pin, expected code, extras).  pin 0: the automatic choice (the fp16 entries have no pin).
BF, HF = torch.bfloat16, torch.float16


def _c(name, B, H, Sq, Sk, mask, pin, code, dtype=BF, **extra):
    return dict(name=name, B=B, H=H, Sq=Sq, Sk=Sk, mask=mask, pin=pin, code=code, dtype=dtype, **extra)


FWD256 = [
    # ---- code 22 (2 x 2: 64-row workgroups, 64-key tiles, two stages)
    _c("22-tiny", 1, 3, 1, 1, "none", 22, 22),
    _c("22-sk31", 1, 3, 31, 31, "first", 22, 22, packed=True),
    _c("22-sk33", 3, 1, 33, 33, "tail", 22, 22, mask_off=1),
    _c("22-sk63", 2, 4, 65, 63, "only0", 22, 22, mask_off=1),
    _c("22-sk65", 2, 4, 64, 65, "onlylast", 22, 22),
    _c("22-sk129", 4, 4, 130, 129, "tile_b0", 22, 22, mask_off=3),
    _c("22-sk257", 1, 3, 33, 257, "hole256", 22, 22),
    _c("22-sk255", 2, 2, 65, 255, "fullrow", 22, 22, drop=True),
    _c("22-sk1100", 1, 3, 65, 1100, "tile", 22, 22),
    _c("22-maxsk", 1, 1, 32, 10112, "tail", 22, 22),
    _c("22-causal", 3, 1, 65, 65, "causal", 22, 22, packed=True),
    _c("22-causal-tall", 2, 2, 130, 97, "causal", 22, 22),
    _c("22-somerows", 2, 2, 33, 129, "somerows", 22, 22),
    # ---- code 41 (4 x 1: 128-row workgroups, 32-key tiles, three stages, prefetch across the barrier)
    _c("41-tiny", 1, 3, 1, 1, "none", 41, 41),
    _c("41-sk32", 1, 3, 31, 32, "first", 41, 41),
    _c("41-sk33", 3, 1, 33, 33, "tail", 41, 41, mask_off=1),
    _c("41-sk64", 2, 4, 130, 64, "only0", 41, 41),
    _c("41-sk97", 2, 4, 257, 97, "onlylast", 41, 41, mask_off=1),
    _c("41-sk129", 4, 4, 130, 129, "tile_b0", 41, 41, mask_off=3),
    _c("41-sk256", 2, 2, 257, 256, "fullrow", 41, 41, drop=True),
    _c("41-sk257", 1, 3, 33, 257, "hole256", 41, 41),
    _c("41-sk1100", 1, 3, 130, 1100, "tile", 41, 41),
    _c("41-maxsk", 1, 1, 32, 10112, "tail", 41, 41),
    _c("41-causal", 3, 1, 65, 65, "causal", 41, 41, packed=True),
    _c("41-causal-tall", 2, 2, 130, 97, "causal", 41, 41),
    _c("41-somerows", 2, 2, 33, 129, "somerows", 41, 41),
    _c("41-auto", 50, 4, 1, 300, "none", 0, 41),                      # 200 workgroups: the automatic choice
    # ---- code 256 (two-phase, at most 256 keys): every tile count 1 .. 8
    _c("256-t1", 1, 3, 1, 1, "none", 256, 256),
    _c("256-t1b", 3, 1, 33, 31, "first", 256, 256, mask_off=1),
    _c("256-t2", 2, 4, 65, 33, "tail", 256, 256, mask_off=1),
    _c("256-t3", 2, 4, 257, 65, "only0", 256, 256, mask_off=1),
    _c("256-t4", 2, 4, 130, 97, "tile_b0", 256, 256, mask_off=3),
    _c("256-t5", 1, 3, 64, 129, "onlylast", 256, 256),
    _c("256-t6", 2, 2, 31, 192, "tile", 256, 256),
    _c("256-t7", 2, 2, 33, 200, "none", 256, 256),
    _c("256-t8", 2, 2, 257, 255, "fullrow", 256, 256, drop=True),
    _c("256-t8b", 1, 3, 256, 256, "hole256", 256, 256, packed=True),
    _c("256-auto", 50, 4, 1, 64, "none", 0, 256),
    # ---- fp16 operands (no pin, no two-phase kernel): one ragged, one masked and one multi-tile case per code
    _c("h22-ragged", 1, 3, 33, 65, "none", 0, 22, dtype=HF),
    _c("h22-masked", 3, 1, 65, 129, "tile_b0", 0, 22, dtype=HF, mask_off=1),
    _c("h22-tiles", 2, 2, 64, 257, "hole256", 0, 22, dtype=HF),
    _c("h41-ragged", 50, 4, 33, 65, "none", 0, 41, dtype=HF),
    _c("h41-masked", 67, 3, 31, 129, "tile_b0", 0, 41, dtype=HF, mask_off=1),
    _c("h41-tiles", 50, 4, 1, 257, "hole256", 0, 41, dtype=HF),
]

FWD128 = [
    # ---- code 22 (2 x 2, 64-key tiles, four stages)
    _c("22-tiny", 1, 3, 1, 1, "none", 22, 22),
    _c("22-sk31", 3, 1, 31, 31, "first", 22, 22, mask_off=1),
    _c("22-sk65", 2, 4, 65, 65, "tail", 22, 22, mask_off=1),
    _c("22-sk129", 8, 2, 130, 129, "tile_b0", 22, 22, mask_off=3),            # B = 8: workgroup map mode 0
    _c("22-sk257", 2, 4, 33, 257, "hole256", 22, 22),
    _c("22-sk255", 2, 2, 64, 255, "fullrow", 22, 22),
    _c("22-sk1100", 1, 3, 65, 1100, "tile", 22, 22),
    _c("22-maxsk", 1, 1, 32, 10112, "tail", 22, 22),
    _c("22-only0", 2, 2, 33, 97, "only0", 22, 22),
    _c("22-onlylast", 2, 2, 33, 97, "onlylast", 22, 22, mask_off=1),
    # ---- code 41 (4 x 1, 32-key tiles, four stages)
    _c("41-tiny", 1, 3, 1, 1, "none", 41, 41),
    _c("41-sk33", 3, 1, 33, 33, "first", 41, 41, mask_off=1),
    _c("41-sk63", 2, 4, 130, 63, "tail", 41, 41, mask_off=1),
    _c("41-sk97", 8, 2, 257, 97, "tile_b0", 41, 41, mask_off=3),
    _c("41-sk129", 2, 2, 65, 129, "onlylast", 41, 41, mask_off=1),
    _c("41-sk256", 2, 2, 64, 256, "fullrow", 41, 41),
    _c("41-sk257", 2, 4, 33, 257, "hole256", 41, 41),
    _c("41-sk1100", 1, 3, 130, 1100, "tile", 41, 41),
    _c("41-maxsk", 1, 1, 32, 10112, "tail", 41, 41),
    _c("41-only0", 2, 2, 33, 97, "only0", 41, 41),
    _c("41-auto", 16, 4, 768, 33, "tail", 0, 41, mask_off=1),
    # ---- code 24 (2 x 4: eight waves, 128-key tiles)
    _c("24-tiny", 1, 3, 1, 1, "none", 24, 24),
    _c("24-sk33", 3, 1, 33, 33, "first", 24, 24, mask_off=1),
    _c("24-sk129", 2, 4, 65, 129, "tail", 24, 24, mask_off=1),
    _c("24-sk257", 8, 2, 130, 257, "hole256", 24, 24),
    _c("24-sk300", 2, 2, 64, 300, "tile_b0", 24, 24),
    _c("24-sk255", 2, 2, 33, 255, "fullrow", 24, 24),
    _c("24-sk1100", 1, 3, 65, 1100, "tile", 24, 24),
    _c("24-sk2100", 1, 2, 33, 2100, "tile", 24, 24),
    _c("24-maxsk", 1, 1, 32, 10112, "tail", 24, 24),
    _c("24-only0", 2, 2, 33, 300, "only0", 24, 24),
    _c("24-onlylast", 2, 2, 33, 300, "onlylast", 24, 24),
    # ---- code 14 (pair form: two heads per wave, four key splits; even H only, bf16 only)
    _c("14-tiny", 1, 2, 1, 1, "none", 14, 14),
    _c("14-sk33", 3, 2, 33, 33, "first", 14, 14, mask_off=1),
    _c("14-sk96", 2, 4, 65, 96, "tail", 14, 14),
    _c("14-sk129", 8, 2, 130, 129, "tile_b0", 14, 14, mask_off=3),
    _c("14-sk257", 2, 4, 33, 257, "hole256", 14, 14),
    _c("14-split", 2, 2, 64, 300, "split", 14, 14),
    _c("14-sk255", 2, 2, 33, 255, "fullrow", 14, 14),
    _c("14-sk1100", 1, 2, 65, 1100, "tile", 14, 14),
    _c("14-maxsk", 1, 2, 32, 10112, "tail", 14, 14),
    _c("14-only0", 2, 2, 33, 300, "only0", 14, 14),
    _c("14-onlylast", 2, 2, 33, 300, "onlylast", 14, 14),
    # ---- fp16 operands (automatic choice only: 22 and 41)
    _c("h22-ragged", 1, 3, 33, 65, "none", 0, 22, dtype=HF),
    _c("h22-masked", 3, 2, 65, 129, "tile_b0", 0, 22, dtype=HF, mask_off=1),
    _c("h22-tiles", 2, 2, 64, 257, "hole256", 0, 22, dtype=HF),
    _c("h41-ragged", 16, 4, 768, 33, "none", 0, 41, dtype=HF),
    _c("h41-masked", 16, 4, 768, 65, "tile_b0", 0, 41, dtype=HF, mask_off=1),
    _c("h41-tiles", 16, 4, 768, 129, "none", 0, 41, dtype=HF),
]

# backward of the shared form: narrow (2 x 2) and wide (4 x 1, reached by shape: B * H * ceil(Sq / 32) >= 1536)
BWD128 = [
    _c("n-tiny", 1, 3, 1, 1, "none", 0, 22),
    _c("n-sk127", 2, 2, 31, 127, "tail", 0, 22, mask_off=1),
    _c("n-sk128", 8, 2, 33, 128, "first", 0, 22, lddx=136),
    _c("n-sk129", 3, 2, 97, 129, "fullrow", 0, 22, mask_off=1),
    _c("n-sk300", 2, 4, 130, 300, "hole256", 0, 22, lddx=136),
    _c("n-tile", 2, 2, 33, 300, "tile_b0", 0, 22),
    _c("n-nomask", 2, 2, 1, 129, "none", 0, 22),
    _c("w-sk33", 16, 4, 768, 33, "tail", 0, 41, mask_off=1),
    _c("w-sk129", 16, 4, 768, 129, "fullrow", 0, 41, lddx=136),
    _c("w-sk300", 192, 4, 33, 300, "hole256", 0, 41),                         # spread rows (300 keys) in the wide kernel
]


def case_id(c):
    return c["name"]
