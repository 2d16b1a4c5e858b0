"""Plain float64 restatement of bmhrl_gemm's contract (include/bmhrl_hip.h) and its per-element error bound.

Shared by tests/test_gemm_paths_gpu.py (which compares every main loop / epilogue path with it) and
tests/test_gemm_plan_cpu.py (which checks on the CPU that the bound is tight enough to catch one wrong product term).
Everything here is torch float64 or numpy integer arithmetic; it runs on whatever device its tensors live on.

Error bound of an fp32 result, element by element:

    |C - R| <= TAU * S[m, n],   S = |alpha| * (|A| |B|)[m, n]  (+ the magnitudes the epilogue adds, see linear_ref)

The operands are bf16, so every product a_mk * b_kn is exact in fp32 (8 + 8 significand bits) and R, the float64 sum, is
exact to 2^-53.  What the kernel adds is the rounding of its fp32 additions.  Each addition rounds with a relative
error of at most u = 2^-24 of the partial sum.  The partial sums are bounded by S, so the error is at most K * u * S
in the worst case (all roundings in one direction).  For the operands of these tests (independent, zero-mean) the
partial sums are about S / sqrt(K) and their roundings independent, so the error is far below u * S -- emulate_fp32_dot
below stays near 2^-27 S at K = 10 176 even with 16-term blocks rounded term by term.  TAU = 2^-17 leaves a wide margin
for that (and for a K split's partial sums) and is still far below one product term at the largest K: S / K is the mean
|a b|: a missing or doubled term of median size moves C by about 2^-14 S at K = 10 176 (normal operands), 8 times
TAU * S (test_gemm_plan_cpu checks exactly this).  The epilogue's own fp32 operations (alpha, bias, residual, dropout
scale, accumulate) each add at most u of their operands' magnitudes, which S includes, so TAU covers them too.

bf16 outputs additionally carry one rounding to bf16: BF16_U * |R| (round to nearest, 8 significand bits).
"""
from __future__ import annotations

import numpy as np
import torch

TAU = 2.0 ** -17
BF16_U = 2.0 ** -8
NEG_MASK = -1e9


# ---- dropout: csrc/common.h dropout_bits / dropout_scale, in numpy uint32 / uint64 arithmetic
def dropout_bits(seed: int, idx: np.ndarray) -> np.ndarray:
    idx = np.asarray(idx, dtype=np.uint64)
    seed = np.uint64(seed & 0xFFFFFFFFFFFFFFFF)
    with np.errstate(over="ignore"):
        x = (idx & np.uint64(0xFFFFFFFF)).astype(np.uint32) * np.uint32(0x9E3779B1) + np.uint32(int(seed) & 0xFFFFFFFF)
        hi = (idx >> np.uint64(32)).astype(np.uint32) + np.uint32(int(seed) >> 32)
        x ^= hi * np.uint32(0x85EBCA77)
        x ^= x >> np.uint32(16)
        x *= np.uint32(0x21F0AAAD)
        x ^= x >> np.uint32(15)
        x *= np.uint32(0x735A2D97)
        x ^= x >> np.uint32(15)
    return x


def dropout_threshold(p: float) -> int:
    # (uint32_t)fminf(p * 4294967296.f, 4294967040.f): p is a float32, the product by 2^32 is exact
    return int(min(float(np.float32(p)) * 4294967296.0, 4294967040.0))


def dropout_scale(p: float) -> float:
    return float(np.float32(1.0) / (np.float32(1.0) - np.float32(p)))


def drop_ids(M, N, batch1, batch2, drop_strides):
    """element ids [b1, b2, m, n] (uint64) of the header: b1*drop_sb1 + b2*drop_sb2 + m*drop_sm + n, all-zero strides ->
    (batch*M + m)*N + n"""
    sb1, sb2, sm = drop_strides
    if sb1 == 0 and sb2 == 0 and sm == 0:
        sm, sb2 = N, M * N
        sb1 = sb2 * batch2
    b1 = np.arange(batch1, dtype=np.uint64)[:, None, None, None]
    b2 = np.arange(batch2, dtype=np.uint64)[None, :, None, None]
    m = np.arange(M, dtype=np.uint64)[None, None, :, None]
    n = np.arange(N, dtype=np.uint64)[None, None, None, :]
    with np.errstate(over="ignore"):
        return b1 * np.uint64(sb1) + b2 * np.uint64(sb2) + m * np.uint64(sm) + n


def keep_mask(p, seed, M, N, batch1, batch2, drop_strides):
    """bool [batch1, batch2, M, N]: True where inverted dropout keeps the element"""
    bits = dropout_bits(seed, drop_ids(M, N, batch1, batch2, drop_strides))
    return bits >= np.uint32(dropout_threshold(p))


# ---- the four epilogues (float64).  acc, absacc: [b1, b2, M, N] = A B and |A| |B|.  Each returns (R, S): the reference
# value and the magnitude the error bound TAU * S scales with.
def linear_ref(acc, absacc, *, alpha=1.0, bias=None, relu=False, mask=None, keep=None, scale=1.0, residual=None, old=None):
    """v = alpha*acc (+bias[n]) ; mask==0 -> -1e9 ; relu ; dropout (keep, scale) ; (+residual) ; (+old C when accumulating)"""
    v = alpha * acc
    s = abs(alpha) * absacc
    if bias is not None:
        v = v + bias
        s = s + bias.abs()
    if mask is not None:
        # the -1e9 fill is exact in fp32; ReLU makes it an exact 0, otherwise later roundings are relative to 1e9
        v = torch.where(mask, v, torch.full_like(v, NEG_MASK))
        s = torch.where(mask, s, torch.full_like(s, 0.0 if relu else -NEG_MASK))
    if relu:
        v = torch.clamp_min(v, 0.0)
    if keep is not None:
        v = torch.where(keep, v * scale, torch.zeros_like(v))
        s = torch.where(keep, s * scale, torch.zeros_like(s))
    if residual is not None:
        v = v + residual
        s = s + residual.abs()
    if old is not None:
        v = v + old
        s = s + old.abs()
    return v, s


def prob_ref(acc, absacc, *, alpha, rowvec, rowvec2, mask=None):
    """p = exp(masked(alpha*acc) - rowvec[m]) / rowvec2[m].  The bound: an error e of the argument becomes a relative error
    e^e - 1 of p (about e), and __expf / the 1-ulp reciprocal / the fp32 argument add a few ulp relative to p, more for a
    large |x| or |rowvec| (their fp32 roundings enter the argument; __expf is exp2 of x*log2(e)) -- 16 ulp per unit of
    magnitude.  The second value returned is this bound RELATIVE to p (the caller multiplies)."""
    x = alpha * acc
    if mask is not None:
        x = torch.where(mask, x, torch.full_like(x, NEG_MASK))
    p = torch.exp(x - rowvec) / rowvec2
    e = TAU * abs(alpha) * absacc
    rel = torch.expm1(e) + 2.0 ** -20 * (1.0 + x.abs() + rowvec.abs())
    if mask is not None:
        rel = torch.where(mask, rel, torch.zeros_like(rel))      # exp(-1e9 - max) is an exact 0 on both sides
    return p, rel


def dscore_ref(acc, absacc, *, alpha, rowvec, aux, mask=None):
    """ds = aux * (acc - rowvec) * alpha, 0 where mask == 0"""
    v = aux * (acc - rowvec) * alpha
    s = aux.abs() * abs(alpha) * (absacc + rowvec.abs())
    if mask is not None:
        v = torch.where(mask, v, torch.zeros_like(v))
        s = torch.where(mask, s, torch.zeros_like(s))
    return v, s


def relu_bwd_ref(acc, absacc, *, alpha, aux):
    """dz = aux > 0 ? alpha*acc : 0"""
    pos = aux > 0
    return torch.where(pos, alpha * acc, torch.zeros_like(acc)), torch.where(pos, abs(alpha) * absacc, torch.zeros_like(acc))


def within(out, ref, bound):
    """bool tensor: |out - ref| <= bound, False for NaN / inf in out"""
    return (out - ref).abs() <= bound


# ---- emulation for the CPU self-check
def emulate_fp32_dot(a: np.ndarray, b: np.ndarray, chunk: int = 16) -> np.float32:
    """sum_k a_k b_k accumulated in fp32 the way an MFMA chain does it: exact products, each block of `chunk` of them summed
    and added to an fp32 accumulator (rounded after every addition)"""
    prod = a.astype(np.float64) * b.astype(np.float64)
    acc = np.float32(0.0)
    for i in range(0, len(prod), chunk):
        part = np.float32(0.0)
        for t in prod[i:i + chunk]:
            part = np.float32(part + np.float32(t))
        acc = np.float32(acc + part)
    return acc
