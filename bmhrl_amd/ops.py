"""Thin torch-tensor wrappers over the C ABI (include/bmhrl_hip.h).  Tensors only lend their device pointers;
every call is enqueued on torch's current HIP stream.  No wrapper has a CPU path.

Every call into the library goes through _launch (the entries of _lib.PROTOTYPES: a stream is appended) or _query (the
host-only entries of _lib.QUERIES), and every address comes from _ptr / _at: a CPU tensor, a tensor where a number
belongs or a wrong argument count is refused there, before the library is touched."""
from __future__ import annotations

import ctypes as C
import math
import os
from typing import Optional, Tuple

import numpy as np
import torch

from . import _lib

EPI_LINEAR, EPI_PROB, EPI_DSCORE, EPI_RELU_BWD = 0, 1, 2, 3


def pad8(n: int) -> int:
    return (n + 7) & ~7


def stream() -> int:
    """torch's current HIP stream on the current device as the handle the C ABI takes: the value of
    torch.cuda.current_stream().cuda_stream without building the Stream object (2.6 us against 0.3 per launch)"""
    return torch._C._cuda_getCurrentRawStream(torch.cuda.current_device())


_Tensor, _Parameter = torch.Tensor, torch.nn.Parameter
_TENSORS = frozenset((_Tensor, _Parameter))


def _ptr(t: Optional[torch.Tensor]):
    """the device address of t (None stays None): the one place a tensor lends its pointer, and it refuses CPU memory (an
    empty tensor has none: it lends the null pointer whatever its device)"""
    if t is None:
        return None
    if not t.is_cuda and t.data_ptr():
        raise RuntimeError("bmhrl_amd ops run on the GPU only (got a CPU tensor); there is no CPU fallback")
    return t.data_ptr()


def _at(t: Optional[torch.Tensor], off: int):
    """the device address of element `off` of t (None stays None)"""
    p = _ptr(t)
    return p + off * t.element_size() if off and p is not None else p


# name -> (arguments without the stream, their pointer slots) of the launching entries, from the tables of _lib
_LAUNCH = {name: (len(argtypes) - 1, _lib.PTR_SLOTS[name][:-1]) for name, argtypes in _lib.PROTOTYPES.items()}


def _launch(name: str, *args) -> None:
    """enqueue entry `name` of _lib.PROTOTYPES on the current stream: the tensors in its pointer slots become device addresses
    (None, ints and ctypes objects pass as they are), a tensor anywhere else is an error; raises _lib.HipError when the
    library refuses.  Every eager launch pays for this: only the pointer slots are walked in Python, exact types first,
    and what is left of the list gets one scan for a stray tensor (a Tensor or a Parameter; any other subclass at an
    integer's position is ctypes' own argument error)."""
    n, slots = _LAUNCH[name]
    if len(args) != n:
        raise TypeError(f"{name} takes {n} arguments and the stream, got {len(args)}")
    a = list(args)
    for i in slots:
        v = a[i]
        t = type(v)
        if t is _Tensor or t is _Parameter or (t is not int and v is not None and isinstance(v, _Tensor)):
            a[i] = _ptr(v)
    if not _TENSORS.isdisjoint(map(type, a)):
        i = next(i for i, v in enumerate(a) if isinstance(v, _Tensor))
        raise TypeError(f"{name}: argument {i} is a number, got a tensor")
    a.append(stream())          # (after the refusals: they need neither the stream nor the library)
    _lib.check(getattr(_lib.load(), name)(*a), name)


def _query(name: str, *args, refusal: bool = True):
    """the value of the host-only entry `name` of _lib.QUERIES (numbers and descriptors in, no stream, no tensor);
    refusal: a negative int is the library refusing the arguments (raises _lib.HipError), not a value"""
    restype, argtypes = _lib.QUERIES[name]
    if len(args) != len(argtypes):
        raise TypeError(f"{name} takes {len(argtypes)} arguments, got {len(args)}")
    for i, v in enumerate(args):
        if isinstance(v, _Tensor):
            raise TypeError(f"{name}: argument {i} is a number or a descriptor, got a tensor")
    r = getattr(_lib.load(), name)(*args)
    if refusal and restype is C.c_int and r < 0:
        _lib.check(r, name)
    return r


def attention_max_keys() -> int:
    """largest Sk of the fused attention kernels (bmhrl_attention_max_keys)"""
    return _query("bmhrl_attention_max_keys")


ATTN_PLAN_KINDS = {"256-fwd": 0, "128-fwd": 1, "128-bwd": 2}


def attention_plan(kind: str, B: int, H: int, Sq: int, Sk: int, mask_sq: int = 0) -> int:
    """the kernel code the entry `kind` would take for this shape under the current bmhrl_attention_config pin (pure host
    query: bmhrl_attention_plan); negative for a shape the entry refuses"""
    return int(_query("bmhrl_attention_plan", ATTN_PLAN_KINDS[kind], B, H, Sq, Sk, mask_sq, refusal=False))


def bf16_zeros(rows: int, cols: int, device) -> torch.Tensor:
    """bf16 (rows, pad8(cols)) buffer with zeroed padding columns (no fill when there is no padding)."""
    if cols % 8 == 0:
        return torch.empty(rows, cols, dtype=torch.bfloat16, device=device)
    return torch.zeros(rows, pad8(cols), dtype=torch.bfloat16, device=device)


def gemm_desc(A: torch.Tensor, B: torch.Tensor, M: int, N: int, K: int, *, lda: int, ldb: int, a_trans=False, b_trans=False,
              batch: Tuple[int, int] = (1, 1), a_strides=(0, 0), b_strides=(0, 0), a_off=0, b_off=0,
              C_f32: Optional[torch.Tensor] = None, ldc=0, c_strides=(0, 0), c_off=0,
              C_bf16: Optional[torch.Tensor] = None, ldcb=0, cb_strides=(0, 0), cb_off=0,
              epilogue=EPI_LINEAR, alpha=1.0, relu=False, accumulate=False, bias=None, residual=None, ldr=0,
              r_strides=(0, 0), mask=None, mask_sb1=0, mask_sm=0, rowvec=None, rowvec2=None, rv_strides=(0, 0),
              aux=None, ldaux=0, aux_strides=(0, 0), aux_off=0, dropout_p=0.0, seed=0, seed_dev=None, drop_strides=(0, 0, 0), allow_split_k=False,
              colsum: Optional[torch.Tensor] = None, colsum_off=0, colsum_sb2=0, bias_sb2=0, colsum_sb1=0, bias_sb1=0,
              split_ws: Optional[torch.Tensor] = None) -> "_lib.GemmDesc":
    """the bmhrl_gemm_desc of gemm(...) with the same arguments (defer aside); the tensors must outlive its use"""
    d = _lib.GemmDesc()
    d.M, d.N, d.K = M, N, K
    d.batch1, d.batch2 = batch
    d.A = _at(A, a_off); d.lda = lda; d.a_sb1, d.a_sb2 = a_strides; d.a_trans = int(a_trans)
    d.B = _at(B, b_off); d.ldb = ldb; d.b_sb1, d.b_sb2 = b_strides; d.b_trans = int(b_trans)
    d.C = _at(C_f32, c_off); d.ldc = ldc; d.c_sb1, d.c_sb2 = c_strides
    d.Cb = _at(C_bf16, cb_off); d.ldcb = ldcb; d.cb_sb1, d.cb_sb2 = cb_strides
    d.epilogue = epilogue; d.alpha = alpha; d.relu = int(relu); d.accumulate = int(accumulate)
    d.allow_split_k = int(allow_split_k)
    d.bias = _ptr(bias)
    d.residual = _ptr(residual); d.ldr = ldr; d.r_sb1, d.r_sb2 = r_strides
    d.mask = _ptr(mask); d.mask_sb1 = mask_sb1; d.mask_sm = mask_sm
    d.rowvec = _ptr(rowvec); d.rowvec2 = _ptr(rowvec2); d.rv_sb1, d.rv_sb2 = rv_strides
    d.aux = _at(aux, aux_off); d.ldaux = ldaux; d.aux_sb1, d.aux_sb2 = aux_strides
    d.dropout_p = dropout_p; d.seed = seed; d.seed_dev = _ptr(seed_dev)
    d.drop_sb1, d.drop_sb2, d.drop_sm = drop_strides
    d.colsum = _at(colsum, colsum_off); d.colsum_sb2 = colsum_sb2
    d.bias_sb2 = bias_sb2; d.bias_sb1 = bias_sb1; d.colsum_sb1 = colsum_sb1
    d.split_ws = _ptr(split_ws); d.split_ws_elems = 0 if split_ws is None else split_ws.numel()
    return d


_GEMM_OPERANDS = ("C_f32", "C_bf16", "bias", "residual", "mask", "rowvec", "rowvec2", "aux", "seed_dev", "colsum")


def gemm(A: torch.Tensor, B: torch.Tensor, M: int, N: int, K: int, *, defer: Optional[list] = None, **desc) -> None:
    """C[b] = epilogue(A[b] @ B[b]); **desc: the keywords of gemm_desc; offsets are in elements from the tensors' data pointers.
    split_ws: fp32 workspace of >= gemm_splits(M, N, K, batch) * batch * M * N elements: a K split then runs as partial tiles +
    an ordered second pass instead of fp32 atomics (reproducible; C needs no zeroing).
    defer: a list -- the problem is appended to it instead of launched; gemm_flush(list) then launches up to four of them as
    ONE kernel (bmhrl_gemm_group: leaf products nothing in between depends on)."""
    d = gemm_desc(A, B, M, N, K, **desc)
    if defer is not None and _GROUP_LEAVES:
        defer.append((d, (A, B, *map(desc.get, _GEMM_OPERANDS))))   # (operands kept alive)
        return
    _launch("bmhrl_gemm", C.byref(d))


GEMM_PLAN_FIELDS = ("loop", "tile", "stages", "splits", "split_form", "epi_path", "vec_ok", "ordered_colsum")


def gemm_plan(d: "_lib.GemmDesc") -> dict:
    """what bmhrl_gemm launches for descriptor d (bmhrl_gemm_plan: the launcher's own decision, host only) as a dict of
    GEMM_PLAN_FIELDS; raises for a descriptor bmhrl_gemm refuses"""
    plan = (_lib.i32 * 8)()
    _lib.check(_query("bmhrl_gemm_plan", C.byref(d), plan), "bmhrl_gemm_plan")
    return dict(zip(GEMM_PLAN_FIELDS, plan))


def gemm_f32_fast_path(d: "_lib.GemmDesc") -> bool:
    """True when the interior tiles of d's fp32 output leave through the specialised fp32 epilogue (bmhrl_gemm_f32_fast_path;
    gemm_plan reports such a launch as epi_path "generic"); raises for a descriptor bmhrl_gemm refuses"""
    return bool(_query("bmhrl_gemm_f32_fast_path", C.byref(d)))


def gemm_group_plan(descs) -> int:
    """gemm_group_kernel launches bmhrl_gemm_group makes for these descriptors (0: one by one); raises on a refused one"""
    return int(_query("bmhrl_gemm_group_plan", (_lib.GemmDesc * len(descs))(*descs), len(descs)))


_GROUP_LEAVES = os.environ.get("BMHRL_GEMM_GROUP", "1") == "1"      # (A/B switch: 0 launches deferred problems at once)


def gemm_flush(deferred: list) -> None:
    """launch the problems collected with gemm(..., defer=deferred): one kernel per up to four of them when they share a
    kernel variant, one by one otherwise (bmhrl_gemm_group decides)"""
    if not deferred:
        return
    _launch("bmhrl_gemm_group", (_lib.GemmDesc * len(deferred))(*[d for d, _ in deferred]), len(deferred))
    deferred.clear()


_SPLITS = {}


def gemm_splits(M: int, N: int, K: int, batch: int = 1) -> int:
    """K splits the launcher uses for a plain fp32 (M, N) output over a reduction of K with allow_split_k (bmhrl_gemm_splits)"""
    key = (M, N, K, batch)
    r = _SPLITS.get(key)
    if r is None:
        r = int(_query("bmhrl_gemm_splits", M, N, K, batch, refusal=False))
        if r < 1:
            raise RuntimeError(f"bmhrl_gemm_splits{key} failed: {r}")
        _SPLITS[key] = r
    return r


def gemm_overwrites(M: int, N: int, K: int, batch: int = 1) -> bool:
    """True when gemm(..., C_f32=..., allow_split_k=True) of this shape stores every element of C exactly once (no K
    split, no atomics): the output may then be uninitialised memory.  The launcher's own decision (bmhrl_gemm_splits)."""
    return gemm_splits(M, N, K, batch) == 1


def attention_fwd(Q, K, V, O, row_max, row_sum, mask, mask_sb, mask_sq, B, H, Sq, Sk, dk, scale, ldq, ldk, ldv, ldo,
                  q_off=0, k_off=0, v_off=0, dropout_p=0.0, seed=0, seed_dev=None):
    f16 = Q.dtype == torch.float16          # IEEE-half operands: the fp16 build of the same kernel
    if any((t.dtype == torch.float16) != f16 for t in (K, V, O)):
        raise RuntimeError("attention_fwd: Q, K, V and O must share one 16-bit type")
    _launch("bmhrl_attention_fwd_f16" if f16 else "bmhrl_attention_fwd", _at(Q, q_off), ldq, _at(K, k_off), ldk, _at(V, v_off),
            ldv, O, ldo, row_max, row_sum, mask, mask_sb, mask_sq, B, H, Sq, Sk, dk, scale, dropout_p, seed, seed_dev)


def small_attention_ok(Sq: int, Sk: int, dk: int) -> bool:
    """shapes bmhrl_small_attention_fwd / _bwd serve (pure host query)"""
    return bool(_query("bmhrl_small_attention_ok", Sq, Sk, dk))


def small_attention_fwd(Q, K, V, O, P, ldp, mask, mask_sb, mask_sq, B, H, Sq, Sk, dk, scale, ldq, ldk, ldv, ldo,
                        q_off=0, k_off=0, v_off=0, dropout_p=0.0, seed=0, seed_dev=None):
    """one launch: O (bf16 [B*Sq, ldo]) = dropout(softmax(scale Q K^T, masked) V), P (bf16 (B, H, Sq, ldp)) kept for backward"""
    _launch("bmhrl_small_attention_fwd", _at(Q, q_off), ldq, _at(K, k_off), ldk, _at(V, v_off), ldv, O, ldo, P, ldp, mask,
            mask_sb, mask_sq, B, H, Sq, Sk, dk, scale, dropout_p, seed, seed_dev)


def small_attention_bwd(dO, lddo, P, ldp, Q, K, V, dQ, dK, dV, mask, mask_sb, mask_sq, B, H, Sq, Sk, dk, scale, ldq, ldk, ldv,
                        lddq, lddk, lddv, q_off=0, k_off=0, v_off=0, dq_off=0, dk_off=0, dv_off=0, dbq=None, dbk=None, dbv=None,
                        dbq_off=0, dbk_off=0, dbv_off=0):
    """one launch: dQ / dK / dV (bf16, written into column slices) and optionally the bias gradients dbq / dbk / dbv
    (fp32 (H * dk) at the given element offsets, added to)"""
    _launch("bmhrl_small_attention_bwd", dO, lddo, P, ldp, _at(Q, q_off), ldq, _at(K, k_off), ldk, _at(V, v_off), ldv,
            _at(dQ, dq_off), lddq, _at(dK, dk_off), lddk, _at(dV, dv_off), lddv, _at(dbq, dbq_off), _at(dbk, dbk_off),
            _at(dbv, dbv_off), mask, mask_sb, mask_sq, B, H, Sq, Sk, dk, scale)


def memory_attention_ok(L: int, Sk: int, dm: int) -> bool:
    """shapes bmhrl_memory_attention serves (pure host query)"""
    return bool(_query("bmhrl_memory_attention_ok", L, Sk, dm))


def cast_memory(x, y, y_t, B, Sk, dm, ldt):
    """fp32 memory (B * Sk, dm) -> bf16 copy y (B * Sk, dm) and per-sample transposed copy y_t (B, dm, ldt), one launch"""
    _launch("bmhrl_cast_memory", x, y, y_t, B, Sk, dm, ldt)


def memory_attention(backward, X, x_off, ldx, mem, mem_t, ldt, PD, pd_row, pd_slot, Y, ldy, mask, mask_sb, n_mem, B2, H, L, Sk, dm,
                     scale):
    """few-query attention core over a memory, one launch (see bmhrl_memory_attention in include/bmhrl_hip.h)"""
    _launch("bmhrl_memory_attention", int(backward), _at(X, x_off), ldx, mem, Sk * dm, mem_t, dm * ldt, ldt, PD, pd_row, pd_slot,
            Y, ldy, mask, mask_sb, n_mem, B2, H, L, Sk, dm, scale)


def attention_shared128_fwd(Qp, X, ctx, row_max, row_sum, mask, mask_sb, B, H, Sq, Sk, scale, ldq, ldx, ldo):
    """absorbed-projection attention: Qp (B,Sq,H,128), X (B,Sk,128) shared by all heads -> ctx (B,Sq,H,128)"""
    f16 = Qp.dtype == torch.float16
    if any((t.dtype == torch.float16) != f16 for t in (X, ctx)):
        raise RuntimeError("attention_shared128_fwd: Qp, X and ctx must share one 16-bit type")
    _launch("bmhrl_attention_shared128_fwd_f16" if f16 else "bmhrl_attention_shared128_fwd", Qp, ldq, X, ldx, ctx, ldo, row_max,
            row_sum, mask, mask_sb, B, H, Sq, Sk, scale)


def attention_shared128_bwd(Qp, X, dCx, row_max, row_sum, delta, mask, mask_sb, dQp, dX, accumulate_dx, B, H, Sq, Sk, scale,
                            ldq, ldx, lddo, lddq, lddx=128):
    """fused backward of attention_shared128_fwd: dQp (bf16) and, when dX is given, dX (fp32 (B,Sk,128), += when
    accumulate_dx) -- P / dS are recomputed per tile and never written to HBM"""
    ws = None
    if dX is not None:
        ws = torch.empty(int(_query("bmhrl_attention_shared128_bwd_workspace", B, H, Sk)), device=Qp.device)
    _launch("bmhrl_attention_shared128_bwd", Qp, ldq, X, ldx, dCx, lddo, row_max, row_sum, delta, mask, mask_sb, dQp, lddq, dX,
            lddx, int(bool(accumulate_dx)), ws, B, H, Sq, Sk, scale)


def softmax_bwd_rows(P, ldp, dP, lddp, dS, ldds, rows, cols, scale, mask=None, mask_sb=0, mask_sq=0, rows_per_query=1, queries=1,
                     rows_per_group=0, group_stride=0, p_off=0, ds_off=0):
    """dS = scale * P * (dP - rowsum(P * dP)), 0 at masked keys; P bf16, dP fp32, dS bf16; rows = (sample, query, rows_per_query).
    rows_per_group > 0: P and dS rows in groups of that many, group g at g * group_stride elements (+ p_off / ds_off)"""
    _launch("bmhrl_softmax_bwd_rows", _at(P, p_off), ldp, dP, lddp, _at(dS, ds_off), ldds, rows, cols, scale, mask, mask_sb,
            mask_sq, rows_per_query, queries, rows_per_group, group_stride)


def softmax_rows(S, lds, P, ldp, rows, cols, rows_per_group=0, group_stride=0, p_off=0):
    _launch("bmhrl_softmax_rows", S, lds, _at(P, p_off), ldp, rows, cols, rows_per_group, group_stride)


def attn_delta(dO, lddo, O, ldo, delta, B, H, Sq, dk, scale=1.0):
    _launch("bmhrl_attn_delta", dO, lddo, O, ldo, delta, scale, B, H, Sq, dk)


def attention_bwd_scores256_ok(Sq, Sk, dk, msq):
    return bool(_query("bmhrl_attention_bwd_scores256_ok", Sq, Sk, dk, msq))


def attention_bwd_scores256(Q, ldq, K, ldk, V, ldv, dO, lddo, row_max, row_sum, mask, msb, P, dS, ldp, B, H, Sq, Sk, scale,
                            q_off=0, k_off=0, v_off=0):
    """P and dS (bf16 (B, H, Sq, ldp)) of a head-dimension-256 attention with at most 256 keys from the forward's statistics:
    one launch (csrc/attention_bwd256.hip); offsets in elements"""
    _launch("bmhrl_attention_bwd_scores256", _at(Q, q_off), ldq, _at(K, k_off), ldk, _at(V, v_off), ldv, dO, lddo, row_max,
            row_sum, mask, msb, P, dS, ldp, B, H, Sq, Sk, scale)


def layernorm_fwd(x, gamma, beta, y_bf16, ldy, y_f32, mean, rstd, rows, D):
    _launch("bmhrl_layernorm_fwd", x, gamma, beta, y_bf16, ldy, y_f32, mean, rstd, rows, D)


def layernorm_fwd_groups(x, gamma, beta, y_bf16, ldy, y_f32, mean, rstd, rows_per_group, D, groups):
    """`groups` LayerNorms of rows_per_group rows each, back to back, in one launch; gamma / beta are (groups, D)"""
    if gamma.numel() != groups * D or beta.numel() != groups * D:
        raise RuntimeError("layernorm_fwd_groups: gamma / beta must hold one row of D per group")
    _launch("bmhrl_layernorm_fwd_groups", x, gamma, beta, y_bf16, ldy, y_f32, mean, rstd, rows_per_group, D, groups)


def deterministic() -> bool:
    """BMHRL_DETERMINISTIC as the LIBRARY reads it (bmhrl_deterministic_enabled: one parse for both sides)"""
    global _DETERMINISTIC
    if _DETERMINISTIC is None:
        _DETERMINISTIC = bool(_query("bmhrl_deterministic_enabled"))
    return _DETERMINISTIC


_DETERMINISTIC = None


def layernorm_bwd_groups(dy, x, gamma, mean, rstd, dx, dx_add, dgamma, dbeta, rows_per_group, D, groups):
    """backward of layernorm_fwd_groups; dgamma / dbeta (groups, D) are ADDED to (zero them first)"""
    if deterministic():         # ordered parameter gradients: the two-stage form with a workspace per call, group by group
        R = rows_per_group
        for g in range(groups):
            sl = lambda t, n: None if t is None else t.reshape(-1)[g * n:(g + 1) * n]
            layernorm_bwd(sl(dy, R * D), sl(x, R * D), sl(gamma, D), sl(mean, R), sl(rstd, R), sl(dx, R * D), sl(dx_add, R * D),
                          sl(dgamma, D), sl(dbeta, D), R, D)
        return
    if gamma.numel() != groups * D or any(t is not None and t.numel() != groups * D for t in (dgamma, dbeta)):
        raise RuntimeError("layernorm_bwd_groups: gamma / dgamma / dbeta must hold one row of D per group")
    _launch("bmhrl_layernorm_bwd_groups", dy, x, gamma, mean, rstd, dx, dx_add, dgamma, dbeta, rows_per_group, D, groups)


def layernorm_bwd_workspace(rows, D) -> int:
    """fp32 elements of the scratch the two-stage column sums of layernorm_bwd go through (uninitialised is fine)."""
    return int(_query("bmhrl_layernorm_bwd_workspace", rows, D))


def layernorm_bwd(dy, x, gamma, mean, rstd, dx, dx_add, dgamma, dbeta, rows, D, workspace=None):
    if workspace is None:
        workspace = torch.empty(layernorm_bwd_workspace(rows, D), device=x.device)
    _launch("bmhrl_layernorm_bwd_ws", dy, x, gamma, mean, rstd, dx, dx_add, dgamma, dbeta, rows, D, workspace, workspace.numel())


def add_posenc(a, b, pe, out, out_bf16, ldob, B, S, D, dropout_p=0.0, seed=0, seed_dev=None):
    _launch("bmhrl_add_posenc", a, b, pe, out, out_bf16, ldob, B, S, D, dropout_p, seed, seed_dev)


def embed_posenc(tok, tok2, mix, table, pe, emb_out, out, B, L, D, scale, dropout_p=0.0, seed=0, seed_dev=None):
    _launch("bmhrl_embed_posenc", tok, tok2, mix, table, pe, emb_out, out, B, L, D, scale, dropout_p, seed, seed_dev)


def embed_bwd(tok, tok2, mix, dC, dtable, B, L, D, scale):
    _launch("bmhrl_embed_bwd", tok, tok2, mix, dC, dtable, B, L, D, scale)


def cast_bf16(x, ldx, y, ldy, rows, cols, scale=1.0, dropout_p=0.0, seed=0, y_off=0, seed_dev=None):
    _launch("bmhrl_cast_bf16", x, ldx, _at(y, y_off), ldy, rows, cols, scale, dropout_p, seed, seed_dev)


def cast_split3_bf16(x, ldx, y, ldy, part, lo_slot, rows, cols, y_off=0, x2=None, ldx2=0, cols2=0):
    """y blocks [hi | . | .] of width `part`: bf16(x) in block 0, bf16(x - hi) in block lo_slot, hi again in the other;
    x2 (rows, cols2): a second source whose columns follow x's inside every block"""
    _launch("bmhrl_cast_split3_bf16", x, ldx, _at(y, y_off), ldy, part, lo_slot, rows, cols, x2, ldx2, cols2)


def cast_colsum_bf16(x, ldx, y, ldy, rows, cols, colsum, scale=1.0, dropout_p=0.0, seed=0, seed_dev=None, colsum_off=0,
                     group_rows=None, colsum_stride=0):
    """y = bf16(x * scale * dropout); colsum[colsum_off + n] += column sums of y (colsum must start zeroed).
    group_rows: the rows form groups of that many, group g adds into colsum[colsum_off + g * colsum_stride + n]"""
    if group_rows is not None:
        _launch("bmhrl_cast_colsum_bf16_groups", x, ldx, y, ldy, rows, cols, scale, dropout_p, seed, seed_dev,
                _at(colsum, colsum_off), group_rows, colsum_stride)
        return
    _launch("bmhrl_cast_colsum_bf16", x, ldx, y, ldy, rows, cols, scale, dropout_p, seed, seed_dev, _at(colsum, colsum_off))


SEG_ELEMS_PER_BLOCK = 4096


def cast_segments(table: torch.Tensor, n_segments: int, n_blocks: int):
    """table: int64 (n_segments, 6) on the device -- see bmhrl_cast_segments in include/bmhrl_hip.h"""
    _launch("bmhrl_cast_segments", table, n_segments, n_blocks)


def colsum_bf16(dY, ld, db, accumulate, rows, cols, dy_off=0, db_off=0):
    _launch("bmhrl_colsum_bf16", _at(dY, dy_off), ld, _at(db, db_off), int(accumulate), rows, cols)


def colsum_bf16_groups(dY, ld, db, rows_per_group, cols, groups, db_stride):
    """db[g * db_stride + n] += sum over the rows of group g of dY[., n] (bf16 (groups * rows_per_group, ld)); one launch"""
    _launch("bmhrl_colsum_bf16_groups", dY, ld, db, rows_per_group, cols, groups, db_stride)


def cast_bf16_copies(x, ldx, y, ldy, rows, cols, copies, copy_stride):
    """y[c * copy_stride + r * ldy + n] = bf16(x[r * ldx + n]) for every copy c; one launch"""
    _launch("bmhrl_cast_bf16_copies", x, ldx, y, ldy, rows, cols, copies, copy_stride)


def gate_fwd(cv, ca, a_v, out, out_bf16, ldob, rows, D):
    _launch("bmhrl_gate_fwd", cv, ca, a_v, out, out_bf16, ldob, rows, D)


def gate_bwd(dout, cv, ca, a_v, dcv, dca, da_v, rows, D):
    _launch("bmhrl_gate_bwd", dout, cv, ca, a_v, dcv, dca, da_v, rows, D)


def _tail_groups(groups, grads=None):
    arr = (_lib.FusionTailParams * len(groups))()
    for i, (g, a) in enumerate(zip(groups, arr)):
        a.gamma_ca, a.beta_ca, a.gamma_cv, a.beta_cv, a.a_v = map(_ptr, g)
        if grads is not None:
            a.dgamma_ca, a.dbeta_ca, a.dgamma_cv, a.dbeta_cv, a.da_v = map(_ptr, grads[i])
    return arr


def fusion_tail_fwd(ca, cv, groups, rows_per_group, D, out, stats, out_bf16=None, ldob=0):
    """out = g * LN_CV(cv) + (1 - g) * LN_CA(ca); groups: list (1 or 2) of (gamma_ca, beta_ca, gamma_cv, beta_cv, a_v);
    out_bf16 (rows, ldob): the same values in bf16 as well"""
    arr = _tail_groups(groups)
    _launch("bmhrl_fusion_tail_fwd", ca, cv, C.cast(arr, C.c_void_p), len(groups), rows_per_group, D, out, stats, out_bf16, ldob)


def fusion_tail_bwd(dout, ca, cv, stats, groups, grads, rows_per_group, D, dca, dcv, dout1=None, ldd0=0, ldd1=0):
    """grads: per group (dgamma_ca, dbeta_ca, dgamma_cv, dbeta_cv, da_v), zeroed fp32 tensors or None.
    dout: gradient of group 0's rows (row stride ldd0, 0 = D); dout1: of group 1's (None: behind group 0's in dout)"""
    arr = _tail_groups(groups, grads)
    _launch("bmhrl_fusion_tail_bwd", dout, dout1, ldd0, ldd1, ca, cv, stats, C.cast(arr, C.c_void_p), len(groups), rows_per_group,
            D, dca, dcv)


def expand_goals_index(seg, src, B, L):
    _launch("bmhrl_expand_goals_index", seg, src, B, L)


def expand_goals(seg, x, src, out, out_bf16, ldob, B, L, D):
    """row map of Manager.expand_goals from the int32 labels `seg` (B, L) + the gather along it, one launch"""
    _launch("bmhrl_expand_goals", seg, x, src, out, out_bf16, ldob, B, L, D)


def expand_goals_explore(seg, x, src, out, out_bf16, ldob, B, L, D, mean_factor, std_factor, seed, seed_dev=None, noise_out=None):
    """expand_goals with the manager's exploration vector (reference :444-452) added in the same launch"""
    _launch("bmhrl_expand_goals_explore", seg, x, src, out, out_bf16, ldob, B, L, D, float(mean_factor), float(std_factor),
            int(seed), seed_dev, noise_out)


def gather_rows(x, src, out, out_bf16, ldob, rows, D):
    _launch("bmhrl_gather_rows", x, src, out, out_bf16, ldob, rows, D)


def scatter_add_rows(dout, src, dx, rows, D):
    _launch("bmhrl_scatter_add_rows", dout, src, dx, rows, D)


def log_softmax_(logits, ld, rows, V):
    _launch("bmhrl_log_softmax", logits, ld, rows, V)


def _amp_form(what, biased_trg, n_row, amp_given):
    """the C entry points read a biased call without n_row as "score IS the amplitude"; here that form has to be asked for by
    name, so that a caller who merely forgot n_row gets an error and not another loss"""
    if biased_trg is not None and (n_row is None) != bool(amp_given):
        raise ValueError(f"{what}: n_row is required with biased_trg unless amp_given=True (score is then the amplitude itself "
                         "and n_row must be None)")


def smooth_kl_fwd(logp, ld, trg, biased_trg, score, n_row, smoothing, pad_idx, zero_pad_rows, row_loss, amp_out, rows, V,
                  amp_given=False):
    _amp_form("smooth_kl_fwd", biased_trg, n_row, amp_given)
    _launch("bmhrl_smooth_kl_fwd", logp, ld, trg, biased_trg, score, n_row, smoothing, pad_idx, zero_pad_rows, row_loss, amp_out,
            rows, V)


def smooth_kl_full(logp, ld, trg, biased_trg, score, n_row, smoothing, pad_idx, zero_pad_rows, out, rows, V, amp_given=False):
    """the unreduced (rows, V) divergence of LabelSmoothing / BiasedKL (no gradient: the differentiable form is the row sums)"""
    _amp_form("smooth_kl_full", biased_trg, n_row, amp_given)
    _launch("bmhrl_smooth_kl_full", logp, ld, trg, biased_trg, score, n_row, smoothing, pad_idx, zero_pad_rows, out, rows, V)


def smooth_kl_bwd(logp, ld, trg, biased_trg, score, n_row, smoothing, pad_idx, zero_pad_rows, loss_scale, g_bf16, ldg,
                  g_f32, rows, V, wrt_logits=True, loss_scale2=None, amp_given=False):
    """loss_scale (and the optional loss_scale2, multiplied in) are one-element device tensors"""
    _amp_form("smooth_kl_bwd", biased_trg, n_row, amp_given)
    _launch("bmhrl_smooth_kl_bwd", logp, ld, trg, biased_trg, score, n_row, smoothing, pad_idx, zero_pad_rows, loss_scale,
            loss_scale2, int(wrt_logits), g_bf16, ldg, g_f32, rows, V)


def smooth_kl_amp_grad(logp, ld, trg, biased_trg, score, n_row, smoothing, pad_idx, zero_pad_rows, out, rows, V, amp_given=False):
    """d rows / d log(raw amplitude); amp_given (n_row None): `score` is the amplitude itself and the result is d rows / d amplitude"""
    _amp_form("smooth_kl_amp_grad", biased_trg, n_row, amp_given)
    _launch("bmhrl_smooth_kl_amp_grad", logp, ld, trg, biased_trg, score, n_row, smoothing, pad_idx, zero_pad_rows, out, rows, V)


def token_loss_reduce(row_loss, trg, rows, pad_idx, weight, factor, loss, scale):
    """loss = weight * sum(row_loss) / (#(trg != pad) * factor); scale = weight / (#tokens * factor) (device scalars)"""
    _launch("bmhrl_token_loss_reduce", row_loss, trg, rows, pad_idx, weight, factor, loss, scale)


def head_loss_ok(V, ld, ldg):
    return V % 4 == 0 and ld % 4 == 0 and ldg % 4 == 0 and 2 < V <= 12288


def head_loss(logits, ld, trg, smoothing, pad_idx, weight, factor, dloss, row_loss, loss_scale, g_bf16, ldg, counter, rows, V):
    """log-softmax in place + label-smoothing row sums + the loops' token-normalised loss (loss_scale = [loss, scale]) + bf16
    d logits for the incoming gradient `dloss` (device scalar or None = 1), one launch"""
    _launch("bmhrl_head_loss", logits, ld, trg, smoothing, pad_idx, weight, factor, dloss, row_loss, loss_scale, g_bf16, ldg,
            counter, rows, V)


def log_softmax_bwd(dlogp, logp, ld, g_bf16, ldg, rows, V):
    _launch("bmhrl_log_softmax_bwd", dlogp, logp, ld, g_bf16, ldg, rows, V)


def sample_tokens(logp, ld, out, p_out, rows, V, greedy, seed, seed_dev=None, row_offset=0):
    """one token per row, inverse-CDF sample for uniform01(seed + seed_dev[0], row + row_offset) or (greedy) the first maximum;
    p_out = exp(logp[token]).  The token is always in [0, V): a row in which no entry exceeds -inf (all NaN, all -inf) gives
    token 0 under greedy, and its p_out = exp(logp[row, 0]) still shows the NaN."""
    _launch("bmhrl_sample_tokens", logp, ld, out, p_out, rows, V, int(greedy), seed, seed_dev, row_offset)


def reinforce_fwd(pred, ld, action, value, critic_value, row_policy, row_value, rows, V, is_logp=True):
    _launch("bmhrl_reinforce_fwd", pred, ld, int(is_logp), action, value, critic_value, row_policy, row_value, rows, V)


def reinforce_bwd(probs, ld, action, value, critic_value, gscale, dprobs, dvalue, dcritic, rows, V):
    _launch("bmhrl_reinforce_bwd", probs, ld, action, value, critic_value, gscale, dprobs, dvalue, dcritic, rows, V)


def adam_step(param, grad, exp_avg, exp_avg_sq, n, lr, beta1, beta2, eps, weight_decay, step, grad_scale=1.0, step_dev=None,
              hyper=None):
    """hyper: the optimizer's hyper-parameter block (include/bmhrl_hip.h) -- the learning rate and the clip coefficient are
    read from it on the device (bmhrl_adam_step_dev) and `lr` is not used"""
    if hyper is not None:
        _launch("bmhrl_adam_step_dev", param, grad, exp_avg, exp_avg_sq, n, lr, beta1, beta2, eps, weight_decay, step, step_dev,
                grad_scale, hyper)
        return
    _launch("bmhrl_adam_step", param, grad, exp_avg, exp_avg_sq, n, lr, beta1, beta2, eps, weight_decay, step, step_dev, grad_scale)


def grad_norm(table, n_segments, n_blocks, grad, grad_scale, partials, hyper):
    """hyper[3] = L2 norm of the gradient the Adam table describes (x grad_scale), hyper[2] = the clip coefficient for the
    threshold in hyper[1] (bmhrl_grad_norm in include/bmhrl_hip.h); partials: fp32 workspace, one element per block"""
    _launch("bmhrl_grad_norm", table, n_segments, n_blocks, grad, grad_scale, partials, partials.numel(), hyper)


def accum_segments(table, n_segments, n_blocks, grad, accum, ctl, loss_in=None, loss_out=None):
    """accum = w * g (ctl[1] != 0: the first micro-batch of a window, a store) or fma(w, g, accum), w = ctl[0], over the
    gradient the Adam table describes (bmhrl_accum_segments in include/bmhrl_hip.h); ctl: two fp32 device words;
    loss_in / loss_out: optional fp32 device scalars, loss_out = (first ? 0 : loss_out) + w * loss_in in the same launch"""
    _launch("bmhrl_accum_segments", table, n_segments, n_blocks, grad, accum, ctl, loss_in, loss_out)


def gemm_f32(A, W, bias1, bias2, C, M, N, K):
    _launch("bmhrl_gemm_f32", A, A.stride(0), W, W.stride(0), bias1, bias2, C, C.stride(0), M, N, K)


def rnn_step(gates, xproj, whh, bhh, h_prev, c_prev, h_out, c_out, seq_out, ar_alpha, ar_beta, B, L, H, t):
    _launch("bmhrl_rnn_step", gates, xproj, whh, bhh, h_prev, c_prev, h_out, c_out, seq_out, ar_alpha, ar_beta, B, L, H, t)


def rnn_wavefront(layers, B, L, H, chunk=1):
    """layers: list of dicts with the fields of bmhrl_rnn_layer (tensors / None); runs the whole stack in
    L + chunk * (len(layers) - 1) launches"""
    arr = (_lib.RnnLayer * len(layers))()
    for d, a in zip(layers, arr):
        a.w_ih, a.w_hh, a.b_ih, a.b_hh = _ptr(d["w_ih"]), _ptr(d["w_hh"]), _ptr(d["b_ih"]), _ptr(d["b_hh"])
        a.in_seq, a.in_ld, a.in_dim, a.gates = _ptr(d["in_seq"]), d["in_ld"], d["in_dim"], d["gates"]
        a.seq_out = _ptr(d["seq_out"])
        a.h[0], a.h[1] = _ptr(d["h"][0]), _ptr(d["h"][1])
        a.c[0], a.c[1] = (_ptr(d["c"][0]), _ptr(d["c"][1])) if d.get("c") is not None else (None, None)
        a.arelu_alpha, a.arelu_beta = _ptr(d.get("arelu_alpha")), _ptr(d.get("arelu_beta"))
        a.xproj = _ptr(d.get("xproj"))
    _launch("bmhrl_rnn_wavefront", C.cast(arr, C.c_void_p), len(layers), B, L, H, chunk)


def critic_head(x, w, b, threshold, score, labels, rows, H):
    _launch("bmhrl_critic_head", x, w, b, threshold, score, labels, rows, H)


def rnn_step_train(gates, xproj, whh, bhh, h_seq, hprev_seq, c_seq, gate_seq, hn_seq, y_seq, ar_alpha, ar_beta, B, L, H, t):
    """one training-forward time step of one layer (bmhrl_rnn_step_train): rnn_step that keeps what the backward needs"""
    _launch("bmhrl_rnn_step_train", gates, xproj, whh, bhh, h_seq, hprev_seq, c_seq, gate_seq, hn_seq, y_seq, ar_alpha, ar_beta,
            B, L, H, t)


def rnn_bwd_step(gates, whh, dy, h_seq, c_seq, gate_seq, hn_seq, carry, dax, dah, ar_alpha, ar_beta, B, L, H, t):
    """backward of one cell, t descending (bmhrl_rnn_bwd_step); the LSTM passes dah=None"""
    _launch("bmhrl_rnn_bwd_step", gates, whh, dy, h_seq, c_seq, gate_seq, hn_seq, carry, dax, dah, ar_alpha, ar_beta, B, L, H, t)


def gemm_f32_nn(A, Bm, C, M, N, K, a_kmajor=False):
    """C[M,N] = op(A) . B, B (K, N) row-major; A (M, K) row-major or, a_kmajor, (K, M) row-major (bmhrl_gemm_f32_nn)"""
    _launch("bmhrl_gemm_f32_nn", A, 0 if A is None else A.stride(0), int(a_kmajor), Bm, 0 if Bm is None else Bm.stride(0), C,
            0 if C is None else C.stride(0), M, N, K)


def rnn_bias_grad(dax, dah, db_x, db_h, rows, N):
    _launch("bmhrl_rnn_bias_grad", dax, dah, db_x, db_h, rows, N)


def arelu_grad(dy, h, alpha, beta, dalpha, dbeta, n):
    """ordered AReLU parameter gradients over n elements (bmhrl_arelu_grad)"""
    partial = None if dy is None else torch.empty(128, device=dy.device)
    _launch("bmhrl_arelu_grad", dy, h, alpha, beta, partial, dalpha, dbeta, n)


def critic_head_loss(y2, lin_w, lin_b, labels, mask, pos_weight, ds_in, score, loss, ds, dy2, dlin_w, dlin_b, rows, H):
    """head (+ masked BCE-with-logits when labels is given) and its backward in one launch (bmhrl_critic_head_loss);
    mask: bool / uint8, one byte per row"""
    _launch("bmhrl_critic_head_loss", y2, lin_w, lin_b, labels, mask, float(pos_weight), ds_in, score, loss, ds, dy2, dlin_w,
            dlin_b, rows, H)


def adam_segments(table, n_segments, n_blocks, param, grad, exp_avg, exp_avg_sq, lr, beta1, beta2, eps, weight_decay, step,
                  grad_scale=1.0, step_dev=None, hyper=None):
    """Adam over the flat bucket through a per-parameter table that also names each weight's bf16 shadow (see
    bmhrl_adam_segments in include/bmhrl_hip.h); hyper: as adam_step (bmhrl_adam_segments_dev)"""
    if hyper is not None:
        _launch("bmhrl_adam_segments_dev", table, n_segments, n_blocks, param, grad, exp_avg, exp_avg_sq, lr, beta1, beta2, eps,
                weight_decay, step, step_dev, grad_scale, hyper)
        return
    _launch("bmhrl_adam_segments", table, n_segments, n_blocks, param, grad, exp_avg, exp_avg_sq, lr, beta1, beta2, eps,
            weight_decay, step, step_dev, grad_scale)


def make_masks(rgb, audio, trg, pad_idx, copies=1):
    """V_mask (copies*B, 1, Tv), A_mask (copies*B, 1, Ta), C_mask (copies*B, L, L) as bool tensors, one launch
    (model/masking.py:18-55, bimodal case; copies > 1: the same masks laid out that many times)"""
    B, Tv = rgb.shape[:2]
    Ta, L = audio.shape[1], trg.shape[1]
    if rgb.stride(2) != 1 or rgb.stride(0) != Tv * rgb.stride(1) or audio.stride(2) != 1 or audio.stride(0) != Ta * audio.stride(1):
        raise RuntimeError("make_masks: feature stacks must be (B, T, D) with contiguous rows")
    trg = trg.contiguous()
    vm = torch.empty(copies * B, 1, Tv, dtype=torch.bool, device=rgb.device)
    am = torch.empty(copies * B, 1, Ta, dtype=torch.bool, device=rgb.device)
    cm = torch.empty(copies * B, L, L, dtype=torch.bool, device=rgb.device)
    _launch("bmhrl_make_masks", rgb, rgb.stride(1), audio, audio.stride(1), trg, B, Tv, Ta, L, pad_idx, copies, vm, am, cm)
    return vm, am, cm


def batch_head(rgb, audio, captions, pad_idx, copies=1, bump64=None, bump32=()):
    """Head of a training step, one launch: captions (B, L + 1) -> (trg_in, trg_y) = (captions[:, :-1], captions[:, 1:])
    as contiguous tensors, make_masks() of trg_in, and `bump64` (int64 device word: the seed) / up to two int32 device
    counters in `bump32` (Adam steps) advanced by one.  Returns (vm, am, cm, trg_in, trg_y)."""
    B, Tv = rgb.shape[:2]
    Ta, L = audio.shape[1], captions.shape[1] - 1
    if rgb.stride(2) != 1 or rgb.stride(0) != Tv * rgb.stride(1) or audio.stride(2) != 1 or audio.stride(0) != Ta * audio.stride(1):
        raise RuntimeError("batch_head: feature stacks must be (B, T, D) with contiguous rows")
    if captions.dtype != torch.int64 or captions.stride(1) != 1 or L < 1:
        raise RuntimeError("batch_head: captions must be (B, L + 1) int64 with contiguous rows")
    if len(bump32) > 2 or any(t.dtype != torch.int32 for t in bump32) or (bump64 is not None and bump64.dtype != torch.int64):
        raise RuntimeError("batch_head: counters are one int64 word and at most two int32 words")
    dev = rgb.device
    vm = torch.empty(copies * B, 1, Tv, dtype=torch.bool, device=dev)
    am = torch.empty(copies * B, 1, Ta, dtype=torch.bool, device=dev)
    cm = torch.empty(copies * B, L, L, dtype=torch.bool, device=dev)
    trg_in = torch.empty(B, L, dtype=torch.int64, device=dev)
    trg_y = torch.empty(B, L, dtype=torch.int64, device=dev)
    b32 = list(bump32) + [None, None]
    _launch("bmhrl_batch_head", rgb, rgb.stride(1), audio, audio.stride(1), captions, captions.stride(0), B, Tv, Ta, L, pad_idx,
            copies, vm, am, cm, trg_in, trg_y, bump64, b32[0], b32[1])
    return vm, am, cm, trg_in, trg_y


# ---- Conv1d('same') + GroupNorm input projection of the DETR-mode agent (csrc/conv_gn.hip)
def unfold1d_bf16(x, out, ldo, B, T, C, k, left):
    """out[(b, t)][j * C + c] = x[b][t + j - left][c] (0 outside the clip), bf16: the operand of a Conv1d as a GEMM"""
    _launch("bmhrl_unfold1d_bf16", x, out, ldo, B, T, C, k, left)


def fold1d(du, ldu, dx, B, T, C, k, left):
    """dx[b][t][c] = sum_j du[(b, t - j + left)][j * C + c]: the data gradient of the unfolded operand"""
    _launch("bmhrl_fold1d", du, ldu, dx, B, T, C, k, left)


def groupnorm_fwd(x, gamma, beta, y, mean, rstd, B, T, C, G, eps):
    _launch("bmhrl_groupnorm_fwd", x, gamma, beta, y, mean, rstd, B, T, C, G, float(eps))


def groupnorm_bwd(dy, x, gamma, mean, rstd, dx, dgamma, dbeta, B, T, C, G):
    _launch("bmhrl_groupnorm_bwd", dy, x, gamma, mean, rstd, dx, dgamma, dbeta, B, T, C, G)


# ---- beam-search decoding (csrc/beam.hip)
BEAM_MAX = 16                       # largest beam of bmhrl_beam_select
BEAM_REORDER_CHUNK = 256 * 16 * 4   # bytes of one (buffer, row) a reorder workgroup moves


def _check_select_buffers(fn, need, K, G, V, ld, logp, scores, scores_out, finished, finished_out, parent, tok, hist, t,
                          last_live, R):
    """the conditions beam_select (G = 1) and group_beam_select share; need: how fn's message words K' = K / G <= V"""
    if not (1 <= K <= BEAM_MAX and G >= 1 and K % G == 0 and K // G <= V and ld >= V and logp.dtype == torch.float32
            and logp.numel() >= (R - 1) * ld + V):
        raise ValueError(f"{fn}: need 1 <= K <= 16, {need} and fp32 logp rows (B*K, ld >= V)")
    for x, dt in ((scores, torch.float32), (scores_out, torch.float32), (finished, torch.uint8), (finished_out, torch.uint8),
                  (parent, torch.int32), (tok, torch.int64)):
        if x.dtype != dt or x.numel() < R or not x.is_contiguous():
            raise ValueError(f"{fn}: expected a contiguous {dt} buffer of {R} elements")
    if hist.dtype != torch.int64 or hist.dim() != 2 or hist.shape[0] != R or hist.stride(1) != 1:
        raise ValueError(f"{fn}: hist must be (B*K, cols) int64 with contiguous rows")
    if t.dtype != torch.int64 or last_live.dtype != torch.int32:
        raise ValueError(f"{fn}: t is an int64 word, last_live an int32 word")


def beam_select(logp, ld, scores, finished, parent, tok, hist, t, last_live, B, K, V, end_idx, pad_idx,
                scores_out=None, finished_out=None):
    """per sample, the K best candidates of rule 3 (see bmhrl_beam_select in include/bmhrl_hip.h): scores (B*K) fp32 and
    finished (B*K) uint8 are updated in place unless *_out are given; parent (B*K) int32, tok (B*K) int64,
    hist (B*K, cols) int64 column t + 1, last_live (1,) int32 = t + 1 when a beam is still live.  t: (1,) int64 device word."""
    scores_out = scores if scores_out is None else scores_out
    finished_out = finished if finished_out is None else finished_out
    _check_select_buffers("beam_select", "K <= V", K, 1, V, ld, logp, scores, scores_out, finished, finished_out, parent, tok,
                          hist, t, last_live, B * K)
    _launch("bmhrl_beam_select", logp, ld, scores, finished, scores_out, finished_out, parent, tok, hist, hist.stride(0),
            hist.shape[1], t, last_live, B, K, V, end_idx, pad_idx)


def group_beam_select(logp, ld, scores, finished, parent, tok, hist, t, last_live, B, K, V, end_idx, pad_idx, G,
                      diversity_penalty, scores_out=None, finished_out=None):
    """beam_select for diverse beam search (the grouped instantiation of csrc/beam.hip's select kernel; rules G2-G4 of
    decode.py, see bmhrl_group_beam_select in include/bmhrl_hip.h): the K beams of a sample form G groups of K / G that choose
    one after another, a later group paying diversity_penalty per earlier beam that chose the token.  Buffers and outputs as
    beam_select's."""
    scores_out = scores if scores_out is None else scores_out
    finished_out = finished if finished_out is None else finished_out
    lam = float(diversity_penalty)
    _check_select_buffers("group_beam_select", "G >= 1 dividing K, K / G <= V", K, G, V, ld, logp, scores, scores_out, finished,
                          finished_out, parent, tok, hist, t, last_live, B * K)
    if not (lam >= 0 and lam < float("inf")):
        raise ValueError(f"group_beam_select: diversity_penalty must be finite and >= 0, got {diversity_penalty}")
    _launch("bmhrl_group_beam_select", logp, ld, scores, finished, scores_out, finished_out, parent, tok, hist, hist.stride(0),
            hist.shape[1], t, last_live, B, K, V, end_idx, pad_idx, G, lam)


def beam_reorder_table(buffers, rows, device):
    """[(state, scratch, pos_bytes)] -> (device table of bmhrl_beam_buffer entries, n_blocks) for beam_reorder.  state and
    scratch: contiguous tensors of the same shape whose first axis is the beam row; pos_bytes: bytes of one position of a
    row (0: no position axis, the whole row moves)."""
    words = []
    n_blocks = 0
    for state, scratch, pos_bytes in buffers:
        if (state.shape != scratch.shape or state.dtype != scratch.dtype or not state.is_contiguous() or not scratch.is_contiguous()
                or state.shape[0] != rows):
            raise ValueError("beam_reorder_table: state and scratch must be contiguous, alike and have one row per beam")
        beam_bytes = state.numel() // rows * state.element_size()
        if pos_bytes < 0 or pos_bytes > beam_bytes:
            raise ValueError("beam_reorder_table: pos_bytes out of range")
        words += [_ptr(state), _ptr(scratch), beam_bytes, pos_bytes]
        n_blocks += rows * (-(-beam_bytes // BEAM_REORDER_CHUNK))
    table = torch.tensor(words, dtype=torch.int64).to(device)
    return table, n_blocks


def beam_reorder(table, n_buffers, n_blocks, parent, rows, K, t, phase):
    """phase 0: scratch[j] = rows [0, t] of state[parent row of j]; phase 1: state[j] = scratch[j] (rows j whose parent is
    themselves are skipped in both); see bmhrl_beam_reorder in include/bmhrl_hip.h"""
    if table.dtype != torch.int64 or table.numel() != 4 * n_buffers or parent.dtype != torch.int32 or parent.numel() < rows:
        raise ValueError("beam_reorder: table of n_buffers x 4 int64 words and an int32 parent per row expected")
    _launch("bmhrl_beam_reorder", table, n_buffers, n_blocks, parent, rows, K, t, phase)


# ---- per-prefix caption rewards (csrc/rewards.hip)
REWARD_CIDER, REWARD_BLEU = 0, 1
REWARDS_MAX_L, REWARDS_MAX_R = 256, 512      # BMHRL_REWARDS_MAX_L / _R of include/bmhrl_hip.h


def rewards(hyp, vmap, eos, ref, ref_len, df_keys, df_logs, metric, n, sigma, scores, delta):
    """per-prefix scores (B, L) fp64 and their first differences (B, L) fp32 of the sampled captions hyp (B, L) int64 against
    ref (>= B, R) int32 word ids, ref_len (>= B) int32; see bmhrl_rewards in include/bmhrl_hip.h.  df_keys (cap, 4) int32 /
    df_logs (cap) fp64: the CIDEr document-frequency table (None for BLEU)."""
    B, L = hyp.shape
    R = ref.shape[1]
    if hyp.dtype != torch.int64 or vmap.dtype != torch.int32 or ref.dtype != torch.int32 or ref_len.dtype != torch.int32:
        raise ValueError("rewards: hyp int64, vmap / ref / ref_len int32 expected")
    if hyp.stride(1) != 1 or ref.stride(1) != 1 or not vmap.is_contiguous() or not ref_len.is_contiguous():
        raise ValueError("rewards: hyp and ref need contiguous rows, vmap and ref_len contiguous")
    if ref.shape[0] < B or ref_len.numel() < B:
        raise ValueError("rewards: fewer reference rows than samples")
    if scores.dtype != torch.float64 or delta.dtype != torch.float32 or tuple(scores.shape) != (B, L) or \
            tuple(delta.shape) != (B, L) or scores.stride(1) != 1 or delta.stride(1) != 1:
        raise ValueError("rewards: scores (B, L) fp64 and delta (B, L) fp32 with contiguous rows expected")
    cap = 0
    if df_keys is not None:
        cap = df_keys.shape[0]
        if df_keys.dtype != torch.int32 or tuple(df_keys.shape) != (cap, 4) or not df_keys.is_contiguous() or \
                df_logs.dtype != torch.float64 or df_logs.numel() != cap:
            raise ValueError("rewards: df_keys (cap, 4) int32 and df_logs (cap) fp64 expected")
    _launch("bmhrl_rewards", hyp, hyp.stride(0), vmap, vmap.numel(), eos, ref, ref.stride(0), ref_len, df_keys, df_logs, cap,
            metric, n, float(sigma), B, L, R, scores, scores.stride(0), delta, delta.stride(0))


# ---- per-prefix METEOR rewards (csrc/meteor.hip)
def meteor(hyp, vmap, vstem, syn_off, syn_ids, ref, ref_stem, ref_len, alpha, beta, gamma, scores, delta):
    """per-prefix METEOR scores (B, L) fp64 and the first differences of their fp32 values (B, L) fp32 of the sampled
    captions hyp (B, L) int64 against ref (>= B, R) int32 word ids, ref_len (>= B) int32; see bmhrl_meteor in
    include/bmhrl_hip.h.  vstem (V) int32 with ref_stem shaped and strided like ref (both None: no stem stage); syn_off
    (V + 1) int32 and syn_ids int32, at least one element (both None: no synonym stage)."""
    B, L = hyp.shape
    R = ref.shape[1]
    V = vmap.numel()
    if hyp.dtype != torch.int64 or vmap.dtype != torch.int32 or ref.dtype != torch.int32 or ref_len.dtype != torch.int32:
        raise ValueError("meteor: hyp int64, vmap / ref / ref_len int32 expected")
    if hyp.stride(1) != 1 or ref.stride(1) != 1 or not vmap.is_contiguous() or not ref_len.is_contiguous():
        raise ValueError("meteor: hyp and ref need contiguous rows, vmap and ref_len contiguous")
    if ref.shape[0] < B or ref_len.numel() < B:
        raise ValueError("meteor: fewer reference rows than samples")
    if (vstem is None) != (ref_stem is None):
        raise ValueError("meteor: vstem and ref_stem go together")
    if vstem is not None:
        if vstem.dtype != torch.int32 or vstem.numel() != V or not vstem.is_contiguous():
            raise ValueError("meteor: vstem (V) int32 expected")
        if ref_stem.dtype != torch.int32 or ref_stem.shape != ref.shape or ref_stem.stride() != ref.stride():
            raise ValueError("meteor: ref_stem int32, shaped and strided like ref, expected")
    n_syn = 0
    if syn_off is not None and syn_ids is not None:
        n_syn = syn_ids.numel()
        if syn_off.dtype != torch.int32 or syn_ids.dtype != torch.int32 or syn_off.numel() != V + 1 or n_syn < 1 or \
                not syn_off.is_contiguous() or not syn_ids.is_contiguous():
            raise ValueError("meteor: syn_off (V + 1) int32 and syn_ids (>= 1) int32 expected")
    if scores.dtype != torch.float64 or delta.dtype != torch.float32 or tuple(scores.shape) != (B, L) or \
            tuple(delta.shape) != (B, L) or scores.stride(1) != 1 or delta.stride(1) != 1:
        raise ValueError("meteor: scores (B, L) fp64 and delta (B, L) fp32 with contiguous rows expected")
    _launch("bmhrl_meteor", hyp, hyp.stride(0), vmap, vstem, V, syn_off, syn_ids, n_syn, ref, ref_stem, ref.stride(0), ref_len,
            float(alpha), float(beta), float(gamma), B, L, R, scores, scores.stride(0), delta, delta.stride(0))


# ---- evaluation forms of the caption metrics (csrc/caption_eval.hip)
CAPTION_EVAL_PAIR_INTS, CAPTION_EVAL_GROUP_SCORES = 10, 6      # BMHRL_CAPTION_EVAL_* of include/bmhrl_hip.h


def caption_eval(hyp, hyp_len, ref, ref_len, group_off):
    """BLEU counts, LCS length and CIDEr of P (hypothesis, reference) pairs and Bleu_1..4 / mean ROUGE_L / mean CIDEr of
    the G groups of contiguous pairs group_off (G + 1) int32 delimits; see bmhrl_caption_eval in include/bmhrl_hip.h.
    hyp (P, L) / ref (P, R) int32 word ids with contiguous rows, hyp_len / ref_len (P) int32.  Returns pair_ints (P, 10)
    int32, pair_lcs (P) int32, pair_cider (P) fp64, group_scores (G, 6) fp64.  Synchronises the stream once (the offsets
    are checked on the host); not for captured graphs."""
    for t in (hyp, hyp_len, ref, ref_len, group_off):
        if t.dtype != torch.int32:
            raise ValueError("caption_eval: int32 tensors expected")
    if hyp.dim() != 2 or ref.dim() != 2 or hyp.stride(1) != 1 or ref.stride(1) != 1 or ref.shape[0] != hyp.shape[0]:
        raise ValueError("caption_eval: hyp (P, L) and ref (P, R) with contiguous rows expected")
    P, L = hyp.shape
    R = ref.shape[1]
    G = group_off.numel() - 1
    if hyp_len.numel() != P or ref_len.numel() != P or not hyp_len.is_contiguous() or not ref_len.is_contiguous() or \
            not group_off.is_contiguous():
        raise ValueError("caption_eval: hyp_len / ref_len (P) and group_off (G + 1), contiguous, expected")
    dev = hyp.device
    pair_ints = torch.empty(max(P, 0), CAPTION_EVAL_PAIR_INTS, dtype=torch.int32, device=dev)
    pair_lcs = torch.empty(max(P, 0), dtype=torch.int32, device=dev)
    pair_cider = torch.empty(max(P, 0), dtype=torch.float64, device=dev)
    group_scores = torch.empty(max(G, 0), CAPTION_EVAL_GROUP_SCORES, dtype=torch.float64, device=dev)
    _launch("bmhrl_caption_eval", hyp, hyp.stride(0), hyp_len, ref, ref.stride(0), ref_len, group_off, P, G, L, R, pair_ints,
            pair_lcs, pair_cider, group_scores)
    return pair_ints, pair_lcs, pair_cider, group_scores


# ---- paragraph n-gram statistics (csrc/paragraph.hip)
PARAGRAPH_MAX_TOKENS, NGRAM_STATS_INTS = 1024, 5             # BMHRL_PARAGRAPH_MAX_TOKENS / BMHRL_NGRAM_STATS_INTS


def ngram_stats(tok, sent_off, para_off):
    """(G, 4, 5) int32: total, distinct, in_repeated, cross, max_count of the n-grams, n = 1..4, of G paragraphs; see
    bmhrl_ngram_stats in include/bmhrl_hip.h.  tok (n_tok) int32 word ids, sent_off (S + 1) int32 token offsets of the
    sentences, para_off (G + 1) int32 sentence offsets of the paragraphs, all contiguous and on one device.  A paragraph
    holds at most PARAGRAPH_MAX_TOKENS tokens.  Synchronises the stream once (the offsets are checked on the host); not for
    captured graphs."""
    for t in (tok, sent_off, para_off):
        if t.dtype != torch.int32:
            raise ValueError("ngram_stats: int32 tensors expected")
    if tok.dim() != 1 or sent_off.dim() != 1 or para_off.dim() != 1 or not (tok.is_contiguous() and sent_off.is_contiguous()
                                                                            and para_off.is_contiguous()):
        raise ValueError("ngram_stats: tok (n_tok), sent_off (S + 1) and para_off (G + 1), contiguous, expected")
    if sent_off.numel() < 1 or para_off.numel() < 1:
        raise ValueError("ngram_stats: sent_off (S + 1) and para_off (G + 1) hold at least one offset")
    S, G = sent_off.numel() - 1, para_off.numel() - 1
    stats = torch.empty(G, 4, NGRAM_STATS_INTS, dtype=torch.int32, device=sent_off.device)
    _launch("bmhrl_ngram_stats", tok, tok.numel(), sent_off, S, para_off, G, stats)
    return stats


# ---- bootstrap over videos (csrc/bootstrap.hip)
BOOTSTRAP_MAX_N, BOOTSTRAP_MAX_M, BOOTSTRAP_MAX_R = 16384, 4096, 1 << 20      # BMHRL_BOOTSTRAP_MAX_N / _M / _R


def _f64c(t, shape, what):
    if t.dtype != torch.float64 or tuple(t.shape) != tuple(shape) or not t.is_contiguous():
        raise ValueError(f"{what}: expected a contiguous fp64 tensor of shape {tuple(shape)}")


def bootstrap_rows(N, resamples):
    """the rows of the output one workgroup of bootstrap_ratios carries at N videos (bmhrl_bootstrap_rows): what the
    benchmark needs to count the bytes the launch reads"""
    return _query("bmhrl_bootstrap_rows", int(N), int(resamples))


def bootstrap_ratios(values, weights, resamples, seed=0):
    """(resamples + 1, M) fp64: row 0 the observed statistic of every column, row r >= 1 that of resample r of the N videos;
    see bmhrl_bootstrap_ratios in include/bmhrl_hip.h (csrc/bootstrap.hip).  values (M, N) fp64 -- a column's N per-video
    values are contiguous -- and weights (M, N) fp64 or None: the statistic is sum(c * x) / sum(c * w) (0.0 for a zero
    denominator), without weights sum(c * x) / N, c the resample's counts (all 1 in row 0), drawn from hash_u32(seed, .).
    N <= BOOTSTRAP_MAX_N, M <= BOOTSTRAP_MAX_M, 1 <= resamples <= BOOTSTRAP_MAX_R; the inputs are finite (the callers in
    evaluate.py check).  One launch, nothing read back."""
    if values.dim() != 2:
        raise ValueError("bootstrap_ratios: values (M, N) expected")
    M, N = values.shape
    _f64c(values, (M, N), "bootstrap_ratios (values)")
    if weights is not None:
        _f64c(weights, (M, N), "bootstrap_ratios (weights)")
        if weights.device != values.device:
            raise ValueError("bootstrap_ratios: values and weights on one device expected")
    R, seed = int(resamples), int(seed)
    if not 0 <= seed < 1 << 64:
        raise ValueError(f"bootstrap_ratios: seed {seed} is no uint64")
    stats = torch.empty(max(R, 0) + 1, M, dtype=torch.float64, device=values.device)
    _launch("bmhrl_bootstrap_ratios", values, weights, N, M, R, seed, stats)
    return stats


# ---- SODA_c: the all-pairs METEOR matrix and the ordered assignment (csrc/soda.hip)
SODA_MAX_REFS, SODA_MAX_T = 256, 16          # BMHRL_SODA_MAX_REFS / _T of include/bmhrl_hip.h


def _soda_offsets(what, hyp_off, ref_off, cell_off):
    if hyp_off.dtype != torch.int32 or ref_off.dtype != torch.int32 or cell_off.dtype != torch.int64:
        raise ValueError(f"{what}: hyp_off / ref_off int32 and cell_off int64 expected")
    G = hyp_off.numel() - 1
    if ref_off.numel() != G + 1 or cell_off.numel() != G + 1 or not (hyp_off.is_contiguous() and ref_off.is_contiguous()
                                                                     and cell_off.is_contiguous()):
        raise ValueError(f"{what}: hyp_off, ref_off and cell_off (G + 1), contiguous, expected")
    return G


def meteor_matrix(hyp, vmap, vstem, syn_off, syn_ids, ref, ref_stem, ref_len, hyp_idx, ref_idx, hyp_off, ref_off, cell_off,
                  alpha, beta, gamma, S):
    """whole-sentence METEOR of every (prediction, reference) cell of G groups into S (n_cells) fp64, group g row-major at
    cell_off[g]; see bmhrl_meteor_matrix in include/bmhrl_hip.h.  hyp (Nh, L) int64 vocab ids and ref / ref_stem (Nr, R)
    int32 with ref_len (Nr) int32 are the distinct sentences, hyp_idx (sum P) / ref_idx (sum R) int32 name the groups'
    members, hyp_off / ref_off (G + 1) int32 and cell_off (G + 1) int64 delimit the groups.  vmap, vstem, syn_off, syn_ids
    as ops.meteor takes them.  Synchronises the stream once (offsets and indices are checked on the host); not for
    captured graphs."""
    G = _soda_offsets("meteor_matrix", hyp_off, ref_off, cell_off)
    V = vmap.numel()
    if hyp.dtype != torch.int64 or vmap.dtype != torch.int32 or ref.dtype != torch.int32 or ref_len.dtype != torch.int32 or \
            hyp_idx.dtype != torch.int32 or ref_idx.dtype != torch.int32:
        raise ValueError("meteor_matrix: hyp int64, vmap / ref / ref_len / hyp_idx / ref_idx int32 expected")
    if hyp.dim() != 2 or ref.dim() != 2 or hyp.stride(1) != 1 or ref.stride(1) != 1 or ref_len.numel() != ref.shape[0] or \
            not (vmap.is_contiguous() and ref_len.is_contiguous() and hyp_idx.is_contiguous() and ref_idx.is_contiguous()):
        raise ValueError("meteor_matrix: hyp (Nh, L) and ref (Nr, R) with contiguous rows, ref_len (Nr), contiguous vmap and "
                         "indices expected")
    if (vstem is None) != (ref_stem is None):
        raise ValueError("meteor_matrix: vstem and ref_stem go together")
    if vstem is not None:
        if vstem.dtype != torch.int32 or vstem.numel() != V or not vstem.is_contiguous():
            raise ValueError("meteor_matrix: vstem (V) int32 expected")
        if ref_stem.dtype != torch.int32 or ref_stem.shape != ref.shape or ref_stem.stride() != ref.stride():
            raise ValueError("meteor_matrix: ref_stem int32, shaped and strided like ref, expected")
    n_syn = 0
    if syn_off is not None and syn_ids is not None:
        n_syn = syn_ids.numel()
        if syn_off.dtype != torch.int32 or syn_ids.dtype != torch.int32 or syn_off.numel() != V + 1 or n_syn < 1 or \
                not syn_off.is_contiguous() or not syn_ids.is_contiguous():
            raise ValueError("meteor_matrix: syn_off (V + 1) int32 and syn_ids (>= 1) int32 expected")
    if S.dtype != torch.float64 or S.dim() != 1 or not S.is_contiguous():
        raise ValueError("meteor_matrix: S (cells) fp64, contiguous, expected")
    _launch("bmhrl_meteor_matrix", hyp, hyp.stride(0), hyp.shape[0], hyp.shape[1], vmap, vstem, V, syn_off, syn_ids, n_syn, ref,
            ref_stem, ref.stride(0), ref_len, ref.shape[0], ref.shape[1], hyp_idx, hyp_idx.numel(), ref_idx, ref_idx.numel(),
            hyp_off, ref_off, cell_off, G, float(alpha), float(beta), float(gamma), S, S.numel())


def soda_dp(pred_seg, ref_seg, hyp_off, ref_off, cell_off, S, tious):
    """(G, T, 4) fp64 max_score, precision, recall, F of the time-ordered one-to-one assignment that maximises the sum of
    tIoU x S per group and threshold; see bmhrl_soda_dp in include/bmhrl_hip.h.  pred_seg (sum P, 2) / ref_seg (sum R, 2)
    fp64 start, end in matching order; the offsets and S as ops.meteor_matrix; tious (T) fp64 on the device.  Synchronises
    the stream once; not for captured graphs."""
    G = _soda_offsets("soda_dp", hyp_off, ref_off, cell_off)
    for t in (pred_seg, ref_seg):
        if t.dtype != torch.float64 or t.dim() != 2 or t.shape[1] != 2 or not t.is_contiguous():
            raise ValueError("soda_dp: pred_seg / ref_seg (n, 2) fp64, contiguous, expected")
    if S.dtype != torch.float64 or S.dim() != 1 or not S.is_contiguous() or tious.dtype != torch.float64 or \
            tious.dim() != 1 or not tious.is_contiguous():
        raise ValueError("soda_dp: S (cells) and tious (T) fp64, contiguous, expected")
    T = tious.numel()
    out = torch.empty(max(G, 0), T, 4, dtype=torch.float64, device=S.device)
    _launch("bmhrl_soda_dp", pred_seg, pred_seg.shape[0], ref_seg, ref_seg.shape[0], hyp_off, ref_off, cell_off, G, S, S.numel(),
            tious, T, out)
    return out


# ---- proposal metrics: tIoU hit counts, first ranks and the ordered pair list (csrc/proposal_eval.hip)
TIOU_MAX_T = 16                              # BMHRL_TIOU_MAX_T of include/bmhrl_hip.h


class TiouGroups:
    """The group table of tiou_hits / tiou_pairs (see include/bmhrl_hip.h): `groups` (G, 4) integers, a row [p0, P, r0, R]
    naming the predictions [p0, p0 + P) and the references [r0, r0 + R) of a group.  Keeps the three copies the ABI takes:
    .host (G, 4) int32 numpy, .groups the same on `device`, .out_off (2, G + 1) int64 on `device` (the running sums of P and
    of R: where a group's outputs start), and .sum_p / .sum_r.  Build it once and reuse it across launches."""

    def __init__(self, groups, device):
        g = np.asarray(groups)
        if g.size == 0:
            g = np.zeros((0, 4), dtype=np.int32)
        if g.ndim != 2 or g.shape[1] != 4 or g.dtype.kind not in "iu":
            raise ValueError("TiouGroups: groups (G, 4) integers [p0, P, r0, R] expected")
        if g.size and (g.min() < 0 or g.max() > np.iinfo(np.int32).max):
            raise ValueError("TiouGroups: entries must lie in [0, 2^31)")
        self.host = np.ascontiguousarray(g, dtype=np.int32)
        self.G = int(g.shape[0])
        off = np.zeros((2, self.G + 1), dtype=np.int64)
        np.cumsum(self.host[:, 1], out=off[0, 1:])
        np.cumsum(self.host[:, 3], out=off[1, 1:])
        self.sum_p, self.sum_r = int(off[0, -1]), int(off[1, -1])
        self.groups = torch.from_numpy(self.host).to(device)
        self.out_off = torch.from_numpy(off).to(device)


def _tiou_segments(what, pred_seg, ref_seg, groups):
    if not isinstance(groups, TiouGroups):
        raise ValueError(f"{what}: groups must be an ops.TiouGroups")
    for t in (pred_seg, ref_seg):
        if t.dtype != torch.float64 or t.dim() != 2 or t.shape[1] != 2 or not t.is_contiguous():
            raise ValueError(f"{what}: pred_seg / ref_seg (n, 2) fp64, contiguous, expected")


def _tiou_out(what, t, rows, cols):
    if t.dtype != torch.int32 or t.dim() != 2 or t.shape[0] != rows or t.shape[1] < cols or (t.shape[1] > 1 and t.stride(1) != 1) \
            or (rows > 1 and t.stride(0) < t.shape[1]):
        raise ValueError(f"{what}: out must hold int32 ({rows}, >= {cols}) tensors with contiguous rows")
    return t.stride(0) if rows > 1 else t.shape[1]


def tiou_hits(pred_seg, ref_seg, groups, tious, strict, out=None):
    """(pred_hits (T, sum P), ref_first (T, sum R)) int32 of one launch over all groups and thresholds; see bmhrl_tiou_hits
    in include/bmhrl_hip.h.  pred_seg (n_pred, 2) / ref_seg (n_ref, 2) fp64 start, end; groups: a TiouGroups on the same
    device; tious (T) fp64 on the device; strict: a cell passes with iou > tious[t] (True) or iou >= tious[t] (False).
    pred_hits[t][slot] = the number of its group's references the prediction passes, ref_first[t][slot] = the smallest
    in-group index of a prediction passing the reference, P when there is none.  out: optionally the two tensors to
    write, rows of at least sum P / sum R words (words behind them are left alone).  Does not synchronise."""
    _tiou_segments("tiou_hits", pred_seg, ref_seg, groups)
    if tious.dtype != torch.float64 or tious.dim() != 1 or not tious.is_contiguous() or not 1 <= tious.numel() <= TIOU_MAX_T:
        raise ValueError(f"tiou_hits: tious (1 <= T <= {TIOU_MAX_T}) fp64, contiguous, expected")
    T = tious.numel()
    if out is None:
        out = (torch.empty(T, groups.sum_p, dtype=torch.int32, device=pred_seg.device),
               torch.empty(T, groups.sum_r, dtype=torch.int32, device=pred_seg.device))
    pred_hits, ref_first = out
    ldp, ldr = _tiou_out("tiou_hits", pred_hits, T, groups.sum_p), _tiou_out("tiou_hits", ref_first, T, groups.sum_r)
    _launch("bmhrl_tiou_hits", pred_seg, pred_seg.shape[0], ref_seg, ref_seg.shape[0], groups.host.ctypes.data, groups.groups,
            groups.out_off, groups.G, tious, T, int(bool(strict)), pred_hits, ldp, ref_first, ldr)
    return pred_hits[:, :groups.sum_p], ref_first[:, :groups.sum_r]


def tiou_pairs(pred_seg, ref_seg, groups, tiou, pair_off, n_pairs, out=None):
    """pair_ref (n_pairs) int32: behind pair_off[slot] the rows of ref_seg, ascending, that the slot's prediction reaches
    with iou >= tiou within its group, or one -1; see bmhrl_tiou_pairs in include/bmhrl_hip.h.  pair_off (sum P + 1) int64
    on the device: the exclusive running sum of max(pred_hits[t], 1) of tiou_hits(strict=False) over the same tables with
    tious[t] == tiou; n_pairs: its last entry.  out: optionally the (>= n_pairs) int32 tensor to write.  Does not
    synchronise."""
    _tiou_segments("tiou_pairs", pred_seg, ref_seg, groups)
    n_pairs = int(n_pairs)
    if pair_off.dtype != torch.int64 or pair_off.dim() != 1 or pair_off.numel() != groups.sum_p + 1 or \
            not pair_off.is_contiguous() or n_pairs < 0:
        raise ValueError("tiou_pairs: pair_off (sum P + 1) int64, contiguous, and n_pairs >= 0 expected")
    if out is None:
        out = torch.empty(n_pairs, dtype=torch.int32, device=pred_seg.device)
    if out.dtype != torch.int32 or out.dim() != 1 or out.numel() < n_pairs or not out.is_contiguous():
        raise ValueError("tiou_pairs: out must be a contiguous int32 tensor of at least n_pairs words")
    _launch("bmhrl_tiou_pairs", pred_seg, pred_seg.shape[0], ref_seg, ref_seg.shape[0], groups.host.ctypes.data, groups.groups,
            groups.out_off, groups.G, float(tiou), pair_off, groups.sum_p, out, n_pairs)
    return out[:n_pairs]


# ---- sampled caption decoding (csrc/sample.hip)
SAMPLE_MAX_V = 16384                         # BMHRL_SAMPLE_MAX_V of include/bmhrl_hip.h


def sample_step(logp, ld, rows, V, temperature, top_k, top_p, seed, seed_dev, t, end_idx, pad_idx, finished, tok, out,
                sum_logp, step_logp=None, step_logq=None, row_offset=0):
    """one step of the sampling rules for every row (see bmhrl_sample_step in include/bmhrl_hip.h): logp (rows, ld >= V)
    fp32; finished (rows) uint8 / bool, tok (rows) int64, sum_logp (rows) fp32 updated in place; out (rows, cols) int64 gets
    column t + 1, step_logp / step_logq (rows, cols) fp32 (optional, the same row stride) column t.  seed_dev: None or a
    (1,) int64 word added to seed (uint64 wraparound); t: (1,) int64 device word."""
    if not (1 <= V <= SAMPLE_MAX_V and ld >= V and rows >= 1 and logp.dtype == torch.float32
            and logp.numel() >= (rows - 1) * ld + V):
        raise ValueError(f"sample_step: need 1 <= V <= {SAMPLE_MAX_V} and fp32 logp rows (rows, ld >= V)")
    if not (math.isfinite(temperature) and temperature >= 0 and top_k >= 0 and 0 < top_p <= 1):
        raise ValueError("sample_step: need a finite temperature >= 0, top_k >= 0 and 0 < top_p <= 1")
    if not (0 <= pad_idx < V and row_offset >= 0 and 0 <= seed < 2**64):
        raise ValueError("sample_step: need 0 <= pad_idx < V, row_offset >= 0 and a uint64 seed")
    for x, dts in ((finished, (torch.uint8, torch.bool)), (tok, (torch.int64,)), (sum_logp, (torch.float32,))):
        if x.dtype not in dts or x.numel() < rows or not x.is_contiguous():
            raise ValueError(f"sample_step: expected a contiguous {dts[0]} buffer of {rows} elements")
    if out.dtype != torch.int64 or out.dim() != 2 or out.shape[0] != rows or out.stride(1) != 1:
        raise ValueError("sample_step: out must be (rows, cols) int64 with contiguous rows")
    for h in (step_logp, step_logq):
        if h is not None and (h.dtype != torch.float32 or h.shape != out.shape or h.stride() != out.stride()):
            raise ValueError("sample_step: step_logp / step_logq must be fp32 with the shape and strides of out")
    if t.dtype != torch.int64 or (seed_dev is not None and seed_dev.dtype != torch.int64):
        raise ValueError("sample_step: t and seed_dev are int64 words")
    _launch("bmhrl_sample_step", logp, ld, rows, V, float(temperature), int(top_k), float(top_p), int(seed), seed_dev, t,
            row_offset, end_idx, pad_idx, finished, tok, out, out.stride(0), sum_logp, step_logp, step_logq)


# ---- constrained caption decoding (csrc/constrain.hip)
LOGIT_RULES_MAX_HIST = 256                    # BMHRL_LOGIT_RULES_MAX_HIST of include/bmhrl_hip.h


def logit_rules(logp, ld, rows, V, hist, t, ngram, min_len, penalty, end_idx, pad_idx):
    """repetition penalty, no-repeat n-gram ban and minimum length on every row of logp (rows, ld >= V) fp32, in place (see
    bmhrl_logit_rules in include/bmhrl_hip.h): hist (rows, cols <= LOGIT_RULES_MAX_HIST) int64 holds the rows' sequences,
    columns 0 .. t; t: (1,) int64 device word."""
    if not (V >= 1 and ld >= V and rows >= 1 and logp.dtype == torch.float32 and logp.numel() >= (rows - 1) * ld + V):
        raise ValueError("logit_rules: need V >= 1 and fp32 logp rows (rows, ld >= V)")
    if not (ngram >= 0 and min_len >= 0 and math.isfinite(penalty) and penalty > 0):
        raise ValueError("logit_rules: need ngram >= 0, min_len >= 0 and a finite penalty > 0")
    if not (0 <= end_idx < V and 0 <= pad_idx < V):
        raise ValueError("logit_rules: need 0 <= end_idx < V and 0 <= pad_idx < V")
    if hist.dtype != torch.int64 or hist.dim() != 2 or hist.shape[0] != rows or hist.stride(1) != 1 or \
            not 1 <= hist.shape[1] <= LOGIT_RULES_MAX_HIST or hist.stride(0) != hist.shape[1]:
        raise ValueError(f"logit_rules: hist must be a contiguous (rows, cols <= {LOGIT_RULES_MAX_HIST}) int64 buffer")
    if t.dtype != torch.int64:
        raise ValueError("logit_rules: t is an int64 word")
    _launch("bmhrl_logit_rules", logp, ld, rows, V, hist, hist.stride(0), t, int(ngram), int(min_len), float(penalty), end_idx,
            pad_idx)


LOGIT_RULES_MAX_CTX = 1024                    # BMHRL_LOGIT_RULES_MAX_CTX of include/bmhrl_hip.h
LOGIT_RULES_CTX_MAX_V = 65536                 # BMHRL_LOGIT_RULES_CTX_MAX_V


def logit_rules_ctx(logp, ld, rows, V, hist, t, ngram, min_len, penalty, end_idx, pad_idx, ctx, rows_per_ctx, ctx_ngram,
                    ctx_penalty):
    """logit_rules and the context rules C1-C2 in one launch (see bmhrl_logit_rules_ctx in include/bmhrl_hip.h): ctx
    (rows / rows_per_ctx, cols <= LOGIT_RULES_MAX_CTX) int64 holds per clip the tokens of the video's earlier captions, an
    entry outside [0, V) or equal to pad_idx a gap; row r reads context row r // rows_per_ctx.  V <= LOGIT_RULES_CTX_MAX_V."""
    if not (1 <= V <= LOGIT_RULES_CTX_MAX_V and ld >= V and rows >= 1 and logp.dtype == torch.float32
            and logp.numel() >= (rows - 1) * ld + V):
        raise ValueError(f"logit_rules_ctx: need 1 <= V <= {LOGIT_RULES_CTX_MAX_V} and fp32 logp rows (rows, ld >= V)")
    if not (ngram >= 0 and min_len >= 0 and math.isfinite(penalty) and penalty > 0):
        raise ValueError("logit_rules_ctx: need ngram >= 0, min_len >= 0 and a finite penalty > 0")
    if not (ctx_ngram >= 0 and math.isfinite(ctx_penalty) and ctx_penalty > 0):
        raise ValueError("logit_rules_ctx: need ctx_ngram >= 0 and a finite ctx_penalty > 0")
    if not (0 <= end_idx < V and 0 <= pad_idx < V):
        raise ValueError("logit_rules_ctx: need 0 <= end_idx < V and 0 <= pad_idx < V")
    if hist.dtype != torch.int64 or hist.dim() != 2 or hist.shape[0] != rows or hist.stride(1) != 1 or \
            not 1 <= hist.shape[1] <= LOGIT_RULES_MAX_HIST or hist.stride(0) != hist.shape[1]:
        raise ValueError(f"logit_rules_ctx: hist must be a contiguous (rows, cols <= {LOGIT_RULES_MAX_HIST}) int64 buffer")
    if not (rows_per_ctx >= 1 and rows % rows_per_ctx == 0):
        raise ValueError("logit_rules_ctx: rows_per_ctx must be >= 1 and divide rows")
    if ctx.dtype != torch.int64 or ctx.dim() != 2 or ctx.shape[0] != rows // rows_per_ctx or not ctx.is_contiguous() or \
            not 1 <= ctx.shape[1] <= LOGIT_RULES_MAX_CTX:
        raise ValueError(f"logit_rules_ctx: ctx must be a contiguous (rows / rows_per_ctx, cols <= {LOGIT_RULES_MAX_CTX}) int64 "
                         "buffer")
    if t.dtype != torch.int64:
        raise ValueError("logit_rules_ctx: t is an int64 word")
    _launch("bmhrl_logit_rules_ctx", logp, ld, rows, V, hist, hist.stride(0), t, int(ngram), int(min_len), float(penalty),
            end_idx, pad_idx, ctx, ctx.shape[1], int(rows_per_ctx), int(ctx_ngram), float(ctx_penalty))


# ---- consensus choice among a clip's hypotheses (csrc/consensus.hip)
CONSENSUS_MAX_STEPS = 256                     # BMHRL_CONSENSUS_MAX_STEPS of include/bmhrl_hip.h (K: BEAM_MAX)
CONSENSUS_MAX_N = 4                           # BMHRL_CONSENSUS_MAX_N


def consensus(hist, steps, K, end_idx, n=4, token_weight=None, pair=False):
    """the consensus utilities util (B, K) fp64 of the hypotheses in hist (B * K, cols >= steps + 1) int64 -- a decoder's
    token history: K consecutive rows per clip, column 0 the start token, columns 1 .. steps the generated tokens (see
    bmhrl_consensus in include/bmhrl_hip.h).  n: the largest gram length; token_weight: None or (V,) fp32 on hist's device;
    pair=True: also the pairwise utilities (B, K, K) fp64, u(i, i) written as 0."""
    for t in (hist, token_weight):
        _ptr(t)                         # (CPU memory is refused before the devices are compared below)
    steps, K, n = int(steps), int(K), int(n)
    if not (1 <= K <= BEAM_MAX and 0 <= steps <= CONSENSUS_MAX_STEPS and 1 <= n <= CONSENSUS_MAX_N):
        raise ValueError(f"consensus: need 1 <= K <= {BEAM_MAX}, 0 <= steps <= {CONSENSUS_MAX_STEPS} and "
                         f"1 <= n <= {CONSENSUS_MAX_N}")
    if hist.dtype != torch.int64 or hist.dim() != 2 or hist.shape[0] < 1 or hist.shape[0] % K or hist.shape[1] < steps + 1 or \
            hist.stride(1) != 1 or hist.stride(0) < steps + 1:
        raise ValueError("consensus: hist must be (B * K, cols >= steps + 1) int64 with contiguous rows")
    V = 0
    if token_weight is not None:
        V = token_weight.numel()
        if token_weight.dtype != torch.float32 or token_weight.dim() != 1 or V < 1 or not token_weight.is_contiguous() or \
                token_weight.device != hist.device:
            raise ValueError("consensus: token_weight must be a contiguous (V >= 1,) fp32 tensor on hist's device")
    B = hist.shape[0] // K
    util = torch.empty(B, K, dtype=torch.float64, device=hist.device)
    pairs = torch.empty(B, K, K, dtype=torch.float64, device=hist.device) if pair else None
    _launch("bmhrl_consensus", hist, hist.stride(0), B, K, steps, int(end_idx), n, token_weight, V, util, pairs)
    return (util, pairs) if pair else util


# ---- DETR word loss: Hungarian matching + weighted cross entropy (csrc/word_loss.hip)
WORD_LOSS_MAX_Q = 128                         # BMHRL_WORD_LOSS_MAX_Q of include/bmhrl_hip.h
WORD_LOSS_MAX_L = 64                          # BMHRL_WORD_LOSS_MAX_L


def _rows_ld(x, shape, what):
    """leading dimension of the B * Q fp32 rows of x (B, Q, C): unit column stride and ONE row stride >= C throughout (a
    view of the first C columns of a wider buffer qualifies)"""
    if x.dtype != torch.float32 or tuple(x.shape) != tuple(shape):
        raise ValueError(f"{what}: expected an fp32 tensor of shape {tuple(shape)}")
    B, Q, Cn = shape
    ld = x.stride(1) if Q > 1 else (x.stride(0) if B > 1 else Cn)
    if (Cn > 1 and x.stride(2) != 1) or ld < Cn or (Q > 1 and B > 1 and x.stride(0) != Q * ld):
        raise ValueError(f"{what}: rows must have unit column stride and one row stride >= {Cn}")
    return ld


def word_cost(logits, captions, pad_idx, cost_scale=1.0):
    """the cost pass of the DETR word loss (see bmhrl_word_cost in include/bmhrl_hip.h): logits (B, Q, C) fp32 whose rows
    may sit in a wider buffer (any row stride >= C), captions (B, L) int64.  Returns words (B, L) int32, n_words (B) int32,
    lse (2, B, Q) -- the log-sum-exp and the rounding residue of its last addition, an fp32 pair the later launches subtract
    together --, x_none (B, Q), gathered (B, Q, L) and cost (B, Q, L) fp32."""
    if logits.dim() != 3 or captions.dim() != 2 or captions.dtype != torch.int64 or captions.shape[0] != logits.shape[0] or \
            (captions.shape[1] > 1 and captions.stride(1) != 1):
        raise ValueError("word_cost: logits (B, Q, C) fp32 and captions (B, L) int64 with contiguous rows expected")
    B, Q, Cn = logits.shape
    L = captions.shape[1]
    ld = _rows_ld(logits, (B, Q, Cn), "word_cost")
    dev = logits.device
    words = torch.empty(B, L, dtype=torch.int32, device=dev)
    n_words = torch.empty(B, dtype=torch.int32, device=dev)
    lse = torch.empty(2, B, Q, device=dev)
    x_none = torch.empty(B, Q, device=dev)
    gathered = torch.empty(B, Q, L, device=dev)
    cost = torch.empty(B, Q, L, device=dev)
    _launch("bmhrl_word_cost", logits, ld, captions, captions.stride(0) if B > 1 else max(L, 1), int(pad_idx), float(cost_scale),
            B, Q, L, Cn, words, n_words, lse[0], lse[1], x_none, gathered, cost)
    return words, n_words, lse, x_none, gathered, cost


def lsa_match(cost, n, out=None):
    """minimum-cost assignment per sample (see bmhrl_lsa_match): cost (B, Q, L) fp32 with any positive strides, n (B) int32
    targets per sample.  Returns query_of_target (B, L) int32: a distinct query for each target j < n[b], -1 behind them."""
    if cost.dim() != 3 or cost.dtype != torch.float32 or n.dtype != torch.int32 or n.numel() != cost.shape[0] or \
            not n.is_contiguous():
        raise ValueError("lsa_match: cost (B, Q, L) fp32 and n (B) int32 expected")
    B, Q, L = cost.shape
    if out is None:
        out = torch.empty(B, L, dtype=torch.int32, device=cost.device)
    elif out.dtype != torch.int32 or tuple(out.shape) != (B, L) or not out.is_contiguous():
        raise ValueError("lsa_match: out must be a contiguous (B, L) int32 tensor")
    sb, sq, sl = (s if d > 1 else 1 for s, d in zip(cost.stride(), cost.shape))
    _launch("bmhrl_lsa_match", cost, sb, sq, sl, n, B, Q, L, out)
    return out


def word_loss(words, n_words, query_of_target, lse, x_none, gathered, eos_coef, C):
    """class map, row weights and the weighted mean (see bmhrl_word_loss).  Returns tgt_class (B, Q) int32, row_w (B, Q)
    fp32 and loss_scale (2,) fp32 = [loss, 1 / sum row_w]."""
    if gathered.dim() != 3:
        raise ValueError("word_loss: gathered must be (B, Q, L)")
    B, Q, L = gathered.shape
    for t, shape, dt in ((words, (B, L), torch.int32), (n_words, (B,), torch.int32), (query_of_target, (B, L), torch.int32),
                         (lse, (2, B, Q), torch.float32), (x_none, (B, Q), torch.float32), (gathered, (B, Q, L), torch.float32)):
        if t.dtype != dt or tuple(t.shape) != shape or not t.is_contiguous():
            raise ValueError(f"word_loss: expected a contiguous {dt} tensor of shape {shape}")
    dev = gathered.device
    tgt_class = torch.empty(B, Q, dtype=torch.int32, device=dev)
    row_w = torch.empty(B, Q, device=dev)
    loss_scale = torch.empty(2, device=dev)
    _launch("bmhrl_word_loss", words, n_words, query_of_target, lse[0], lse[1], x_none, gathered, float(eos_coef), B, Q, L, int(C),
            tgt_class, row_w, loss_scale)
    return tgt_class, row_w, loss_scale


def word_loss_bwd(logits, lse, tgt_class, row_w, loss_scale, g=None, out=None):
    """d loss / d logits (see bmhrl_word_loss_bwd): logits (B, Q, C) fp32 and lse (2, B, Q) as word_cost takes and
    returns them; g: None or a (1,) fp32
    device scalar, the incoming gradient; out: None or (B, Q, C) fp32 rows in a buffer of any row stride >= C, whose
    padding columns are left alone."""
    if logits.dim() != 3:
        raise ValueError("word_loss_bwd: logits must be (B, Q, C)")
    B, Q, Cn = logits.shape
    ld = _rows_ld(logits, (B, Q, Cn), "word_loss_bwd")
    if out is None:
        out = torch.empty(B, Q, Cn, device=logits.device)
    ldd = _rows_ld(out, (B, Q, Cn), "word_loss_bwd (out)")
    for t, n, dt in ((lse, 2 * B * Q, torch.float32), (tgt_class, B * Q, torch.int32), (row_w, B * Q, torch.float32),
                     (loss_scale, 2, torch.float32)):
        if t.dtype != dt or t.numel() != n or not t.is_contiguous():
            raise ValueError(f"word_loss_bwd: expected a contiguous {dt} tensor of {n} elements")
    if g is not None and (g.dtype != torch.float32 or g.numel() != 1):
        raise ValueError("word_loss_bwd: g is a (1,) fp32 device scalar")
    _launch("bmhrl_word_loss_bwd", logits, ld, lse, _at(lse, B * Q), tgt_class, row_w, loss_scale, g, out, ldd, B, Q, Cn)
    return out


# ---- temporal proposal generation: target assignment, head decode + loss, top-k + NMS (csrc/proposal.hip)
PROPOSAL_MAX_K = 128                          # BMHRL_PROPOSAL_MAX_K of include/bmhrl_hip.h
PROPOSAL_MAX_N = 1 << 24                      # BMHRL_PROPOSAL_MAX_N
_PROPOSAL_CHUNK = 4096                        # keys sorted per block (csrc/proposal.hip kChunk)


def _f32c(t, shape, what):
    if t.dtype != torch.float32 or tuple(t.shape) != tuple(shape) or not t.is_contiguous():
        raise ValueError(f"{what}: expected a contiguous fp32 tensor of shape {tuple(shape)}")


def proposal_assign(targets, anchors, cell_sec, B, S):
    """target assignment of one modality (see bmhrl_proposal_assign): targets (N, 4) fp32 rows [video index, centre s,
    length s, meta index], anchors (A) fp32 seconds.  Returns owner (B, A, S) int32 (the target row that owns the cell, -1
    for none), tx (N), tw (N) fp32 and counts (2) int32 = [owned cells, the others], all on the device."""
    if targets.dim() != 2 or targets.shape[1] != 4 or anchors.dim() != 1:
        raise ValueError("proposal_assign: targets (N, 4) and anchors (A) expected")
    N, A = targets.shape[0], anchors.shape[0]
    _f32c(targets, (N, 4), "proposal_assign (targets)")
    _f32c(anchors, (A,), "proposal_assign (anchors)")
    dev = anchors.device
    owner = torch.empty(B, A, S, dtype=torch.int32, device=dev)
    tx = torch.empty(N, device=dev)
    tw = torch.empty(N, device=dev)
    counts = torch.empty(2, dtype=torch.int32, device=dev)
    _launch("bmhrl_proposal_assign", targets if N else None, N, anchors, A, float(cell_sec), int(B), int(S), owner,
            tx if N else None, tw if N else None, counts)
    return owner, tx, tw, counts


def proposal_head(x, anchors, cell_sec, pred, row_off, assigned=None, obj_coeff=1.0, noobj_coeff=100.0, sums=None, dx=None,
                  dscale=None):
    """decode, loss and gradient of one head (see bmhrl_proposal_head): x (B, S, 3A) fp32, pred (B, N_total, 3) fp32 whose
    rows row_off .. row_off + A*S - 1 are written.  assigned = proposal_assign's (owner, tx, tw, counts) selects training:
    sums (5) fp32 = [loss_x, loss_w, loss_obj, loss_noobj, total] is written (allocated when None) and dx (B, S, 3A), when
    given, gets dscale * d total / d x.  assigned=None is inference: predictions only.  Returns sums (None in inference)."""
    if x.dim() != 3 or anchors.dim() != 1 or x.shape[2] != 3 * anchors.shape[0] or pred.dim() != 3:
        raise ValueError("proposal_head: x (B, S, 3A), anchors (A) and pred (B, N_total, 3) expected")
    B, S, A = x.shape[0], x.shape[1], anchors.shape[0]
    _f32c(x, (B, S, 3 * A), "proposal_head (x)")
    _f32c(anchors, (A,), "proposal_head (anchors)")
    _f32c(pred, (B, pred.shape[1], 3), "proposal_head (pred)")
    dev = x.device
    owner = tx = tw = counts = partials = counter = None
    if assigned is not None:
        owner, tx, tw, counts = assigned
        if owner.dtype != torch.int32 or tuple(owner.shape) != (B, A, S) or not owner.is_contiguous() or \
                counts.dtype != torch.int32 or counts.numel() != 2:
            raise ValueError("proposal_head: assigned must be proposal_assign's result for this head's (B, A, S)")
        if sums is None:
            sums = torch.empty(5, device=dev)
        _f32c(sums, (5,), "proposal_head (sums)")
        if dx is not None:
            _f32c(dx, (B, S, 3 * A), "proposal_head (dx)")
        if dscale is not None and (dscale.dtype != torch.float32 or dscale.numel() != 1):
            raise ValueError("proposal_head: dscale is a (1,) fp32 device scalar")
        partials = torch.empty(4 * 1024, device=dev)                    # 4 * BMHRL_PROPOSAL_HEAD_BLOCKS
        counter = torch.empty(4, dtype=torch.int32, device=dev)        # the ticket word (the call zeroes it on the stream)
    elif dx is not None or sums is not None:
        raise ValueError("proposal_head: sums and dx need assigned targets")
    _launch("bmhrl_proposal_head", x, anchors, float(cell_sec), B, S, A, pred, pred.shape[1], int(row_off), owner, tx, tw, counts,
            float(obj_coeff), float(noobj_coeff), dscale, dx, sums, partials, counter)
    return sums


def proposal_select_workspace(N, k):
    """64-bit words per video bmhrl_proposal_select needs"""
    if N <= _PROPOSAL_CHUNK:
        return 0
    c1 = -(-N // _PROPOSAL_CHUNK) * k
    return c1 + -(-c1 // _PROPOSAL_CHUNK) * k


def proposal_select(predictions, durations, k, nms_tiou=None):
    """top-k + corner coordinates + trimming + greedy NMS of a batch (see bmhrl_proposal_select): predictions (B, N, 3) fp32
    rows [centre s, length s, confidence], durations (B) fp32, nms_tiou None = no suppression.  Returns props (B, k, 3) =
    [start, end, confidence], survivors first in confidence order and zeros behind them, and count (B) int32."""
    if predictions.dim() != 3 or predictions.shape[2] != 3:
        raise ValueError("proposal_select: predictions (B, N, 3) expected")
    B, N = predictions.shape[0], predictions.shape[1]
    _f32c(predictions, (B, N, 3), "proposal_select (predictions)")
    _f32c(durations, (B,), "proposal_select (durations)")
    k = int(k)
    dev = predictions.device
    props = torch.empty(B, max(k, 0), 3, device=dev)
    count = torch.empty(B, dtype=torch.int32, device=dev)
    words = B * proposal_select_workspace(N, k) if 1 <= k <= PROPOSAL_MAX_K else 0
    ws = torch.empty(words, dtype=torch.int64, device=dev) if words else None
    _launch("bmhrl_proposal_select", predictions, B, N, durations, k, -1.0 if nms_tiou is None else float(nms_tiou), props, count,
            ws, words)
    return props, count


PROPOSAL_SOFT_MAX_M = 1024                    # BMHRL_PROPOSAL_SOFT_MAX_M
NMS_METHODS = {"hard": 0, "linear": 1, "gaussian": 2}            # BMHRL_NMS_*


def proposal_select_soft(predictions, durations, m, k, method, tiou_thresh=0.0, sigma=0.5, min_score=None):
    """Soft-NMS over a pool (see bmhrl_proposal_select_soft): predictions (B, N, 3) fp32 rows [centre s, length s,
    confidence], durations (B) fp32; the pool is the m rows of highest confidence, of which at most k are picked by their
    current score.  method: "hard", "linear" or "gaussian" (or the BMHRL_NMS_* number); min_score None = no floor.  Returns
    props (B, k, 3) = [start, end, rescored confidence] in pick order with zeros behind, rows (B, k) int32 = the picked
    rows of `predictions` with -1 behind, and count (B) int32."""
    if predictions.dim() != 3 or predictions.shape[2] != 3:
        raise ValueError("proposal_select_soft: predictions (B, N, 3) expected")
    if isinstance(method, str):
        if method not in NMS_METHODS:
            raise ValueError(f"proposal_select_soft: method is one of {sorted(NMS_METHODS)}, got {method!r}")
        method = NMS_METHODS[method]
    B, N = predictions.shape[0], predictions.shape[1]
    _f32c(predictions, (B, N, 3), "proposal_select_soft (predictions)")
    _f32c(durations, (B,), "proposal_select_soft (durations)")
    m, k = int(m), int(k)
    dev = predictions.device
    props = torch.empty(B, max(k, 0), 3, device=dev)
    rows = torch.empty(B, max(k, 0), dtype=torch.int32, device=dev)
    count = torch.empty(B, dtype=torch.int32, device=dev)
    words = B * proposal_select_workspace(N, m) if 1 <= m <= PROPOSAL_SOFT_MAX_M else 0
    ws = torch.empty(words, dtype=torch.int64, device=dev) if words else None
    _launch("bmhrl_proposal_select_soft", predictions, B, N, durations, m, k, int(method), float(tiou_thresh), float(sigma),
            float("-inf") if min_score is None else float(min_score), props, rows, count, ws, words)
    return props, rows, count


PROPOSAL_CHAIN_MAX_P = 1024                   # BMHRL_PROPOSAL_CHAIN_MAX_P
PROPOSAL_CHAIN_MAX_L = 32                     # BMHRL_PROPOSAL_CHAIN_MAX_L


def proposal_chain(props, count, max_events, max_tiou=0.0, overlap_weight=0.0, event_cost=0.0, min_length=0.2):
    """event-chain selection (see bmhrl_proposal_chain, csrc/event_chain.hip): props (B, P, 3) fp32 rows [start, end, score]
    and count (B) int32 as proposal_select / proposal_select_soft return them (count None = all P rows).  Per video the
    time-ordered chain of at most max_events eligible rows that maximises the sum of (score - event_cost) minus
    overlap_weight times the tIoU of neighbours, neighbours overlapping by at most max_tiou.  Returns events (B, max_events,
    3) = the chosen rows in time order with zeros behind, chain (B, max_events) int32 = their row indices with -1 behind,
    length (B) int32 and value (B) fp32.  One launch, nothing read back."""
    if props.dim() != 3 or props.shape[2] != 3:
        raise ValueError("proposal_chain: props (B, P, 3) expected")
    B, P = props.shape[0], props.shape[1]
    _f32c(props, (B, P, 3), "proposal_chain (props)")
    if count is not None and (count.dtype != torch.int32 or tuple(count.shape) != (B,) or not count.is_contiguous()):
        raise ValueError(f"proposal_chain (count): expected a contiguous int32 tensor of shape {(B,)}")
    L = int(max_events)
    dev = props.device
    events = torch.empty(B, max(L, 0), 3, device=dev)
    chain = torch.empty(B, max(L, 0), dtype=torch.int32, device=dev)
    length = torch.empty(B, dtype=torch.int32, device=dev)
    value = torch.empty(B, device=dev)
    _launch("bmhrl_proposal_chain", props, count, B, P, L, float(max_tiou), float(overlap_weight), float(event_cost),
            float(min_length), events, chain, length, value)
    return events, chain, length, value


# ---- segment crop: the rows of temporal segments out of device-resident full-length stacks (csrc/segment_crop.hip)
def crop_segments(src, src_len, durations, seg_video, seg_times, pad_value, T_out, out=None):
    """crop and pad P segments out of the full-length stacks of V videos (see bmhrl_crop_segments): src (V, S_pad, D) fp32,
    src_len (V) int32 true row counts, durations (V) float64 seconds, seg_video (P) int32, seg_times (P, 2) float64 [start,
    end].  Returns out (P, T_out, D) fp32, lengths (P) int32 (the crop's row count, not clipped to T_out), lo (P) int32 (its
    first row) and status (2) int32 = [segments longer than T_out, segments without a defined crop], all on the device;
    nothing is read back.  `out`: a contiguous (P, T_out, D) fp32 tensor to fill instead of a new one."""
    for t in (src, src_len, durations, seg_video, seg_times, out):
        _ptr(t)                         # (CPU memory is refused before the devices are compared below)
    if src.dim() != 3 or seg_times.dim() != 2:
        raise ValueError("crop_segments: src (V, S_pad, D) and seg_times (P, 2) expected")
    V, S_pad, D = src.shape
    P, T_out = seg_times.shape[0], int(T_out)
    if min(V, S_pad, D, P, T_out) < 1:
        raise ValueError(f"crop_segments: V, S_pad, D, P and T_out must be >= 1, got {(V, S_pad, D, P, T_out)}")
    _f32c(src, (V, S_pad, D), "crop_segments (src)")
    for t, dtype, shape, what in ((src_len, torch.int32, (V,), "src_len"), (durations, torch.float64, (V,), "durations"),
                                  (seg_video, torch.int32, (P,), "seg_video"), (seg_times, torch.float64, (P, 2), "seg_times")):
        if t.dtype != dtype or tuple(t.shape) != shape or not t.is_contiguous():
            raise ValueError(f"crop_segments ({what}): expected a contiguous {dtype} tensor of shape {shape}")
        if t.device != src.device:
            raise ValueError(f"crop_segments ({what}): on {t.device}, src on {src.device}")
    dev = src.device
    if out is None:
        out = torch.empty(P, T_out, D, device=dev)
    else:
        _f32c(out, (P, T_out, D), "crop_segments (out)")
        if out.device != dev:
            raise ValueError(f"crop_segments (out): on {out.device}, src on {dev}")
    lengths = torch.empty(P, dtype=torch.int32, device=dev)
    lo = torch.empty(P, dtype=torch.int32, device=dev)
    status = torch.empty(2, dtype=torch.int32, device=dev)
    _launch("bmhrl_crop_segments", src, src_len, durations, V, S_pad, D, seg_video, seg_times, P, float(pad_value), T_out, out,
            lengths, lo, status)
    return out, lengths, lo, status


# ---- self-critical policy gradient on sampled rollouts (csrc/policy_loss.hip)
ROLLOUT_MAX_N = 16                            # BMHRL_ROLLOUT_MAX_N of include/bmhrl_hip.h
BASELINE_NONE, BASELINE_LEAVE_ONE_OUT, BASELINE_GIVEN = 0, 1, 2      # BMHRL_BASELINE_*


def _rows2d(t, dtype, rows, cols, what):
    """row stride of a (rows, >= cols) tensor of `dtype` with unit column stride"""
    if t.dtype != dtype or t.dim() != 2 or t.shape[0] != rows or t.shape[1] < cols or (t.shape[1] > 1 and t.stride(1) != 1):
        raise ValueError(f"{what}: expected a ({rows}, >= {cols}) {dtype} tensor with contiguous rows")
    return t.stride(0) if rows > 1 else max(t.stride(0), cols)


def rollout_advantage(toks, n, m, end_idx, scores, baseline=BASELINE_LEAVE_ONE_OUT, base=None, out=None):
    """rules R1-R7 of bmhrl_rollout_advantage (include/bmhrl_hip.h): toks (B * n, >= m + 1) int64 sample-major, column 0 the
    start token; scores (B * n, >= m) fp64, the per-prefix table of toks[:, 1:]; base (B,) fp64 with BASELINE_GIVEN.
    -> (len (B * n,) int32, reward (B * n,) fp64, adv (B * n,) fp64, weight (B * n, m) fp32, stats (4,) fp64 = mean reward,
    mean baseline, mean length, token count).  out: the same five tensors to write into (weight may be a view with a wider
    row stride).  Nothing is read on the host."""
    n, m, baseline = int(n), int(m), int(baseline)
    if not (1 <= n <= ROLLOUT_MAX_N and 1 <= m <= REWARDS_MAX_L):
        raise ValueError(f"rollout_advantage: need 1 <= n <= {ROLLOUT_MAX_N} and 1 <= m <= {REWARDS_MAX_L}")
    rows = toks.shape[0] if toks.dim() == 2 else 0
    if rows < 1 or rows % n:
        raise ValueError("rollout_advantage: toks must hold n consecutive rows per clip")
    B = rows // n
    ldt = _rows2d(toks, torch.int64, rows, m + 1, "rollout_advantage: toks")
    lds = _rows2d(scores, torch.float64, rows, m, "rollout_advantage: scores")
    if baseline == BASELINE_GIVEN and (base is None or base.dtype != torch.float64 or base.numel() != B or not base.is_contiguous()):
        raise ValueError(f"rollout_advantage: BASELINE_GIVEN needs a contiguous ({B},) fp64 base")
    dev = toks.device
    if out is None:
        out = (torch.empty(rows, dtype=torch.int32, device=dev), torch.empty(rows, dtype=torch.float64, device=dev),
               torch.empty(rows, dtype=torch.float64, device=dev), torch.empty(rows, m, device=dev),
               torch.empty(4, dtype=torch.float64, device=dev))
    ln, reward, adv, weight, stats = out
    ldw = _rows2d(weight, torch.float32, rows, m, "rollout_advantage: weight")
    for t, dt, k in ((ln, torch.int32, rows), (reward, torch.float64, rows), (adv, torch.float64, rows), (stats, torch.float64, 4)):
        if t.dtype != dt or t.numel() != k or not t.is_contiguous() or t.device != dev:
            raise ValueError("rollout_advantage: len / reward / adv / stats must be contiguous int32 / fp64 tensors on toks' device")
    _launch("bmhrl_rollout_advantage", toks, ldt, B, n, m, int(end_idx), scores, lds, baseline, base, ln, reward, adv, weight, ldw,
            stats)
    return ln, reward, adv, weight[:, :m], stats


def policy_loss_fwd(logp, ld, action, weight, logq, clip, ent_weight, row_loss, row_entropy, rows, V):
    """row_loss / row_entropy (rows,) fp32 of bmhrl_policy_loss_fwd: logp (rows, V) fp32 with row stride ld, action (rows,)
    int64, weight (rows,) fp32, logq (rows,) fp32 with clip > 0 (both or neither), ent_weight (rows,) fp32 or None"""
    _launch("bmhrl_policy_loss_fwd", logp, ld, action, weight, logq, float(clip), ent_weight, row_loss, row_entropy, rows, V)


def policy_loss_bwd(logp, ld, action, weight, logq, clip, ent_weight, gscale, drow, dlogp, ldg, rows, V):
    """the dense gradient dlogp (rows, V) fp32 with row stride ldg of bmhrl_policy_loss_bwd, times gscale[0] * drow[row]"""
    _launch("bmhrl_policy_loss_bwd", logp, ld, action, weight, logq, float(clip), ent_weight, gscale, drow, dlogp, ldg, rows, V)
