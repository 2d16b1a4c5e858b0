"""CPU checks of the one call path from bmhrl_amd.ops into the HIP library: ops._launch / ops._query over the tables of
bmhrl_amd._lib, and ops._ptr / ops._at for every address.  The library is replaced by a recording stand-in, so nothing here
needs a GPU and only the last test needs nothing at all but the source file."""
import ast
import ctypes as C
import os

import pytest
import torch

from bmhrl_amd import _lib, ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STREAM = 0x5EED
NO_CPU = "no CPU fallback"


class Recorder:
    """stands in for the loaded library: every attribute is a function that records (name, args) and returns `rc`"""

    def __init__(self, rc=0):
        self.calls, self.rc = [], rc

    def __getattr__(self, name):
        def fn(*args):
            self.calls.append((name, args))
            return self.rc
        return fn


@pytest.fixture
def rec(monkeypatch):
    r = Recorder()
    monkeypatch.setattr(_lib, "load", lambda: r)
    monkeypatch.setattr(ops, "stream", lambda: STREAM)
    return r


def cpu(n=4, dtype=torch.float32):
    return torch.zeros(n, dtype=dtype)


def plain_args(name):
    """arguments of a launching entry without its stream: an int in every pointer slot (a zeroed descriptor by reference
    where the entry takes descriptors), 1 in an int slot, 0.5 in a float slot"""
    out = []
    for i, t in enumerate(_lib.PROTOTYPES[name][:-1]):
        if t is C.POINTER(_lib.GemmDesc):
            out.append(C.byref(_lib.GemmDesc()))
        elif i in _lib.PTR_SLOTS[name]:
            out.append(4096 + 64 * i)
        else:
            out.append(0.5 if t in (_lib.f32, _lib.f64) else 1)
    return out


ENTRIES = sorted(_lib.PROTOTYPES)


def test_pointer_slots_are_derived_from_the_tables():
    assert _lib.PTR_SLOTS["bmhrl_gemm"] == (0, 1) and _lib.PTR_SLOTS["bmhrl_gemm_plan"] == (0, 1)
    assert _lib.PTR_SLOTS["bmhrl_log_softmax"] == (0, 4) and _lib.PTR_SLOTS["bmhrl_gemm_splits"] == ()
    assert _lib.PTR_SLOTS["bmhrl_rnn_step"] == (1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 15)
    assert set(_lib.PTR_SLOTS) == set(_lib.PROTOTYPES) | set(_lib.QUERIES)
    for name, argtypes in [*_lib.PROTOTYPES.items(), *((n, q[1]) for n, q in _lib.QUERIES.items())]:
        for i, t in enumerate(argtypes):
            assert (i in _lib.PTR_SLOTS[name]) == (t is C.c_void_p or issubclass(t, C._Pointer)), (name, i)


@pytest.mark.parametrize("name", ENTRIES)
def test_every_launching_entry_refuses_cpu_memory_before_the_call(rec, name):
    slots = _lib.PTR_SLOTS[name][:-1]
    assert slots, name
    for i in slots:
        args = plain_args(name)
        args[i] = cpu()
        with pytest.raises(RuntimeError, match=NO_CPU):
            ops._launch(name, *args)
        args[i] = torch.nn.Parameter(cpu())
        with pytest.raises(RuntimeError, match=NO_CPU):
            ops._launch(name, *args)
    assert rec.calls == []


@pytest.mark.parametrize("name", ENTRIES)
def test_the_pass_through_is_exact(rec, name):
    args = plain_args(name)
    ops._launch(name, *args)
    assert rec.calls == [(name, (*args, STREAM))]
    assert all(type(got) is type(given) for got, given in zip(rec.calls[0][1], args))
    rec.calls.clear()
    for i in _lib.PTR_SLOTS[name][:-1]:
        args[i] = None
    ops._launch(name, *args)
    assert rec.calls == [(name, (*args, STREAM))]
    assert all(rec.calls[0][1][i] is None for i in _lib.PTR_SLOTS[name][:-1])


@pytest.mark.parametrize("name", ENTRIES)
def test_arity_and_position_are_enforced(rec, name):
    args = plain_args(name)
    with pytest.raises(TypeError, match=name):
        ops._launch(name, *args[:-1])
    with pytest.raises(TypeError, match=name):
        ops._launch(name, *args, 1)
    for i in range(len(args)):
        if i in _lib.PTR_SLOTS[name]:
            continue
        for stray in (cpu(1), torch.nn.Parameter(cpu(1))):      # (one element: float() and int() would take it)
            bad = list(args)
            bad[i] = stray
            with pytest.raises(TypeError, match=rf"{name}: argument {i} "):
                ops._launch(name, *bad)
    assert rec.calls == []


def test_an_unknown_entry_and_a_query_are_no_launches(rec):
    with pytest.raises(KeyError):
        ops._launch("bmhrl_no_such_entry", 1)
    with pytest.raises(KeyError):
        ops._launch("bmhrl_gemm_splits", 1, 1, 1, 1)
    with pytest.raises(KeyError):
        ops._query("bmhrl_log_softmax", 1, 1, 1, 1)
    assert rec.calls == []


def test_a_refusal_by_the_library_keeps_its_message(monkeypatch):
    for rc, text in ((-22, "bmhrl_log_softmax failed: invalid argument -22"), (700, "bmhrl_log_softmax failed: hipError_t 700")):
        r = Recorder(rc)
        monkeypatch.setattr(_lib, "load", lambda r=r: r)
        monkeypatch.setattr(ops, "stream", lambda: STREAM)
        with pytest.raises(_lib.HipError, match=f"^{text}$"):
            ops._launch("bmhrl_log_softmax", 4096, 8, 2, 8)
        assert r.calls == [("bmhrl_log_softmax", (4096, 8, 2, 8, STREAM))]


def test_query_passes_through_returns_the_value_and_checks_a_negative_int(monkeypatch):
    r = Recorder(3)
    monkeypatch.setattr(_lib, "load", lambda: r)
    monkeypatch.setattr(ops, "stream", lambda: pytest.fail("a query takes no stream"))
    assert ops._query("bmhrl_gemm_splits", 8, 8, 64, 1) == 3 and r.calls == [("bmhrl_gemm_splits", (8, 8, 64, 1))]
    d = C.byref(_lib.GemmDesc())
    assert ops._query("bmhrl_gemm_f32_fast_path", d) == 3 and r.calls[-1] == ("bmhrl_gemm_f32_fast_path", (d,))
    n = len(r.calls)
    for bad in ((8, 8, 64), (8, 8, 64, 1, 1)):
        with pytest.raises(TypeError, match="bmhrl_gemm_splits"):
            ops._query("bmhrl_gemm_splits", *bad)
    with pytest.raises(TypeError, match="bmhrl_gemm_splits: argument 2 "):
        ops._query("bmhrl_gemm_splits", 8, 8, cpu(1), 1)
    with pytest.raises(TypeError, match="bmhrl_gemm_f32_fast_path: argument 0 "):
        ops._query("bmhrl_gemm_f32_fast_path", cpu())
    assert len(r.calls) == n
    r.rc = -22
    with pytest.raises(_lib.HipError, match="^bmhrl_gemm_group_plan failed: invalid argument -22$"):
        ops._query("bmhrl_gemm_group_plan", d, 1)
    assert ops._query("bmhrl_attention_plan", 0, 1, 1, 32, 32, 0, refusal=False) == -22       # (a value there, not a refusal)
    assert ops.attention_plan("256-fwd", 1, 1, 32, 32) == -22
    r.rc = -1
    assert ops._query("bmhrl_layernorm_bwd_workspace", 4, 8) == -1                              # int64: a size, never checked


def test_splits_and_overwrites_share_one_cached_query(rec, monkeypatch):
    monkeypatch.setattr(ops, "_SPLITS", {})
    rec.rc = 1
    assert ops.gemm_overwrites(8, 16, 64) is True and ops.gemm_splits(8, 16, 64) == 1 and ops.gemm_splits(8, 16, 64, 1) == 1
    rec.rc = 4
    assert ops.gemm_splits(8, 16, 64, 2) == 4 and ops.gemm_overwrites(8, 16, 64, 2) is False
    assert rec.calls == [("bmhrl_gemm_splits", (8, 16, 64, 1)), ("bmhrl_gemm_splits", (8, 16, 64, 2))]
    rec.rc = -22
    for _ in range(2):                                          # a refusal is raised every time, not remembered as a value
        with pytest.raises(RuntimeError, match=r"bmhrl_gemm_splits\(0, 16, 64, 1\) failed: -22"):
            ops.gemm_splits(0, 16, 64)
    assert len(rec.calls) == 4


# ---- the wrappers that checked no tensor (or, for gemm, only A / B / C) before: public functions, CPU tensors
def _f(*shape):
    return torch.zeros(*shape)


def _b(*shape):
    return torch.zeros(*shape, dtype=torch.bfloat16)


def _i(*shape, dtype=torch.int64):
    return torch.zeros(*shape, dtype=dtype)


R, D, V = 2, 8, 8       # rows, width, vocabulary of the smallest plausible calls

UNCHECKED = {
    "softmax_rows": lambda: ops.softmax_rows(_f(R, D), D, _b(R, D), D, R, D),
    "attn_delta": lambda: ops.attn_delta(_b(R, D), D, _b(R, D), D, _f(R), 1, 1, R, D),
    "layernorm_bwd": lambda: ops.layernorm_bwd(_f(R, D), _f(R, D), _f(D), _f(R), _f(R), _f(R, D), None, _f(D), _f(D), R, D,
                                               workspace=_f(64)),
    "embed_bwd": lambda: ops.embed_bwd(_i(1, R), None, 0.0, _f(R, D), _f(V, D), 1, R, D, 1.0),
    "colsum_bf16": lambda: ops.colsum_bf16(_b(R, D), D, _f(D), False, R, D),
    "colsum_bf16_groups": lambda: ops.colsum_bf16_groups(_b(2 * R, D), D, _f(2, D), R, D, 2, D),
    "gate_fwd": lambda: ops.gate_fwd(_f(R, D), _f(R, D), _f(D), _f(R, D), None, 0, R, D),
    "gate_bwd": lambda: ops.gate_bwd(_f(R, D), _f(R, D), _f(R, D), _f(D), _f(R, D), _f(R, D), _f(D), R, D),
    "expand_goals_index": lambda: ops.expand_goals_index(_i(1, R, dtype=torch.int32), _i(R, dtype=torch.int32), 1, R),
    "gather_rows": lambda: ops.gather_rows(_f(R, D), _i(R, dtype=torch.int32), _f(R, D), None, 0, R, D),
    "scatter_add_rows": lambda: ops.scatter_add_rows(_f(R, D), _i(R, dtype=torch.int32), _f(R, D), R, D),
    "log_softmax_": lambda: ops.log_softmax_(_f(R, V), V, R, V),
    "smooth_kl_fwd": lambda: ops.smooth_kl_fwd(_f(R, V), V, _i(R), None, None, None, 0.1, 1, 0, _f(R), None, R, V),
    "smooth_kl_bwd": lambda: ops.smooth_kl_bwd(_f(R, V), V, _i(R), None, None, None, 0.1, 1, 0, _f(1), _b(R, V), V, None, R, V),
    "smooth_kl_amp_grad": lambda: ops.smooth_kl_amp_grad(_f(R, V), V, _i(R), _i(R), _f(R), _f(R), 0.1, 1, 0, _f(R), R, V),
    "log_softmax_bwd": lambda: ops.log_softmax_bwd(_f(R, V), _f(R, V), V, _b(R, V), V, R, V),
    "sample_tokens": lambda: ops.sample_tokens(_f(R, V), V, _i(R), _f(R), R, V, True, 0),
    "reinforce_bwd": lambda: ops.reinforce_bwd(_f(R, V), V, _i(R), _f(R), _f(R), _f(1), _f(R, V), _f(R), _f(R), R, V),
    "rnn_step": lambda: ops.rnn_step(3, _f(R, 3 * D), _f(3 * D, D), _f(3 * D), None, None, _f(R, D), None, _f(R, D), None, None,
                                     R, 1, D, 0),
    "rnn_wavefront": lambda: ops.rnn_wavefront([dict(w_ih=_f(3 * D, D), w_hh=_f(3 * D, D), b_ih=_f(3 * D), b_hh=_f(3 * D),
                                                     in_seq=_f(R, D), in_ld=D, in_dim=D, gates=3, seq_out=_f(R, D),
                                                     h=(_f(R, D), _f(R, D)))], R, 1, D),
    "critic_head": lambda: ops.critic_head(_f(R, D), _f(1, D), _f(1), 0.5, _f(R), None, R, D),
    # the struct filler alone: no tensor but those of the group table
    "fusion_tail_fwd": lambda: ops.fusion_tail_fwd(None, None, [(_f(D), _f(D), _f(D), _f(D), _f(D))], R, D, None, None),
}


@pytest.mark.parametrize("wrapper", sorted(UNCHECKED))
def test_wrappers_that_checked_nothing_refuse_cpu_tensors(rec, wrapper):
    with pytest.raises(RuntimeError, match=NO_CPU):
        UNCHECKED[wrapper]()
    assert rec.calls == []


@pytest.mark.parametrize("which", ["last_direct_argument", "group_gradient"])
def test_a_cpu_tensor_behind_good_ones_is_refused_too(rec, monkeypatch, which):
    """(the cases above stop at their first tensor) every tensor but one is taken for device memory here"""
    real, good = ops._ptr, []
    monkeypatch.setattr(ops, "_ptr", lambda t: 4096 if any(t is g for g in good) else real(t))
    if which == "last_direct_argument":
        good += [_f(R, D), _f(R, D), _f(D), _f(R, D)]
        with pytest.raises(RuntimeError, match=NO_CPU):
            ops.gate_fwd(*good, _b(R, D), D, R, D)
    else:
        good += [_f(R, D) for _ in range(6)] + [_f(D) for _ in range(5)]
        with pytest.raises(RuntimeError, match=NO_CPU):
            ops.fusion_tail_bwd(good[0], good[1], good[2], good[3], [tuple(good[6:])], [(None, None, None, None, _f(D))], R, D,
                                good[4], good[5])
    assert rec.calls == []


GEMM_OPERANDS = {"bias": _f(D), "residual": _f(R, D), "mask": _i(R, D, dtype=torch.uint8), "rowvec": _f(R), "aux": _b(R, D),
                 "colsum": _f(D), "seed_dev": _i(1), "split_ws": _f(64)}


@pytest.mark.parametrize("operand", sorted(GEMM_OPERANDS))
def test_gemm_refuses_every_cpu_operand(rec, monkeypatch, operand):
    A, B, Cf = _b(R, D), _b(D, D), _f(R, D)
    real = ops._ptr
    monkeypatch.setattr(ops, "_ptr", lambda t: 4096 if t is A or t is B or t is Cf else real(t))
    kw = dict(lda=D, ldb=D, C_f32=Cf, ldc=D)
    ops.gemm(A, B, R, D, D, **kw)                               # the three stand for device tensors: this one goes through
    assert [c[0] for c in rec.calls] == ["bmhrl_gemm"] and rec.calls[0][1][1] == STREAM
    rec.calls.clear()
    deferred = []
    for how in (dict(), dict(defer=deferred)):
        with pytest.raises(RuntimeError, match=NO_CPU):
            ops.gemm(A, B, R, D, D, **kw, **how, **{operand: GEMM_OPERANDS[operand]})
    with pytest.raises(RuntimeError, match=NO_CPU):
        ops.gemm_desc(A, B, R, D, D, **kw, **{operand: GEMM_OPERANDS[operand]})
    assert rec.calls == [] and deferred == []


def test_gemm_builds_what_gemm_desc_builds_and_keeps_the_operands_alive(rec, monkeypatch):
    A, B, Cb, bias, res = _b(R, D), _b(D, D), _b(R, D), _f(D), _f(R, D)
    addr = {id(t): 4096 * (k + 1) for k, t in enumerate((A, B, Cb, bias, res))}
    monkeypatch.setattr(ops, "_ptr", lambda t: None if t is None else addr[id(t)])
    monkeypatch.setattr(ops, "_GROUP_LEAVES", True)
    kw = dict(lda=D, ldb=D, a_off=3, b_trans=True, C_bf16=Cb, ldcb=D, cb_off=5, bias=bias, residual=res, ldr=D, relu=True, alpha=0.5)
    want = ops.gemm_desc(A, B, R, D, D, **kw)
    assert (want.A, want.B, want.Cb, want.C, want.bias, want.residual) == (4096 + 3 * 2, 8192, 3 * 4096 + 5 * 2, None, 4 * 4096,
                                                                          5 * 4096)
    deferred = []
    ops.gemm(A, B, R, D, D, defer=deferred, **kw)
    assert rec.calls == [] and len(deferred) == 1
    d, alive = deferred[0]
    assert bytes(d) == bytes(want)
    assert [id(t) for t in alive if t is not None] == [id(t) for t in (A, B, Cb, bias, res)] and len(alive) == 12
    ops.gemm_flush(deferred)
    assert [c[0] for c in rec.calls] == ["bmhrl_gemm_group"] and rec.calls[0][1][1:] == (1, STREAM) and deferred == []
    with pytest.raises(TypeError):
        ops.gemm(A, B, R, D, D, lda=D, ldb=D, no_such_keyword=1)


def test_at_scales_by_the_element_size(monkeypatch):
    monkeypatch.setattr(ops, "_ptr", lambda t: None if t is None else 1 << 20)
    for dtype, size in ((torch.bfloat16, 2), (torch.float16, 2), (torch.float32, 4), (torch.int64, 8), (torch.uint8, 1)):
        t = torch.zeros(8, dtype=dtype)
        assert ops._at(t, 3) == (1 << 20) + 3 * size and ops._at(t, 0) == 1 << 20
    assert ops._at(None, 3) is None and ops._at(None, 0) is None


def test_an_empty_tensor_is_the_null_pointer(rec):
    """(a zero-size workspace is written torch.empty(0) by callers: no memory, so nothing a kernel could touch)"""
    assert ops._ptr(torch.empty(0)) == 0 and ops._at(torch.empty(0), 0) == 0
    ops._launch("bmhrl_log_softmax", torch.empty(0), 8, 0, 8)
    assert rec.calls == [("bmhrl_log_softmax", (0, 8, 0, 8, STREAM))]


# ---- the module keeps the property: a structural check of bmhrl_amd/ops.py itself
def _functions_of(node_type, pred):
    """names of the outermost functions of ops.py (or '<module>') that hold a node of node_type satisfying pred"""
    tree = ast.parse(open(os.path.join(ROOT, "bmhrl_amd", "ops.py")).read())
    found = set()
    for top in tree.body:
        where = top.name if isinstance(top, (ast.FunctionDef, ast.ClassDef)) else "<module>"
        found |= {where for n in ast.walk(top) if isinstance(n, node_type) and pred(n)}
    return found


def test_ops_takes_every_address_and_makes_every_call_in_one_place():
    assert _functions_of(ast.Attribute, lambda n: n.attr == "data_ptr") <= {"_ptr", "_at"}
    assert _functions_of(ast.Attribute, lambda n: n.attr.startswith("bmhrl_")) == set()
    assert _functions_of(ast.Call, lambda n: isinstance(n.func, ast.Name) and n.func.id == "getattr") == {"_launch", "_query"}
    assert _functions_of(ast.Attribute, lambda n: n.attr == "load") == {"_launch", "_query"}
    assert not hasattr(ops, "_need_cuda") and not hasattr(ops, "_p")
