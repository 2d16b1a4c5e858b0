"""CPU checks of tests/attention_reference.py: that its bounds mean something before tests/test_attention_paths_gpu.py relies on
them.  A correct emulation of the kernels' documented roundings stays within HALF of the bound at every element of every
table case; the backward reference agrees with float64 autograd; deliberately wrong emulations -- the mistakes such kernels
make -- each break the bound on a named table case; and the statistics tolerance is derived from plain fp32 here."""
import functools

import pytest
import torch

from . import attention_reference as ar


def _fwd_key(form, c):
    return (form, c["B"], c["H"], c["Sq"], c["Sk"], c["mask"], c["dtype"])


def _unique(form, table):
    seen, out = set(), []
    for c in table:
        k = _fwd_key(form, c)
        if k not in seen:
            seen.add(k)
            out.append(pytest.param(k, id=f"{form}-{c['name']}"))
    return out


def _case(form, table, name):
    return _fwd_key(form, next(c for c in table if c["name"] == name))


FWD_KEYS = _unique("split", ar.FWD256) + _unique("shared", ar.FWD128)


@pytest.mark.parametrize("key", FWD_KEYS)
def test_forward_emulation_within_half_the_bound(key):
    inp, ref = ar.make_inputs(*key), ar.reference(*key)
    K, V = ar.kv_of(inp)
    emu = ar.emulate_forward(inp["Q"], K, V, inp["mask"], inp["scale"], key[-1])
    ok, worst, at = ar.within(emu, ref["O"], ref["bound"], 0.5)
    assert ok, (worst, at)
    assert bool((ref["bound"] > 0).all())


@pytest.mark.parametrize("c", ar.BWD128, ids=ar.case_id)
def test_backward_emulation_within_half_the_bound(c):
    key = _fwd_key("shared", c) + (True,)
    inp, ref = ar.make_inputs(*key), ar.reference(*key)
    dQ, dX = ar.emulate_backward(inp["Q"], inp["K0"][:, :, 0], inp["dCx"], inp["mask"], inp["scale"], c["dtype"])
    for out, name in ((dQ, "dQ"), (dX, "dX")):
        ok, worst, at = ar.within(out, ref[name], ref["bound_" + name], 0.5)
        assert ok, (name, worst, at)
    # the exact "pair" rows carry a gradient that is far from trivial
    assert float(ref["dQ"].abs().max()) >= 1.0 or c["Sk"] == 1


@pytest.mark.parametrize("name", ["n-sk129", "n-sk300", "n-tile"])
def test_backward_reference_matches_float64_autograd(name):
    c = next(c for c in ar.BWD128 if c["name"] == name)
    key = _fwd_key("shared", c) + (True,)
    inp, ref = ar.make_inputs(*key), ar.reference(*key)
    q = inp["Q"].clone().requires_grad_(True)
    x = inp["K0"][:, :, 0].clone().requires_grad_(True)
    s = torch.einsum("bqhd,bkd->bhqk", q, x) * inp["scale"]
    if inp["mask"] is not None:
        s = s.masked_fill(inp["mask"][:, None, None, :] == 0, -1e9)
    ctx = torch.einsum("bhqk,bkd->bqhd", torch.softmax(s, -1), x)
    assert float((ctx.detach() - ref["O"]).abs().max()) <= 1e-12 * float(ref["O"].abs().max())
    ctx.backward(inp["dCx"])
    for got, want in ((ref["dQ"], q.grad), (ref["dX"], x.grad)):
        assert float((got - want).abs().max()) <= 1e-12 * float(want.abs().max())


# ---- mutation checks: each wrong emulation must leave the bound on the named case
def _mutated(key, mutate=None, mask=None, signature_everywhere=False):
    inp, ref = ar.make_inputs(*key), ar.reference(*key)
    K, V = (inp["Kc"], inp["Vc"] if inp["form"] == "split" else inp["Kc"]) if signature_everywhere else ar.kv_of(inp)
    emu = ar.emulate_forward(inp["Q"], K, V, inp["mask"] if mask is None else mask, inp["scale"], key[-1], mutate)
    return emu, ref, inp


def _broken(emu, ref):
    ok, worst, _ = ar.within(emu, ref["O"], ref["bound"])
    return not ok


def test_the_unmutated_emulation_passes_where_the_mutations_fail():
    for key in (_case("split", ar.FWD256, "22-sk65"), _case("shared", ar.FWD128, "22-sk65")):
        emu, ref, _ = _mutated(key)
        assert not _broken(emu, ref)


def test_mutation_last_key_of_a_ragged_tile_dropped():
    key = _case("split", ar.FWD256, "22-sk65")           # Sk = 65: the last key is alone in its tile

    def drop(e, s, keep):
        e = e.clone()
        e[..., -1] = 0
        return e
    emu, ref, _ = _mutated(key, drop)
    assert _broken(emu, ref)


def test_mutation_last_key_counted_twice():
    key = _case("split", ar.FWD256, "22-sk65")           # (the clamped re-read of a ragged tile treated as a valid key)

    def twice(e, s, keep):
        e = e.clone()
        e[..., -1] *= 2
        return e
    emu, ref, _ = _mutated(key, twice)
    assert _broken(emu, ref)


def test_mutation_one_masked_key_let_through():
    key = _case("split", ar.FWD256, "22-sk33")           # tail mask in batch row 0
    inp = ar.make_inputs(*key)
    mask = inp["mask"].clone()
    first_masked = int(torch.nonzero(mask[0] == 0)[0])
    mask[0, first_masked] = 1
    emu, ref, _ = _mutated(key, mask=mask, signature_everywhere=True)
    assert _broken(emu, ref)


def test_mutation_masked_tile_between_valid_tiles_ends_the_row():
    key = _case("split", ar.FWD256, "22-sk129")          # tile_b0: keys 32 .. 63 of batch row 0 masked, 64 .. 96 valid

    def stop(e, s, keep):
        e = e.clone()
        e[0, :, :, 32:] = 0
        return e
    emu, ref, _ = _mutated(key, stop)
    assert _broken(emu, ref)


def test_mutation_fully_masked_row_gives_zero():
    key = _case("split", ar.FWD256, "22-sk255")          # fullrow: the last batch row is fully masked
    emu, ref, _ = _mutated(key)
    emu = emu.clone()
    emu[-1] = 0
    assert _broken(emu, ref)


def test_mutation_rescale_skipped_after_a_jump():
    key = _case("split", ar.FWD256, "22-sk257")          # staircase rows: the maximum jumps by 16 nats (> 8 ln 2) per tile

    def skip(e, s, keep):
        # what lies before the key of the row maximum stays at the old maximum: O and the sum are not scaled down
        top = s.argmax(-1, keepdim=True)
        before = torch.arange(s.shape[-1])[None, None, None, :] < top
        m_old = s.masked_fill(~before, -float("inf")).max(-1, keepdim=True).values
        m_new = s.max(-1, keepdim=True).values
        jump = (m_new - m_old) > ar.LAG_MAX
        return torch.where(before & jump, torch.exp(s - m_old), e)
    emu, ref, _ = _mutated(key, skip)
    assert _broken(emu, ref)


def test_mutation_rows_past_sq_stored():
    """a ragged query tile stores one row more than Sq (the clamped last row): it lands in row 0 of the next batch row, or,
    behind the last batch row, in the guard row -- the GPU test's two checks (bound, sentinel)"""
    key = _case("split", ar.FWD256, "22-sk33")           # B = 3, Sq = 33
    emu, ref, _ = _mutated(key)
    B, Sq = key[1], key[3]
    sent = -776.0
    buf = torch.full((B * Sq + 1,) + tuple(emu.shape[2:]), sent, dtype=emu.dtype)
    buf[:B * Sq] = emu.reshape((B * Sq,) + tuple(emu.shape[2:]))
    for b in range(B):
        buf[(b + 1) * Sq] = emu[b, Sq - 1]
    assert bool((buf[B * Sq] != sent).any())                                        # the sentinel check
    assert _broken(buf[:B * Sq].reshape(emu.shape), ref)                            # the bound, in the next batch row


def test_mutation_heads_swapped_in_the_shared_form():
    key = _case("shared", ar.FWD128, "22-sk65")          # H = 4
    emu, ref, _ = _mutated(key)
    assert _broken(emu[:, :, [1, 0, 3, 2]], ref)


def _bwd(name, **kw):
    c = next(c for c in ar.BWD128 if c["name"] == name)
    key = _fwd_key("shared", c) + (True,)
    inp, ref = ar.make_inputs(*key), ar.reference(*key)
    dQ, dX = ar.emulate_backward(inp["Q"], inp["K0"][:, :, 0], inp["dCx"], inp["mask"], inp["scale"], c["dtype"], **kw)
    return dQ, dX, ref


def test_mutation_ds_not_zeroed_in_a_fully_masked_row():
    def leak(dS, P, dP, delta, keep):
        return P * (dP - delta[..., None]) / 16           # (scale = 1 / 16) without the masked_fill
    dQ, dX, ref = _bwd("n-sk129", mutate_ds=leak)         # fullrow: the last sample is fully masked
    assert not ar.within(dQ, ref["dQ"], ref["bound_dQ"])[0]
    assert bool((ref["dQ"][-1] == 0).all()) and bool((dQ[-1] != 0).any())
    good = _bwd("n-sk129")
    assert ar.within(good[0], ref["dQ"], ref["bound_dQ"])[0] and bool((good[0][-1] == 0).all())


def test_mutation_delta_from_the_wrong_head():
    dQ, dX, ref = _bwd("n-sk300", delta_perm=[1, 0, 3, 2])
    assert not ar.within(dQ, ref["dQ"], ref["bound_dQ"])[0]
    assert not ar.within(dX, ref["dX"], ref["bound_dX"])[0]


# ---- statistics
def test_statistics_tolerance():
    """lse in plain torch fp32 on the table's inputs: its largest deviation from float64 is what LSE_FP32_DEV records, and the
    GPU tolerance is 8 times that, never above the 2e-3 of the older tests"""
    worst = 0.0
    for key in [p.values[0] for p in FWD_KEYS]:
        form, B, H, Sq, Sk = key[:5]
        if B * H * Sq * Sk > 4_000_000:
            continue
        inp, ref = ar.make_inputs(*key), ar.reference(*key)
        K, _ = ar.kv_of(inp)
        s32 = torch.einsum("bqhd,bhkd->bhqk", inp["Q"].float(), ar._kv(K, H).float()) * torch.tensor(inp["scale"], dtype=torch.float32)
        s32 = s32.masked_fill(~ref["keep"], -1e9)
        lse32 = torch.logsumexp(s32, -1).double()
        live = ref["lse"] > -1e8
        if live.any():
            worst = max(worst, float((lse32 - ref["lse"])[live].abs().max()))
    print(f"largest fp32 deviation of lse: {worst:.3e}")
    assert 0.25 * ar.LSE_FP32_DEV <= worst <= ar.LSE_FP32_DEV
    assert ar.LSE_TOL == 8 * ar.LSE_FP32_DEV and ar.LSE_TOL <= 2e-3


# ---- the plan query is a pure host function
def test_attention_plan_reports_the_dispatch():
    from bmhrl_amd import _lib, ops
    lib = _lib.load()
    try:
        assert ops.attention_plan("256-fwd", 2, 4, 64, 64) == 22
        assert ops.attention_plan("256-fwd", 16, 4, 800, 256) == 256         # 256 workgroups of 256 rows: two-phase
        assert ops.attention_plan("256-fwd", 16, 4, 800, 256, 256) == 41     # per-query mask: the generic kernel, 448 workgroups
        assert ops.attention_plan("256-fwd", 16, 4, 800, 800) == 41
        assert ops.attention_plan("256-fwd", 1, 1, 32, 10112) == 22 and ops.attention_plan("256-fwd", 1, 1, 32, 10113) < 0
        for code in (22, 41):
            lib.bmhrl_attention_config(256, code)
            assert ops.attention_plan("256-fwd", 16, 4, 800, 256) == code
        lib.bmhrl_attention_config(256, 256)
        assert ops.attention_plan("256-fwd", 2, 4, 64, 64) == 256 and ops.attention_plan("256-fwd", 2, 4, 64, 300) == 22
        lib.bmhrl_attention_config(256, 33)
        assert ops.attention_plan("256-fwd", 2, 4, 64, 64) < 0
        lib.bmhrl_attention_config(256, 0)
        assert ops.attention_plan("128-fwd", 16, 4, 800, 800) == 41 and ops.attention_plan("128-fwd", 16, 4, 256, 800) == 22
        assert ops.attention_plan("128-fwd", 2, 2, 64, 64, 64) < 0           # the shared form takes key masks only
        for code in (22, 41, 24, 14):
            lib.bmhrl_attention_config(128, code)
            assert ops.attention_plan("128-fwd", 2, 4, 64, 64) == code
        assert ops.attention_plan("128-fwd", 2, 3, 64, 64) < 0               # a pinned 14 with an odd head count is an error
        lib.bmhrl_attention_config(128, 0)
        assert ops.attention_plan("128-bwd", 16, 4, 800, 800) == 41 and ops.attention_plan("128-bwd", 16, 4, 256, 800) == 22
        assert ops.attention_plan("128-bwd", 16, 4, 767, 33) == 41 and ops.attention_plan("128-bwd", 16, 4, 736, 33) == 22
        assert ops.attention_plan("128-bwd", 0, 4, 64, 64) < 0 and ops.attention_plan("128-bwd", 1, 1, 32, 10113) < 0
    finally:
        lib.bmhrl_attention_config(256, 0)
        lib.bmhrl_attention_config(128, 0)
