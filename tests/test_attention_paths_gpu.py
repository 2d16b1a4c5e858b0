"""Every fused attention forward and backward kernel against the float64 reference of tests/attention_reference.py, element by
element within the bounds stated there (no global normalisation), on tables of small cases that reach every kernel the
host dispatch can choose: head dimension 256 codes 22 / 41 / 256 (two-phase, every tile count), head dimension 128 codes 22 /
41 / 24 / 14, and the shared form's backward with the narrow and the wide dQp kernel.  bmhrl_attention_plan tells which
kernel a case takes; test_paths_covered asserts that the tables reach all of them.

Every case: operands inside larger NaN-filled buffers (NaN columns beside them, NaN guard rows around them, mask bytes
of 1 around the mask), outputs as views into sentinel-filled buffers (every sentinel must survive, every written element
must be finite), finite garbage at masked keys (a second run with zeros there must be bit-identical).
"""
# Statistics tolerance.  lse = row_max + log(row_sum) evaluated in plain torch fp32 on the inputs of every table case deviates
# from float64 by at most 1.6e-4 (tests/test_attention_reference_cpu.py::test_statistics_tolerance measures it: the scores of
# the staircase rows reach 128 nats, and an fp32 dot product of 256 terms of that size carries about that much).  The kernels
# are held to 8 times that, LSE_TOL = 1.28e-3 (hardware exp2 / log2, another summation order) -- below the 2e-3 the older
# tests use.  The maximum may lag: row_max in [max - 8 ln 2, max] for the online kernels, row_max = max for the two-phase one.
import pytest
import torch

from . import attention_reference as ar

pytestmark = pytest.mark.gpu

SENT = -776.0            # exactly representable in bf16, fp16 and fp32
GUARD = 3                # guard rows on either side of an operand / output
MGUARD = 16              # guard bytes on either side of a mask


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


def _sync():
    """a HIP error ends the session: nothing more is launched on a device that has faulted"""
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit(f"GPU error, no further launches: {e}", returncode=3)


def _place(parts, rows, ld, dtype, dev, fill):
    """a (rows + 2 GUARD, ld) buffer filled with `fill`; parts: [(col0, x (rows, cols) float64)].  Returns (buffer, views)"""
    buf = torch.full((rows + 2 * GUARD, ld), fill, dtype=dtype)
    for col0, x in parts:
        buf[GUARD:GUARD + rows, col0:col0 + x.shape[1]] = x.to(dtype)
    buf = buf.to(dev)
    return buf, [buf[GUARD:, col0:] for col0, _ in parts]


def _out(rows, cols, ld, dtype, dev):
    buf = torch.full((rows + 2 * GUARD, ld), SENT, dtype=dtype, device=dev)
    return buf, buf[GUARD:, :]


def _stats(n, dev):
    buf = torch.full((n + 128,), SENT, device=dev)
    return buf, buf[64:64 + n]


def _mask(mask, off, dev):
    """mask bytes inside a buffer of ones, the view `off` bytes past a 16-byte boundary (odd: unaligned rows)"""
    if mask is None:
        return None, None
    n = mask.numel()
    buf = torch.ones(n + 2 * MGUARD + 16, dtype=torch.uint8)
    buf[MGUARD + off:MGUARD + off + n] = mask.flatten()
    buf = buf.to(dev)
    view = buf[MGUARD + off:MGUARD + off + n]
    if view.data_ptr() % 16 != (MGUARD + off) % 16:          # (torch allocations are at least 16-byte aligned)
        raise RuntimeError("unexpected allocation alignment")
    return buf, view


def _check_sentinels(buf, rows, cols, what):
    """everything outside [GUARD, GUARD + rows) x [0, cols) still holds the sentinel, everything inside is finite"""
    b = buf.float().cpu()
    inside = torch.zeros_like(b, dtype=torch.bool)
    inside[GUARD:GUARD + rows, :cols] = True
    assert bool((b[~inside] == SENT).all()), f"{what}: a sentinel beside or around the output was overwritten"
    assert bool(torch.isfinite(b[inside]).all()), f"{what}: an output element is not finite (or was not written)"
    assert not bool((b[inside] == SENT).all()), f"{what}: nothing was written"


def _check_stat_sentinels(buf, n, what):
    b = buf.cpu()
    assert bool((b[:64] == SENT).all()) and bool((b[64 + n:] == SENT).all()), f"{what}: written outside its extent"
    assert bool(torch.isfinite(b[64:64 + n]).all()), f"{what}: not finite"


def _assert_within(out, ref, bound, what):
    ok, worst, at = ar.within(out, ref, bound)
    print(f"{what}: worst |err| / bound = {worst:.3f} at {tuple(int(i) for i in at)}")
    assert ok, f"{what}: |err| / bound = {worst:.3f} at {tuple(int(i) for i in at)}: got {float(out[at]):.6g}, reference {float(ref[at]):.6g}"


def _check_statistics(c, ref, rmax, rsum, Sk, two_phase):
    """lse, the lag of the maximum, fully masked rows; rmax / rsum (B, H, Sq) float64 on the CPU"""
    B, H, Sq = rmax.shape
    full = ref["full"].expand(B, H, Sq)
    live = ~full
    lse = rmax + torch.log(rsum)
    if live.any():
        dev_lse = float((lse - ref["lse"])[live].abs().max())
        lag = (ref["max"] - rmax)[live]
        print(f"{c['name']}: lse deviation {dev_lse:.2e} (tolerance {ar.LSE_TOL:.2e}), lag of the maximum in [{float(lag.min()):.3g}, {float(lag.max()):.3g}]")
        assert dev_lse <= ar.LSE_TOL
        # "to fp32": a score is an fp32 sum of up to 256 products, each addition rounding by up to 2^-24 of the partial sum;
        # independent roundings walk sqrt(256) = 16 of them far: 2^-20 of the largest score (and of 1 for the final scaling)
        eps = 2.0 ** -20 * float(ref["max"][live].abs().max() + 1.0)
        if two_phase:
            assert float(lag.abs().max()) <= eps
        else:
            assert float(lag.min()) >= -eps and float(lag.max()) <= ar.LAG_MAX + eps
    if full.any():          # the backward relies on both
        assert bool((rmax[full] == ar.NEG_MASK).all())
        assert float((rsum[full] - Sk).abs().max()) <= 1e-3 * Sk


def _pin(head_dim, code):
    from bmhrl_amd import _lib
    _lib.check(_lib.load().bmhrl_attention_config(head_dim, code), "bmhrl_attention_config")


def _mask_strides(mask, Sq, Sk):
    if mask is None:
        return 0, 0
    return (Sq * Sk, Sk) if mask.dim() == 3 else (Sk, 0)


# ------------------------------------------------------------------------------------------------- head dimension 256
def _plan256(c, msq):
    """the code the entry takes.  The fp16 entry has no two-phase kernel and no pin: it takes the automatic choice between 41
    and 22, which does not depend on Sk -- asked for at a key count the two-phase kernel does not serve."""
    from bmhrl_amd import ops
    if c["dtype"] == torch.float16:
        return ops.attention_plan("256-fwd", c["B"], c["H"], c["Sq"], max(c["Sk"], 257), msq)
    return ops.attention_plan("256-fwd", c["B"], c["H"], c["Sq"], c["Sk"], msq)


def _run256(c, inp, dev, clean, dropout_p=0.0, seed=0, seed_dev=None):
    from bmhrl_amd import ops
    B, H, Sq, Sk, dt = c["B"], c["H"], c["Sq"], c["Sk"], c["dtype"]
    dk, D = 256, H * 256
    K, V = ar.kv_of(inp, clean)
    q2, k2, v2 = inp["Q"].reshape(B * Sq, D), K.reshape(B * Sk, D), V.reshape(B * Sk, D)
    nan = float("nan")
    if c.get("packed") and Sq == Sk:                  # Q | K | V side by side in one buffer, as the self attention passes them
        ld = 3 * D + 8
        keepalive, (Qv, Kv, Vv) = _place([(0, q2), (D, k2), (2 * D, v2)], B * Sq, ld, dt, dev, nan)
        ldq = ldk = ldv = ld
    else:
        ldq, ldk, ldv = D + 8, D + 16, D + 24
        b1, (Qv,) = _place([(0, q2)], B * Sq, ldq, dt, dev, nan)
        b2, (Kv,) = _place([(8, k2)], B * Sk, ldk, dt, dev, nan)
        b3, (Vv,) = _place([(16, v2)], B * Sk, ldv, dt, dev, nan)
        keepalive = (b1, b2, b3)
    ldo = D + 16
    obuf, Ov = _out(B * Sq, D, ldo, dt, dev)
    mxbuf, mx = _stats(B * H * Sq, dev)
    smbuf, sm = _stats(B * H * Sq, dev)
    mbuf, mview = _mask(inp["mask"], c.get("mask_off", 0), dev)
    msb, msq = _mask_strides(inp["mask"], Sq, Sk)
    ops.attention_fwd(Qv, Kv, Vv, Ov, mx, sm, mview, msb, msq, B, H, Sq, Sk, dk, inp["scale"], ldq, ldk, ldv, ldo,
                      dropout_p=dropout_p, seed=seed, seed_dev=seed_dev)
    _sync()
    _check_sentinels(obuf, B * Sq, D, c["name"] + " O")
    _check_stat_sentinels(mxbuf, B * H * Sq, c["name"] + " row_max")
    _check_stat_sentinels(smbuf, B * H * Sq, c["name"] + " row_sum")
    if mbuf is not None:
        assert bool((mbuf.cpu()[:MGUARD] == 1).all())
    del keepalive
    O = obuf[GUARD:GUARD + B * Sq, :D].cpu().reshape(B, Sq, H, dk)
    return O, mx.cpu().reshape(B, H, Sq), sm.cpu().reshape(B, H, Sq)


@pytest.mark.parametrize("c", ar.FWD256, ids=ar.case_id)
def test_attention256_paths(dev, c):
    key = ("split", c["B"], c["H"], c["Sq"], c["Sk"], c["mask"], c["dtype"])
    inp, ref = ar.make_inputs(*key), ar.reference(*key)
    _, msq = _mask_strides(inp["mask"], c["Sq"], c["Sk"])
    try:
        _pin(256, c["pin"])
        assert _plan256(c, msq) == c["code"]
        O, mx, sm = _run256(c, inp, dev, clean=False)
        O0, mx0, sm0 = _run256(c, inp, dev, clean=True)
        assert torch.equal(O.view(torch.int16), O0.view(torch.int16)) and torch.equal(mx, mx0) and torch.equal(sm, sm0), \
            "values at masked keys reached the result"
        _assert_within(O, ref["O"], ref["bound"], c["name"] + " O")
        _check_statistics(c, ref, mx.double(), sm.double(), c["Sk"], c["code"] == 256)
        if c.get("drop"):
            p = 0.25
            keep = ar.dropout_keep(p, 5, c["B"], c["Sq"], c["H"], 256)
            Od, _, _ = _run256(c, inp, dev, clean=True, dropout_p=p, seed=5)
            Oe, _, _ = _run256(c, inp, dev, clean=True, dropout_p=p, seed=3, seed_dev=torch.tensor([2], dtype=torch.int64, device=dev))
            assert torch.equal(Od.view(torch.int16), Oe.view(torch.int16)), "seed and seed + seed_dev[0] differ"
            assert bool((Od[~keep] == 0).all()), "an element the numbering drops was kept"
            s = float(torch.tensor(1.0, dtype=torch.float32) / (1 - torch.tensor(p, dtype=torch.float32)))
            kept = torch.where(keep, Od.double(), ref["O"] * s)
            _assert_within(kept, ref["O"] * s, ref["bound"] * s, c["name"] + " O after dropout")
    finally:
        _pin(256, 0)


def test_attention256_dropout_pattern_is_the_same_in_every_kernel(dev):
    """one shape under the three codes: the same elements are dropped (the numbering of the GEMM epilogues)"""
    c = dict(name="drop", B=2, H=2, Sq=65, Sk=130, mask="none", dtype=torch.bfloat16)
    key = ("split", 2, 2, 65, 130, "none", torch.bfloat16)
    inp, ref = ar.make_inputs(*key), ar.reference(*key)
    keep = ar.dropout_keep(0.25, 9, 2, 65, 2, 256)
    outs = []
    try:
        for code in (22, 41, 256):
            _pin(256, code)
            O, _, _ = _run256(c, inp, dev, clean=True, dropout_p=0.25, seed=9)
            assert bool((O[~keep] == 0).all())
            big = keep & (ref["O"].abs() > 4 * ref["bound"])
            assert bool((O[big] != 0).all()), "an element the numbering keeps was dropped"
            outs.append(O == 0)
    finally:
        _pin(256, 0)
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2])


# ------------------------------------------------------------------------------------------------- head dimension 128
def _run128(c, inp, dev, clean):
    from bmhrl_amd import ops
    B, H, Sq, Sk, dt = c["B"], c["H"], c["Sq"], c["Sk"], c["dtype"]
    D = H * 128
    X, _ = ar.kv_of(inp, clean)
    nan = float("nan")
    ldq, ldx, ldo = D + 8, 128 + 16, D + 16
    b1, (Qv,) = _place([(0, inp["Q"].reshape(B * Sq, D))], B * Sq, ldq, dt, dev, nan)
    b2, (Xv,) = _place([(8, X.reshape(B * Sk, 128))], B * Sk, ldx, dt, dev, nan)
    obuf, Ov = _out(B * Sq, D, ldo, dt, dev)
    mxbuf, mx = _stats(B * H * Sq, dev)
    smbuf, sm = _stats(B * H * Sq, dev)
    mbuf, mview = _mask(inp["mask"], c.get("mask_off", 0), dev)
    ops.attention_shared128_fwd(Qv, Xv, Ov, mx, sm, mview, Sk if mview is not None else 0, B, H, Sq, Sk, inp["scale"], ldq, ldx, ldo)
    _sync()
    _check_sentinels(obuf, B * Sq, D, c["name"] + " ctx")
    _check_stat_sentinels(mxbuf, B * H * Sq, c["name"] + " row_max")
    _check_stat_sentinels(smbuf, B * H * Sq, c["name"] + " row_sum")
    return obuf[GUARD:GUARD + B * Sq, :D].cpu().reshape(B, Sq, H, 128), mx.cpu().reshape(B, H, Sq), sm.cpu().reshape(B, H, Sq)


@pytest.mark.parametrize("c", ar.FWD128, ids=ar.case_id)
def test_attention128_paths(dev, c):
    from bmhrl_amd import ops
    key = ("shared", c["B"], c["H"], c["Sq"], c["Sk"], c["mask"], c["dtype"])
    inp, ref = ar.make_inputs(*key), ar.reference(*key)
    try:
        _pin(128, c["pin"])
        assert ops.attention_plan("128-fwd", c["B"], c["H"], c["Sq"], c["Sk"]) == c["code"]
        O, mx, sm = _run128(c, inp, dev, clean=False)
        O0, mx0, sm0 = _run128(c, inp, dev, clean=True)
        assert torch.equal(O.view(torch.int16), O0.view(torch.int16)) and torch.equal(mx, mx0) and torch.equal(sm, sm0), \
            "values at masked keys reached the result"
        _assert_within(O, ref["O"], ref["bound"], c["name"] + " ctx")
        _check_statistics(c, ref, mx.double(), sm.double(), c["Sk"], False)
    finally:
        _pin(128, 0)


def test_pair_form_refuses_an_odd_head_count(dev):
    from bmhrl_amd import _lib, ops
    c = dict(name="odd", B=1, H=3, Sq=33, Sk=65, dtype=torch.bfloat16)
    inp = ar.make_inputs("shared", 1, 3, 33, 65, "none", torch.bfloat16)
    try:
        _pin(128, 14)
        assert ops.attention_plan("128-fwd", 1, 3, 33, 65) < 0
        with pytest.raises(_lib.HipError):
            _run128(c, inp, dev, clean=True)
    finally:
        _pin(128, 0)


# ------------------------------------------------------------------------------------------- backward, shared form
def _run_bwd(c, inp, ref, dev, clean, with_dx=True, accumulate=False, prefill=None):
    from bmhrl_amd import ops
    B, H, Sq, Sk, dt = c["B"], c["H"], c["Sq"], c["Sk"], c["dtype"]
    D = H * 128
    X, _ = ar.kv_of(inp, clean)
    nan = float("nan")
    ldq, ldx, lddo, lddq, lddx = D + 8, 128 + 16, D + 24, D + 16, c.get("lddx", 128)
    b1, (Qv,) = _place([(0, inp["Q"].reshape(B * Sq, D))], B * Sq, ldq, dt, dev, nan)
    b2, (Xv,) = _place([(8, X.reshape(B * Sk, 128))], B * Sk, ldx, dt, dev, nan)
    b3, (Gv,) = _place([(16, inp["dCx"].reshape(B * Sq, D))], B * Sq, lddo, dt, dev, nan)
    rmax, rsum = ar.lagged_statistics(ref["s"])          # from the float64 reference: the backward is judged on its own
    delta = ref["delta"].float().contiguous()
    dqbuf, dQv = _out(B * Sq, D, lddq, dt, dev)
    dxbuf, dXv = _out(B * Sk, 128, lddx, torch.float32, dev)
    if prefill is not None:
        dxbuf[GUARD:GUARD + B * Sk, :128] = prefill.to(dev)
    mbuf, mview = _mask(inp["mask"], c.get("mask_off", 0), dev)
    ops.attention_shared128_bwd(Qv, Xv, Gv, rmax.to(dev), rsum.to(dev), delta.to(dev), mview, Sk if mview is not None else 0,
                                dQv, dXv if with_dx else None, accumulate, B, H, Sq, Sk, inp["scale"], ldq, ldx, lddo, lddq, lddx)
    _sync()
    _check_sentinels(dqbuf, B * Sq, D, c["name"] + " dQp")
    if with_dx:
        _check_sentinels(dxbuf, B * Sk, 128, c["name"] + " dX")
    else:
        assert bool((dxbuf.cpu() == SENT).all()), "dX = NULL wrote to a buffer it was not given"
    dQ = dqbuf[GUARD:GUARD + B * Sq, :D].cpu().reshape(B, Sq, H, 128)
    return dQ, dxbuf[GUARD:GUARD + B * Sk, :128].cpu().reshape(B, Sk, 128)


@pytest.mark.parametrize("c", ar.BWD128, ids=ar.case_id)
def test_attention128_backward_paths(dev, c):
    from bmhrl_amd import ops
    B, H, Sq, Sk = c["B"], c["H"], c["Sq"], c["Sk"]
    key = ("shared", B, H, Sq, Sk, c["mask"], c["dtype"], True)
    inp, ref = ar.make_inputs(*key), ar.reference(*key)
    assert ops.attention_plan("128-bwd", B, H, Sq, Sk) == c["code"]
    dQ, dX = _run_bwd(c, inp, ref, dev, clean=False)               # dX over a sentinel: accumulate_dx = 0 overwrites
    dQ0, dX0 = _run_bwd(c, inp, ref, dev, clean=True)
    assert torch.equal(dQ.view(torch.int16), dQ0.view(torch.int16)) and torch.equal(dX, dX0), "values at masked keys reached the result"
    _assert_within(dQ, ref["dQ"], ref["bound_dQ"], c["name"] + " dQp")
    _assert_within(dX, ref["dX"], ref["bound_dX"], c["name"] + " dX")
    full = ref["full"][:, 0, 0]                                   # (B): fully masked samples get no score gradient at all
    if full.any():
        assert bool((dQ[full] == 0).all())
    # accumulate_dx = 1 adds to what is there (small integers: the sum rounds once more in fp32); dX = NULL skips the key side
    g = torch.Generator().manual_seed(Sq + Sk)
    A = torch.randint(-8, 9, (B * Sk, 128), generator=g).float()
    dQ1, dX1 = _run_bwd(c, inp, ref, dev, clean=True, accumulate=True, prefill=A)
    want = ref["dX"] + A.double().reshape(B, Sk, 128)
    _assert_within(dX1, want, ref["bound_dX"] + 2.0 ** -23 * want.abs(), c["name"] + " dX accumulated")
    dQ2, _ = _run_bwd(c, inp, ref, dev, clean=True, with_dx=False)
    assert torch.equal(dQ1.view(torch.int16), dQ0.view(torch.int16)) and torch.equal(dQ2.view(torch.int16), dQ0.view(torch.int16))


# --------------------------------------------------------------------------------------------------- limits, coverage
def test_one_key_more_than_the_limit_is_refused_without_a_launch(dev):
    from bmhrl_amd import _lib, ops
    Sk = ops.attention_max_keys() + 1
    assert Sk == 10113
    for kind in ("256-fwd", "128-fwd", "128-bwd"):
        assert ops.attention_plan(kind, 1, 1, 32, Sk) < 0 and ops.attention_plan(kind, 1, 1, 32, Sk - 1) > 0
    for dt in (torch.bfloat16, torch.float16):
        Q = torch.zeros(32, 256, dtype=dt, device=dev)
        KV = torch.zeros(Sk, 256, dtype=dt, device=dev)
        O = torch.full((32, 256), SENT, dtype=dt, device=dev)
        st = torch.full((2, 32), SENT, device=dev)
        with pytest.raises(_lib.HipError):
            ops.attention_fwd(Q, KV, KV, O, st[0], st[1], None, 0, 0, 1, 1, 32, Sk, 256, 1 / 16, 256, 256, 256, 256)
        with pytest.raises(_lib.HipError):
            ops.attention_shared128_fwd(Q, KV, O, st[0], st[1], None, 0, 1, 1, 32, Sk, 1 / 16, 128, 128, 128)
        _sync()
        assert bool((O == SENT).all()) and bool((st == SENT).all())
    Q = torch.zeros(32, 128, dtype=torch.bfloat16, device=dev)
    X = torch.zeros(Sk, 128, dtype=torch.bfloat16, device=dev)
    dQ = torch.full((32, 128), SENT, dtype=torch.bfloat16, device=dev)
    dX = torch.full((Sk, 128), SENT, device=dev)
    st = torch.ones(3, 32, device=dev)
    with pytest.raises(_lib.HipError):
        ops.attention_shared128_bwd(Q, X, Q, st[0], st[1], st[2], None, 0, dQ, dX, False, 1, 1, 32, Sk, 1 / 16, 128, 128, 128, 128)
    _sync()
    assert bool((dQ == SENT).all()) and bool((dX == SENT).all())


def test_paths_covered():
    """the tables reach every kernel the host dispatch can choose (asked of bmhrl_attention_plan under each case's pin)"""
    from bmhrl_amd import ops
    got256, got128, gotbwd = set(), set(), set()
    try:
        for c in ar.FWD256:
            if c["dtype"] != torch.bfloat16:
                continue
            qm = c["mask"] in ar.QMASKS
            _pin(256, c["pin"])
            code = ops.attention_plan("256-fwd", c["B"], c["H"], c["Sq"], c["Sk"], c["Sk"] if qm else 0)
            assert code == c["code"]
            got256.add((code, "qmask") if qm else ((code, (c["Sk"] + 31) // 32) if code == 256 else code))
        _pin(256, 0)
        for c in ar.FWD128:
            if c["dtype"] != torch.bfloat16:
                continue
            _pin(128, c["pin"])
            got128.add(ops.attention_plan("128-fwd", c["B"], c["H"], c["Sq"], c["Sk"]))
        _pin(128, 0)
        for c in ar.BWD128:
            gotbwd.add(ops.attention_plan("128-bwd", c["B"], c["H"], c["Sq"], c["Sk"]))
    finally:
        _pin(256, 0)
        _pin(128, 0)
    assert got256 >= {22, 41, (22, "qmask"), (41, "qmask")} | {(256, t) for t in range(1, 9)}, got256
    assert got128 == {22, 41, 24, 14}, got128
    assert gotbwd == {22, 41}, gotbwd          # 22: the narrow dQp kernel, 41: the wide one
    # the fp16 entries take the automatic choice: both of its outcomes
    assert {c["code"] for c in ar.FWD256 if c["dtype"] == torch.float16} == {22, 41}
    assert {c["code"] for c in ar.FWD128 if c["dtype"] == torch.float16} == {22, 41}
