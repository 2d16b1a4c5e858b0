"""Oracle of the row-kernel tests (csrc/elementwise.hip, csrc/conv_gn.hip): every operation written out from its formula
in plain torch on the CPU, in the dtype of its inputs (float64 = the oracle; float32 = the yardstick of the rounding error).
Nothing here touches the package under test, and nothing calls torch's own layer_norm / group_norm / conv1d / index_add_:
tests/test_row_reference_cpu.py proves these formulas against those, in float64."""
import torch

LN_EPS = 1e-5


def rel_err(a, b, floor=1e-6):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).abs().max() / max(float(b.abs().max()), floor))


# ---- LayerNorm over the last axis of (rows, D)
def layernorm_fwd(x, gamma, beta, eps=LN_EPS):
    """-> y, mean (rows), rstd (rows); biased variance"""
    mean = x.mean(1)
    xc = x - mean[:, None]
    rstd = 1.0 / torch.sqrt((xc * xc).mean(1) + eps)
    return xc * rstd[:, None] * gamma + beta, mean, rstd


def layernorm_bwd(dy, x, gamma, dx_add=None, eps=LN_EPS):
    """-> dx (+ dx_add), dgamma, dbeta.  dx = rstd (g - mean(g) - xh mean(g xh)), g = dy gamma, xh = (x - mean) rstd"""
    _, mean, rstd = layernorm_fwd(x, gamma, torch.zeros_like(gamma), eps)
    xh = (x - mean[:, None]) * rstd[:, None]
    g = dy * gamma
    dx = rstd[:, None] * (g - g.mean(1, keepdim=True) - xh * (g * xh).mean(1, keepdim=True))
    if dx_add is not None:
        dx = dx + dx_add
    return dx, (dy * xh).sum(0), dy.sum(0)


# ---- GroupNorm over (T, C / G) per (sample, group) of a (B, T, C) layout; channel c belongs to group c // (C / G)
def groupnorm_fwd(x, gamma, beta, G, eps=LN_EPS):
    """-> y (B, T, C), mean (B, G), rstd (B, G)"""
    B, T, C = x.shape
    xg = x.reshape(B, T, G, C // G)
    mean = xg.mean((1, 3))
    xc = xg - mean[:, None, :, None]
    rstd = 1.0 / torch.sqrt((xc * xc).mean((1, 3)) + eps)
    xh = (xc * rstd[:, None, :, None]).reshape(B, T, C)
    return xh * gamma + beta, mean, rstd


def groupnorm_bwd(dy, x, gamma, G, eps=LN_EPS):
    """-> dx, dgamma, dbeta"""
    B, T, C = x.shape
    _, mean, rstd = groupnorm_fwd(x, gamma, torch.zeros_like(gamma), G, eps)
    r4 = rstd[:, None, :, None]
    xh = (x.reshape(B, T, G, C // G) - mean[:, None, :, None]) * r4
    g = (dy * gamma).reshape(B, T, G, C // G)
    dx = r4 * (g - g.mean((1, 3), keepdim=True) - xh * (g * xh).mean((1, 3), keepdim=True))
    xh = xh.reshape(B, T, C)
    return dx.reshape(B, T, C), (dy * xh).sum((0, 1)), dy.sum((0, 1))


# ---- Conv1d(padding='same') as a GEMM over an unfolded operand
def same_left(k):
    """steps of padding on the left; an even kernel has its extra step on the right"""
    return (k - 1) // 2


def unfold1d(x, k, left=None):
    """(B, T, C) -> (B * T, k * C): row (b, t) holds the steps t - left .. t - left + k - 1 side by side, zeros outside the clip"""
    B, T, C = x.shape
    left = same_left(k) if left is None else left
    out = torch.zeros(B, T, k, C, dtype=x.dtype)
    for j in range(k):
        for t in range(T):
            ts = t + j - left
            if 0 <= ts < T:
                out[:, t, j] = x[:, ts]
    return out.reshape(B * T, k * C)


def fold1d_terms(du, B, T, C, k, left=None):
    """the k terms of every element of the fold, (k, B, T, C): term j of (b, t, c) is du[(b, t - j + left)][j * C + c] or 0"""
    left = same_left(k) if left is None else left
    u = du.reshape(B, T, k, C)
    terms = torch.zeros(k, B, T, C, dtype=du.dtype)
    for j in range(k):
        for t in range(T):
            tr = t - j + left
            if 0 <= tr < T:
                terms[j, :, t] = u[:, tr, j]
    return terms


def fold1d(du, B, T, C, k, left=None):
    """(B * T, k * C) -> (B, T, C): the adjoint of unfold1d"""
    return fold1d_terms(du, B, T, C, k, left).sum(0)


# ---- embedding gradient of the mixed two-token lookup e = scale ((1 - mix) table[tok] + mix table[tok2])
def embed_bwd(tok, tok2, mix, dC, V, scale):
    """tok, tok2 (rows) int64, dC (rows, D) -> dtable (V, D)"""
    dt = torch.zeros(V, dC.shape[1], dtype=dC.dtype)
    for r in range(dC.shape[0]):
        g = dC[r] * scale
        if tok2 is None:
            dt[int(tok[r])] += g
        else:
            dt[int(tok[r])] += g * (1.0 - mix)
            dt[int(tok2[r])] += g * mix
    return dt


# ---- backward of a row gather: dx[src[r]] += dout[r] for src[r] >= 0
def general_row_map(rows, generator):
    """a row map no expand_goals produces: random targets in [0, rows) with repeats, every fifth row pointing nowhere (-1)"""
    src = torch.randint(0, rows, (rows,), generator=generator).to(torch.int32)
    src[::5] = -1
    return src


def scatter_add_rows(dout, src, n_rows):
    dx = torch.zeros(n_rows, dout.shape[1], dtype=dout.dtype)
    for r in range(dout.shape[0]):
        s = int(src[r])
        if s >= 0:
            dx[s] += dout[r]
    return dx


# ---- fusion gate out = g cv + (1 - g) ca, g = sigmoid(clamp(a, -2, 2)); the clamp passes gradient on the CLOSED interval
def gate_bwd(dout, cv, ca, a):
    """a: python float -> dcv, dca, da (0-d tensor)"""
    ac = min(max(float(a), -2.0), 2.0)
    g = 1.0 / (1.0 + torch.exp(torch.tensor(-ac, dtype=dout.dtype)))
    inside = -2.0 <= float(a) <= 2.0
    da = (dout * (cv - ca)).sum() * g * (1.0 - g) if inside else torch.zeros((), dtype=dout.dtype)
    return g * dout, (1.0 - g) * dout, da
