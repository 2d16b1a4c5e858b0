"""Oracle of the loss-tail tests (csrc/loss.hip): the log-softmax, the label-smoothing and biased KL divergences with their
amplitudes, the token-normalised loss, the REINFORCE terms and the inverse-CDF sampler, each written out from its formula in
plain torch, in the dtype and on the device of its inputs (float64 on the CPU = the oracle; float32 = the yardstick of the
rounding error).  Every gradient comes from torch autograd on these formulas; none is derived by hand.  Nothing here touches
the package under test; tests/test_loss_reference_cpu.py proves the formulas against torch.nn.functional.kl_div and the
recorded outputs of the original project (tests/golden/losses.npz, kat.npz).

The target distribution of a row (loss/label_smoothing.py:12-32, loss/biased_kl.py:22-53), V columns:
    smoothing / (V - 2) everywhere; (1 - smoothing)(1 - amp) at the target; 0 at the pad; + (1 - smoothing) amp at the sampled
    token; a row whose target is the pad is all 0 -- but only if the flat indices of the padded rows sum to more than 0, so a
    padded row 0 alone stays as it is; + 1e-8 everywhere in the biased form.  divergence = d log d - d logp (0 log 0 = 0)."""
import torch

# the REINFORCE clamp [1e-5, 1 - 1e-5] as the original's float32 clamp holds it: both bounds rounded to float32, so that a
# float32 probability can sit exactly on either and the float64 oracle sees it there too (closed interval: it carries gradient)
REINFORCE_LO = float(torch.tensor(1e-5, dtype=torch.float32))
REINFORCE_HI = float(torch.tensor(1.0 - 1e-5, dtype=torch.float32))
REST, TARGET, SAMPLED, PADCOL = 0, 1, 2, 3
CLASS_NAMES = ("rest", "target", "sampled", "pad")
MASK64 = (1 << 64) - 1


# ---- the divergences
def zeroed_rows(trg, pad, zero_pad_rows=-1):
    """(rows,) bool: the padded rows that the original zeroes.  zero_pad_rows 0 / 1 overrides its index-sum guard."""
    padded = trg.reshape(-1) == pad
    if zero_pad_rows >= 0:
        return padded & bool(zero_pad_rows)
    idx = torch.nonzero(padded).reshape(-1)
    return padded & bool(idx.numel() > 0 and int(idx.sum()) > 0)


def target_distribution(like, trg, biased_trg, amp, smoothing, pad, zero_pad_rows=-1):
    """(rows, V) in the dtype of `like` (rows, V); amp (rows,) or None with biased_trg None (plain label smoothing)"""
    rows, V = like.shape
    trg = trg.reshape(-1)
    col = torch.arange(V, device=like.device)[None, :]
    keep = 1.0 - smoothing
    dist = torch.full_like(like, smoothing / (V - 2))
    at_t = keep * (1.0 - amp)[:, None] if biased_trg is not None else torch.full_like(like[:, :1], keep)
    dist = torch.where(col == trg[:, None], at_t.expand(rows, V), dist)
    dist = torch.where(col == pad, torch.zeros_like(dist), dist)
    if biased_trg is not None:
        dist = dist + (col == biased_trg.reshape(-1)[:, None]).to(like.dtype) * (keep * amp)[:, None]
    dist = torch.where(zeroed_rows(trg, pad, zero_pad_rows)[:, None], torch.zeros_like(dist), dist)
    return dist + 1e-8 if biased_trg is not None else dist


def divergence(logp, trg, biased_trg, amp, smoothing, pad, zero_pad_rows=-1):
    """(rows, V): xlogy(d, d) - d * logp over the materialised target distribution d"""
    d = target_distribution(logp, trg, biased_trg, amp, smoothing, pad, zero_pad_rows)
    return torch.xlogy(d, d) - d * logp


def amplitude(logp, biased_trg, score, n_row):
    """-> raw = score exp(logp[a]) n_row and its clamp to [0, 1], both (rows,)"""
    raw = score * torch.exp(torch.gather(logp, 1, biased_trg.reshape(-1, 1)).squeeze(1)) * n_row
    return raw, torch.clamp(raw, 0.0, 1.0)


def manager_amplitude(logp, biased_trg, score, n_seg, segments):
    """logp (B, S, V), biased_trg / score / segments (B, S), n_seg (B,): clamp(score * prod_{j in the position's segment}
    p(a_j) * n_seg, 0, 1); `segments` marks the last position of every segment, the positions behind the last mark belong to
    no segment and get 0.  -> (B, S)"""
    B, S, _ = logp.shape
    p = torch.exp(torch.gather(logp, 2, biased_trg.unsqueeze(-1)).squeeze(-1))
    out = []
    for b in range(B):
        row, start = [torch.zeros((), dtype=logp.dtype, device=logp.device)] * S, 0
        for s in range(S):
            if int(segments[b, s]) != 0:
                prod = torch.ones((), dtype=logp.dtype, device=logp.device)
                for j in range(start, s + 1):
                    prod = prod * p[b, j]
                for j in range(start, s + 1):
                    row[j] = torch.clamp(score[b, j] * prod * n_seg[b], 0.0, 1.0)
                start = s + 1
        out.append(torch.stack(row))
    return torch.stack(out)


def column_classes(V, trg, biased_trg, pad):
    """(rows, V) int64: SAMPLED at the row's sampled token wherever it sits (also on the target or the pad: it is the one column
    that receives the amplitude), else PADCOL at the pad, else TARGET at the target, else REST"""
    trg = trg.reshape(-1)
    col = torch.arange(V, device=trg.device)[None, :]
    cls = torch.zeros(trg.numel(), V, dtype=torch.int64, device=trg.device)
    cls[col == trg[:, None]] = TARGET
    cls[(col == pad).expand_as(cls)] = PADCOL
    if biased_trg is not None:
        cls[col == biased_trg.reshape(-1)[:, None]] = SAMPLED
    return cls


def kl_rows(logp, trg, biased_trg, score, n_row, smoothing, pad, zero_pad_rows=-1):
    """row sums (rows,) with the amplitude formed from the log-probs themselves (attached), and the amplitude"""
    amp = amplitude(logp, biased_trg, score, n_row)[1] if biased_trg is not None else None
    return divergence(logp, trg, biased_trg, amp, smoothing, pad, zero_pad_rows).sum(1), amp


def kl_grad(x, trg, biased_trg, score, n_row, smoothing, pad, zero_pad_rows=-1, scale=1.0, wrt_logits=False):
    """autograd of scale * sum(rows) w.r.t. x: the log-probs themselves, or (wrt_logits) logits behind a log-softmax"""
    x = x.detach().clone().requires_grad_(True)
    logp = torch.log_softmax(x, -1) if wrt_logits else x
    rows, _ = kl_rows(logp, trg, biased_trg, score, n_row, smoothing, pad, zero_pad_rows)
    (rows.sum() * scale).backward()
    return x.grad


def kl_amp_grad(logp, trg, biased_trg, score, n_row, smoothing, pad, zero_pad_rows=-1):
    """d rows / d log raw (rows,): the log-prob of the sampled token is a leaf of its own that feeds the amplitude alone, so
    what autograd returns for it is d rows / d raw * raw"""
    lpa = torch.gather(logp, 1, biased_trg.reshape(-1, 1)).squeeze(1).detach().clone().requires_grad_(True)
    amp = torch.clamp(score * torch.exp(lpa) * n_row, 0.0, 1.0)
    divergence(logp.detach(), trg, biased_trg, amp, smoothing, pad, zero_pad_rows).sum().backward()
    return lpa.grad


def given_amp(logp, trg, biased_trg, amp, smoothing, pad, drow):
    """BiasedKL with the amplitude as an argument: rows, d (rows . drow) / d logp and / d amp"""
    logp = logp.detach().clone().requires_grad_(True)
    amp = amp.detach().clone().requires_grad_(True)
    rows = divergence(logp, trg, biased_trg, amp, smoothing, pad).sum(1)
    (rows * drow).sum().backward()
    return rows.detach(), logp.grad, amp.grad


def manager_kl(logp, trg, biased_trg, score, n_seg, segments, smoothing, pad, drow):
    """logp (B, S, V) -> rows (B*S,), amplitude (B*S,), d (rows . drow) / d logp (B, S, V)"""
    B, S, V = logp.shape
    logp = logp.detach().clone().requires_grad_(True)
    amp = manager_amplitude(logp, biased_trg, score, n_seg, segments).reshape(-1)
    rows = divergence(logp.reshape(B * S, V), trg, biased_trg, amp, smoothing, pad).sum(1)
    (rows * drow).sum().backward()
    return rows.detach(), amp.detach(), logp.grad


# ---- the reductions
def token_loss(rows, trg, pad, weight=None, factor=1.0):
    """-> loss = weight sum(rows) / (n_tokens factor), scale = weight / (n_tokens factor); n_tokens = #(trg != pad)"""
    n = (trg.reshape(-1) != pad).sum().to(rows.dtype)
    w = (1.0 if weight is None else weight) / (n * factor)
    return rows.sum() * w, w


def head_loss(logits, trg, smoothing, pad, weight=None, factor=1.0, dloss=1.0):
    """the warmstart tail: -> logp, rows, loss, scale, d (loss dloss) / d logits"""
    x = logits.detach().clone().requires_grad_(True)
    logp = torch.log_softmax(x, -1)
    rows = divergence(logp, trg, None, None, smoothing, pad).sum(1)
    loss, scale = token_loss(rows, trg, pad, weight, factor)
    (loss * dloss).backward()
    return logp.detach(), rows.detach(), loss.detach(), scale, x.grad


def log_softmax_bwd(x, dlogp):
    """d <log_softmax(x), dlogp> / d x"""
    x = x.detach().clone().requires_grad_(True)
    torch.log_softmax(x, -1).backward(dlogp)
    return x.grad


def reinforce(pred, is_logp, action, value, critic):
    """pred (rows, V) log-probs or probabilities -> row_policy = -adv.detach() log clamp(p(a), 1e-5, 1 - 1e-5), row_value = adv^2"""
    raw = torch.gather(pred, 1, action.reshape(-1, 1)).squeeze(1)
    pa = torch.clamp(torch.exp(raw) if is_logp else raw, REINFORCE_LO, REINFORCE_HI)
    adv = value - critic
    return -adv.detach() * torch.log(pa), adv * adv


def reinforce_grad(probs, action, value, critic, gscale=1.0):
    """autograd of gscale (mean(row_policy) + mean(row_value)) w.r.t. the probabilities, value and critic"""
    probs, value, critic = (t.detach().clone().requires_grad_(True) for t in (probs, value, critic))
    rp, rv = reinforce(probs, False, action, value, critic)
    ((rp.mean() + rv.mean()) * gscale).backward()
    return probs.grad, value.grad, critic.grad


# ---- the sampler
def hash_u32(seed, idx):
    """csrc/common.h hash_u32 in python integers masked to 64 bits"""
    z = (idx * 0x9E3779B97F4A7C15 + seed) & MASK64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & MASK64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & MASK64
    z = z ^ (z >> 31)
    return z >> 32


def uniform01(seed, idx):
    """the top 24 bits of the hash times 2^-24: exact in float32 and in float64"""
    return (hash_u32(seed & MASK64, idx & MASK64) >> 8) * 2.0 ** -24


def inverse_cdf(logp64, u):
    """logp64 (V,) float64 -> pick (first c with cdf[c] > u total; V - 1 if none), cdf (V,), total"""
    cdf = torch.cumsum(torch.exp(logp64), 0)
    total = float(cdf[-1])
    above = torch.nonzero(cdf > u * total).reshape(-1)
    return (int(above[0]) if above.numel() else logp64.numel() - 1), cdf, total


def sampler_tol(V, total, nt=256):
    """bound on the fp32 error of the sampler's running sums against the float64 cdf: non-negative terms summed over a thread's
    chunk, over the 256 partials and over the final chunk, (2 chunk + 256) 2^-24 total, + 16 for the few-ulp error of the fast
    exponential per term"""
    chunk = (V + nt - 1) // nt
    return 2.0 ** -24 * (2 * chunk + 256 + 16) * total


def sampler_rows(logp64, seed, row_offset):
    """per row of logp64 (rows, V): (u, float64 pick, cdf, total, tol, decided) -- decided: u total lies more than tol from every
    cdf boundary, so every correct fp32 sampler must return the float64 pick"""
    out = []
    V = logp64.shape[1]
    for r in range(logp64.shape[0]):
        u = uniform01(seed, r + row_offset)
        pick, cdf, total = inverse_cdf(logp64[r], u)
        tol = sampler_tol(V, total)
        out.append((u, pick, cdf, total, tol, bool(((cdf - u * total).abs() > tol).all())))
    return out
