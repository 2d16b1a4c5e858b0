"""float64 numpy / scipy restatement of the DETR word loss (bmhrl_amd/csrc/word_loss.hip): the
compaction of a caption into its words, the matching cost, the assignment (scipy's linear_sum_assignment, which is what
the reference runs), the class map, the weighted cross entropy and its gradient.  The tests compare the kernels, and the
fixture recorded from the reference, against this."""
import numpy as np
from scipy.optimize import linear_sum_assignment


def compact(captions, pad_idx, C):
    """words (B, L) int32 with -1 behind the n_b words, n_words (B) int32: entries != pad_idx with an id in [0, C - 2], in order"""
    cap = np.asarray(captions, dtype=np.int64)
    B, L = cap.shape
    words = np.full((B, L), -1, dtype=np.int32)
    n = np.zeros(B, dtype=np.int32)
    for b in range(B):
        w = [v for v in cap[b] if v != pad_idx and 0 <= v <= C - 2]
        words[b, :len(w)] = w
        n[b] = len(w)
    return words, n


def row_stats(logits):
    """lse (B, Q) and x_none (B, Q) in float64 from the logits as given (B, Q, C)"""
    x = np.asarray(logits, dtype=np.float64)
    m = x.max(-1)
    return m + np.log(np.exp(x - m[..., None]).sum(-1)), x[..., -1]


def cost_pass(logits, captions, pad_idx, cost_scale=1.0):
    """words, n_words, lse, x_none, gathered (B, Q, L), cost (B, Q, L): gathered and cost are 0 behind the n_b words"""
    x = np.asarray(logits, dtype=np.float64)
    B, Q, C = x.shape
    words, n = compact(captions, pad_idx, C)
    L = words.shape[1]
    lse, x_none = row_stats(x)
    gathered = np.zeros((B, Q, L))
    cost = np.zeros((B, Q, L))
    for b in range(B):
        k = int(n[b])
        gathered[b, :, :k] = x[b][:, words[b, :k]]
        cost[b, :, :k] = cost_scale * -np.exp(gathered[b, :, :k] - lse[b][:, None])
    return words, n, lse, x_none, gathered, cost


def match(cost, n):
    """query_of_target (B, L) int32 by scipy: cost (B, Q, L), the first n[b] columns are targets; -1 behind them"""
    cost = np.asarray(cost)
    B, Q, L = cost.shape
    qot = np.full((B, L), -1, dtype=np.int32)
    for b in range(B):
        k = int(n[b])
        if k:
            qi, tj = linear_sum_assignment(cost[b, :, :k])
            qot[b, tj] = qi
    return qot


def matching_cost(cost_b, qot_b, k):
    """total cost of sample b's matching, summed in float64 over the entries as given"""
    return float(sum(np.float64(cost_b[int(qot_b[j]), j]) for j in range(int(k))))


def class_map(words, n, qot, Q, C):
    """tgt_class (B, Q) int32: the matched word or C - 1"""
    B = words.shape[0]
    cls = np.full((B, Q), C - 1, dtype=np.int32)
    for b in range(B):
        for j in range(int(n[b])):
            if 0 <= qot[b, j] < Q:
                cls[b, qot[b, j]] = words[b, j]
    return cls


def loss_and_grad(logits, cls, eos_coef):
    """weighted cross entropy sum w (lse - x_t) / sum w with w = eos_coef on the rows of class C - 1 and 1 elsewhere, and
    d loss / d logits (B, Q, C), in float64"""
    x = np.asarray(logits, dtype=np.float64)
    B, Q, C = x.shape
    lse, _ = row_stats(x)
    cls = np.asarray(cls, dtype=np.int64)
    w = np.where(cls == C - 1, float(eos_coef), 1.0)
    xt = np.take_along_axis(x, cls[..., None], -1)[..., 0]
    den = w.sum()
    loss = (w * (lse - xt)).sum() / den
    grad = np.exp(x - lse[..., None])
    np.put_along_axis(grad, cls[..., None], np.take_along_axis(grad, cls[..., None], -1) - 1.0, -1)
    return loss, grad * (w / den)[..., None]


def word_loss(logits, captions, pad_idx=1, eos_coef=0.1, cost_scale=1.0):
    """the whole forward and backward: (class map, loss, gradient, query_of_target, n_words)"""
    x = np.asarray(logits, dtype=np.float64)
    B, Q, C = x.shape
    words, n, _, _, _, cost = cost_pass(x, captions, pad_idx, cost_scale)
    qot = match(cost, n)
    cls = class_map(words, n, qot, Q, C)
    loss, grad = loss_and_grad(x, cls, eos_coef)
    return cls, loss, grad, qot, n
