"""Test oracle of afhip_sample_filter: the processor pipeline of transformers' GenerationMixin (repetition penalty -> temperature ->
top-k -> top-p) restated on one row, and the draw as the inverse CDF at u over the kept ids in ascending id order.

The element-wise steps (guidance mix, penalty, temperature) are done in f32 exactly as torch does them on f32 logits; the selection,
the softmax masses and the CDF in float64.  Top-p is value-granular (ids of equal value are kept or dropped together); tests keep
every cumulative mass away from the 1 - p boundary, where that and torch.sort's tie order could differ."""
import numpy as np


def mix_f32(logits, cfg_logits, cfg):
    """logits * cfg + cfg_logits * (1 - cfg) as three f32 tensor ops (the f32 model dtype of lm/parallel.py:489-492)."""
    a = np.float32(logits) * np.float32(cfg)
    b = np.float32(cfg_logits) * np.float32(1.0 - cfg)
    return (a + b).astype(np.float32)


def process(row, *, penalty=1.0, ids=None, temperature=1.0, top_k=0, exact_k=False, top_p=1.0, allowed=None):
    """row [V] f32 -> (processed f32 row with -inf where removed, kept mask)."""
    x = np.array(row, dtype=np.float32).copy()
    V = x.shape[0]
    if allowed is not None:
        ok = np.zeros(V, dtype=bool)
        for lo, hi in allowed:
            ok[lo:hi] = True
        x[~ok] = -np.inf
    if penalty != 1.0 and ids is not None:
        u = np.unique(np.asarray(ids, dtype=np.int64))
        u = u[(u >= 0) & (u < V)]
        s = x[u]
        x[u] = np.where(s < 0, s * np.float32(penalty), s / np.float32(penalty))
    if temperature != 1.0:
        x = (x / np.float32(temperature)).astype(np.float32)
    keep = np.ones(V, dtype=bool)
    if top_k and top_k < V:
        if exact_k:
            order = np.lexsort((np.arange(V), -x.astype(np.float64)))      # value descending, then smaller id
            keep = np.zeros(V, dtype=bool)
            keep[order[:top_k]] = True
        else:
            kth = np.sort(x)[::-1][top_k - 1]
            keep = x >= kth
    if top_p < 1.0:
        above = mass_above(np.where(keep, x, -np.inf))
        keep &= above < top_p
    return np.where(keep, x, np.float32(-np.inf)).astype(np.float32), keep


def softmax64(x):
    x = np.asarray(x, dtype=np.float64)
    m = x.max()
    if not np.isfinite(m):
        return np.zeros_like(x)
    e = np.exp(x - m)
    return e / e.sum()


def mass_above(x):
    """per id: softmax mass of the ids with a STRICTLY larger value"""
    p = softmax64(x)
    order = np.argsort(-x.astype(np.float64), kind="stable")
    xs, ps = x[order].astype(np.float64), p[order]
    cum = np.concatenate([[0.0], np.cumsum(ps)])
    first = np.searchsorted(-xs, -xs, side="left")             # index of the first id of each id's value group
    out = np.empty_like(p)
    out[order] = cum[first]
    return out


def p_margin(x, keep_k, top_p):
    """distance of the top-p boundary from the nearest value group's `mass above` (how safe p is for this row)"""
    above = mass_above(np.where(keep_k, x, -np.inf))
    return float(np.min(np.abs(above[keep_k] - top_p)))


def probs(scores):
    return softmax64(scores)


def draw(scores, u):
    """inverse CDF at u over the kept ids in ascending id order -> (token, distance of u from the nearest CDF step)"""
    p = softmax64(scores)
    cdf = np.cumsum(p)
    j = int(np.searchsorted(cdf, u, side="right"))
    j = min(j, len(p) - 1)
    while p[j] == 0 and j > 0:
        j -= 1
    steps = cdf[p > 0]
    return j, float(np.min(np.abs(steps - u))) if steps.size else 1.0


def argmax_first(x):
    return int(np.argmax(x))
