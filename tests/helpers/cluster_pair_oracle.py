"""Plain numpy fp64 oracle of the extrinsic clustering scores: the contingency table by ``np.unique`` / ``np.add.at``, the
nine formulas and their edge rules stated directly, EMI by the triple loop (sklearn's ``_expected_mutual_info_fast``)."""
from math import exp, lgamma, log

import numpy as np

EPS32 = float(np.finfo(np.float32).eps)


def pair_table(preds, target):
    """int64 ``[K_target, K_preds]`` co-occurrence counts."""
    _, ip = np.unique(np.asarray(preds), return_inverse=True)
    _, it = np.unique(np.asarray(target), return_inverse=True)
    table = np.zeros((it.max() + 1, ip.max() + 1), dtype=np.int64)
    np.add.at(table, (it.reshape(-1), ip.reshape(-1)), 1)
    return table


def _entropy(counts, n):
    return -sum(c / n * (log(c) - log(n)) for c in counts if c > 0)


def _emi(a, b, n):
    if len(a) == 1 or len(b) == 1:
        return 0.0
    lg = [lgamma(i + 1.0) for i in range(n + 1)]
    total = 0.0
    for ai in a:
        for bj in b:
            for nij in range(max(1, ai + bj - n), min(ai, bj) + 1):
                gln = lg[ai] + lg[bj] + lg[n - ai] + lg[n - bj] - lg[n] - lg[nij] - lg[ai - nij] - lg[bj - nij] - lg[n - ai - bj + nij]
                total += nij / n * (log(n * nij) - log(ai * bj)) * exp(gln)
    return total


def pair_stats(preds, target, emi=False):
    """The quantities every score is made of: ``mi``, ``h_p``, ``h_t``, the pair matrix ``tn, fp, fn, tp`` and, on request, ``emi``."""
    table = pair_table(preds, target)
    n = int(table.sum())
    a, b = [int(v) for v in table.sum(axis=1)], [int(v) for v in table.sum(axis=0)]
    mi = sum(int(table[i, j]) / n * (log(n * int(table[i, j])) - log(a[i] * b[j])) for i, j in zip(*np.nonzero(table)))
    sq, sa, sb = int((table.astype(object) ** 2).sum()), sum(v * v for v in a), sum(v * v for v in b)
    out = {"n": n, "mi": mi, "h_p": _entropy(b, n), "h_t": _entropy(a, n), "tp": sq - n, "fp": sa - sq, "fn": sb - sq,
           "tn": n * n - sa - sb + sq, "tk": sq - n, "pk": sb - n, "qk": sa - n}
    if emi:
        out["emi"] = _emi(a, b, n)
    return out


def _mean(h_p, h_t, average):
    if average == "geometric":
        return (h_p * h_t) ** 0.5
    return {"min": min(h_p, h_t), "max": max(h_p, h_t), "arithmetic": 0.5 * (h_p + h_t)}[average]


def ami_denominator(s, average):
    return _mean(s["h_p"], s["h_t"], average) - s["emi"]


def pair_score(s, metric, average="arithmetic", beta=1.0):
    """The score ``metric`` from ``pair_stats`` ``s``, with the rules of the functionals."""
    mi, h_p, h_t = s["mi"], s["h_p"], s["h_t"]
    if metric == "mutual_info":
        return mi
    if metric == "normalized_mutual_info":
        return mi if abs(mi) <= EPS32 else mi / _mean(h_p, h_t, average)
    if metric == "adjusted_mutual_info":
        den = ami_denominator(s, average)
        den = min(den, -EPS32) if den < 0 else max(den, EPS32)
        return (mi - s["emi"]) / den
    if metric == "rand":
        num, den = s["tn"] + s["tp"], s["tn"] + s["fp"] + s["fn"] + s["tp"]
        return 1.0 if num == den or den == 0 else num / den
    if metric == "adjusted_rand":
        tn, fp, fn, tp = s["tn"], s["fp"], s["fn"], s["tp"]
        return 1.0 if fn == 0 and fp == 0 else 2.0 * (tp * tn - fn * fp) / ((tp + fn) * (fn + tn) + (tp + fp) * (fp + tn))
    if metric == "fowlkes_mallows":
        return 0.0 if s["tk"] == 0 else (s["tk"] / s["pk"]) ** 0.5 * (s["tk"] / s["qk"]) ** 0.5
    h = mi / h_t if h_t else 1.0
    c = mi / h_p if h_p else 1.0
    if metric == "homogeneity":
        return h
    if metric == "completeness":
        return c
    return 1.0 if h + c == 0.0 else (1 + beta) * h * c / (beta * h + c)
