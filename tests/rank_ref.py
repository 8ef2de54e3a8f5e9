"""dad_rank_metrics and dad_rank_eval_columns (include/dad.h, csrc/rank.hip) restated in NumPy: integers as integers,
doubles in float64, `quant` in the float32 arithmetic of the step's DACP threshold.

`variant` switches on one deliberate mistake (WRONG): the GPU cases must tell each of them from the right answer."""
import math

import numpy as np

MEMBER, POSITIVE = 1, 2
(C_MEMBERS, C_POSITIVES, C_NONFINITE, C_RUNS, C_U2, C_ACCEPTED, C_ACCEPTED_POS, C_VALID_AUROC, N_COUNTS) = range(9)
V_AUROC, V_AP, V_AURC, V_KEY_MEAN, V_KEY_STD, V_KEY_MIN, V_KEY_MAX, N_VALUES = 0, 1, 2, 3, 4, 5, 6, 8
WRONG = ("ties_by_descending_index", "gt_at_threshold", "negative_zero_below", "no_tie_term", "aurc_every_position")
U = 2.0 ** -53


def quantile_f32(sorted_desc, gamma):
    """torch.quantile(linear) of float32 keys in float32: rank gamma (M - 1), lerp with the w < 0.5 branch."""
    M = len(sorted_desc)
    if M == 0:
        return np.float32(np.nan)
    asc = sorted_desc[::-1]
    rank = np.float32(gamma) * np.float32(M - 1)
    lo, hi = int(rank), int(np.ceil(rank))
    w = np.float32(rank - np.float32(lo))
    vlo, vhi = asc[min(max(lo, 0), M - 1)], asc[min(max(hi, 0), M - 1)]
    if w < np.float32(0.5):
        return np.float32(vlo + np.float32(w * np.float32(vhi - vlo)))
    return np.float32(vhi - np.float32(np.float32(vhi - vlo) * np.float32(np.float32(1) - w)))


def column(key, flags, thr=np.nan, gammas=(), bins=0, bin_range=(0.0, 1.0), variant=""):
    """One column: {'order', 'cum_pos', 'tie_end' [n], 'counts' [8] int64, 'values' [8] float64, 'scale' [8] (the sum of
    |terms| behind each value, for the bound of a sum in any order), 'quant' [Q] float32, 'bin_counts' [B][2],
    'bin_sum' [B], 'bin_abs' [B]}."""
    assert variant in ("",) + WRONG
    key = np.asarray(key, np.float32)
    flags = np.asarray(flags, np.uint8)
    n = len(key)
    member = (flags & MEMBER) != 0
    part = member & np.isfinite(key)
    idx = np.nonzero(part)[0]
    k = key[idx] + np.float32(0.0)                   # one zero
    cmp = k.astype(np.float64)
    if variant == "negative_zero_below":
        cmp = np.where((key[idx] == 0) & np.signbit(key[idx]), -1e-300, cmp)
    pos = (flags[idx] & POSITIVE) != 0
    o = np.lexsort((-idx if variant == "ties_by_descending_index" else idx, -cmp))
    sk, sc, sp = k[o], cmp[o], pos[o].astype(np.int64)
    M, P = len(idx), int(pos.sum())
    N = M - P
    order = np.full(n, -1, np.int32)
    order[:M] = idx[o]
    cum = np.zeros(n, np.int32)
    cum[:M] = np.cumsum(sp)
    tie = np.zeros(n, np.uint8)
    if M:
        tie[:M - 1] = sc[1:] != sc[:-1]
        tie[M - 1] = 1
    te = np.nonzero(tie)[0].astype(np.int64)
    C = cum[te].astype(np.int64)
    Cp = np.concatenate(([0], C[:-1]))
    size = te - np.concatenate(([-1], te[:-1]))
    pos_r, taken = C - Cp, te + 1
    below = N - (taken - C)
    u2 = int(np.sum(pos_r * (2 * below + (0 if variant == "no_tie_term" else size - pos_r))))
    thr = np.float32(thr)
    with np.errstate(invalid="ignore"):
        acc = (sk > thr) if variant == "gt_at_threshold" else (sk >= thr)
    counts = np.zeros(N_COUNTS, np.int64)
    counts[[C_MEMBERS, C_POSITIVES, C_NONFINITE, C_RUNS, C_U2]] = M, P, int((member & ~part).sum()), len(te), u2
    counts[[C_ACCEPTED, C_ACCEPTED_POS]] = int(acc.sum()), int(sp[acc].sum())
    counts[C_VALID_AUROC] = int(P > 0 and N > 0)
    values, scale = np.zeros(N_VALUES), np.zeros(N_VALUES)
    if P > 0 and N > 0:
        values[V_AUROC] = u2 / (2 * P * N)
    if P > 0:
        values[V_AP] = np.sum((C / P - Cp / P) * (C / taken))
    if M > 0:
        if variant == "aurc_every_position":
            every = np.arange(1, M + 1)
            values[V_AURC] = np.sum((every - cum[:M]) / every) / M
        else:
            values[V_AURC] = np.sum(size * ((taken - C) / taken)) / M
        k64 = sk.astype(np.float64)
        values[V_KEY_MEAN], values[V_KEY_STD] = np.mean(k64), np.std(k64)
        values[V_KEY_MIN], values[V_KEY_MAX] = k64.min(), k64.max()
        scale[V_KEY_MEAN] = np.sum(np.abs(k64)) / M
    scale[[V_AUROC, V_AP, V_AURC, V_KEY_STD]] = values[[V_AUROC, V_AP, V_AURC, V_KEY_STD]]   # (sums of terms >= 0)
    quant = np.array([quantile_f32(sk, g) for g in gammas], np.float32)
    B = int(bins)
    bin_counts, bin_sum, bin_abs = np.zeros((B, 2), np.int64), np.zeros(B), np.zeros(B)
    if B:
        lo, hi = float(np.float32(bin_range[0])), float(np.float32(bin_range[1]))
        b = np.clip(np.floor((sk.astype(np.float64) - lo) / (hi - lo) * B), 0, B - 1).astype(np.int64)
        for j in range(B):
            sel = b == j
            bin_counts[j] = int(sel.sum()), int(sp[sel].sum())
            bin_sum[j] = math.fsum(sk[sel].astype(np.float64))
            bin_abs[j] = math.fsum(np.abs(sk[sel].astype(np.float64)))
    return {"order": order, "cum_pos": cum, "tie_end": tie, "counts": counts, "values": values, "scale": scale,
            "quant": quant, "bin_counts": bin_counts, "bin_sum": bin_sum, "bin_abs": bin_abs}


def rank_metrics(key, flags, thr=None, gammas=(), bins=0, bin_range=(0.0, 1.0), variant=""):
    """Every column of key [m][n] / flags [m][n]: the dict of column() with a leading axis m."""
    key = np.atleast_2d(np.asarray(key, np.float32))
    flags = np.atleast_2d(np.asarray(flags, np.uint8))
    thr = np.full(len(key), np.nan, np.float32) if thr is None else np.asarray(thr, np.float32)
    cols = [column(key[j], flags[j], thr[j], gammas, bins, bin_range, variant) for j in range(len(key))]
    return {name: np.stack([c[name] for c in cols]) for name in cols[0]}


def value_bound(ref):
    """The bound of each double against any order of summation: (M + 4) 2^-53 sum |terms| (KEY_MIN / KEY_MAX and, up to
    its one division, AUROC are exact: the same bound with their own size is generous)."""
    M = ref["counts"][:, C_MEMBERS].astype(np.float64)[:, None]
    return (M + 4) * U * ref["scale"]


def bin_bound(ref):
    M = ref["counts"][:, C_MEMBERS].astype(np.float64)[:, None]
    return (M + 4) * U * ref["bin_abs"]


def eval_columns(score, probs, pred, labels=None):
    """dad_rank_eval_columns: key [10][n] float32 and flags [10][n] uint8 of an evaluated split."""
    score = np.asarray(score, np.float32)
    probs = np.asarray(probs, np.float32)
    pred = np.asarray(pred, np.int64)
    n = len(score)
    have = labels is not None
    y = np.asarray(labels, np.int64) if have else np.zeros(n, np.int64)
    inside = (pred >= 0) & (pred < 4) & (y >= 0) & (y < 4)
    right = inside & (pred == y) & have
    key = np.zeros((10, n), np.float32)
    flags = np.zeros((10, n), np.uint8)
    key[0], key[5] = score, probs.max(axis=1)
    flags[0] = flags[5] = inside * MEMBER + right * POSITIVE
    for c in range(4):
        is_c = inside & (y == c) & have
        key[1 + c], key[6 + c] = score, probs[:, c]
        flags[1 + c] = (inside & (pred == c)) * MEMBER + is_c * POSITIVE
        flags[6 + c] = inside * MEMBER + is_c * POSITIVE
    return key, flags


def risk_coverage(col):
    """(coverage, risk) at the tie ends of a column() dict."""
    M = int(col["counts"][C_MEMBERS])
    te = np.nonzero(col["tie_end"][:M])[0]
    taken = (te + 1).astype(np.float64)
    return taken / max(M, 1), (taken - col["cum_pos"][te]) / taken


def roc_points(col):
    """(fpr, tpr) at the tie ends of a column() dict."""
    M, P = int(col["counts"][C_MEMBERS]), int(col["counts"][C_POSITIVES])
    te = np.nonzero(col["tie_end"][:M])[0]
    tp = col["cum_pos"][te].astype(np.float64)
    return (te + 1 - tp) / max(M - P, 1), tp / max(P, 1)
