"""float64 NumPy restatement of what dad_eval_models (include/dad.h, "several networks on one split") builds from
the K models' float32 probabilities and the labels: the mean-ensemble chain, the vote, the DAD_EM_* counts block and
the float64 sums.  The per-model forward is not restated here: the GPU tests hold it to dad_eval_split bit for bit.

`variant` selects a deliberately wrong reference (the CPU tests show that each differs from the right one on the
cases the GPU tests use, so the comparison can fail):
    vote_tie_high         ties of the vote go to the highest class
    only_transposed       ONLY[a][b] counts "b right and a wrong"
    disagree_labelled     DISAGREE counts labelled utterances only
"""
import numpy as np

VARIANTS = ("vote_tie_high", "only_transposed", "disagree_labelled")
MEMBERS = 10


def norm_weights(weights, K):
    """w^_k = (float)(w_k / sum_j w_j), the quotient in double, as float32"""
    w = np.ones(K, np.float64) if weights is None else np.asarray(weights, np.float64)
    total = 0.0
    for v in w:
        total += float(v)
    return (w / total).astype(np.float32)


def ensemble_chain32(probs, wn):
    """The device's definition in its own arithmetic: e = 0; e = fmaf(w^_k, p_k, e) in k order, float32.  The product
    of two float32 is exact in float64 and |e| <= 1, so rounding the float64 sum once to float32 is the fused
    operation up to double rounding, which the GPU tests' bound (K * 2^-24) covers."""
    e = np.zeros(probs.shape[1:], np.float32)
    for k in range(probs.shape[0]):
        e = (wn[k].astype(np.float64) * probs[k].astype(np.float64) + e.astype(np.float64)).astype(np.float32)
    return e


def ensemble64(probs, wn):
    """sum_k w^_k p_k in float64, k order"""
    e = np.zeros(probs.shape[1:], np.float64)
    for k in range(probs.shape[0]):
        e = e + wn[k].astype(np.float64) * probs[k].astype(np.float64)
    return e


def certainty64(p, use_entropy=True):
    """DACPManager.calculate_certainty_scores on probabilities p [..., 4] in float64"""
    p = np.asarray(p, np.float64)
    pmax = p.max(-1)
    if not use_entropy:
        return pmax
    ent = -(p * np.log2(p + 1e-8)).sum(-1)
    return pmax * (1.0 - ent / 2.0)


def vote(pred, variant=None):
    """(votes [n, 4], vote_pred [n]) of the models' predictions pred [K, n]: most votes, ties to the lowest class"""
    votes = np.stack([(pred == c).sum(0) for c in range(4)], 1).astype(np.int32)
    if variant == "vote_tie_high":
        vp = 3 - np.argmax(votes[:, ::-1], 1)
    else:
        vp = np.argmax(votes, 1)
    return votes, vp.astype(np.int64)


def n_correct(pred, labels):
    lab = (labels >= 0) & (labels < 4)
    return np.where(lab, (pred == labels[None]).sum(0), -1).astype(np.int32)


def terms(p, labels):
    """Per-utterance float64 terms of the sums from float32 probabilities p [n, 4]: (entropy, nll, brier); nll and
    brier are 0 on unlabelled utterances."""
    p = np.asarray(p).astype(np.float64)
    lab = (labels >= 0) & (labels < 4)
    with np.errstate(divide="ignore", invalid="ignore"):
        ent = -np.where(p > 0, p * np.log(np.where(p > 0, p, 1.0)), 0.0).sum(1)
    y = np.where(lab, labels, 0)
    py = p[np.arange(len(p)), y]
    with np.errstate(divide="ignore"):
        nll = np.where(lab, -np.log(py), 0.0)
    onehot = np.zeros_like(p)
    onehot[np.arange(len(p)), y] = lab
    brier = np.where(lab, ((p - onehot) ** 2).sum(1), 0.0)
    return ent, nll, brier


def block(L, probs, pred, score, labels, weights=None, use_entropy=True, bad=None, variant=None):
    """The result of dad_eval_models restated from the device's own per-model outputs: probs [K, n, 4] float32,
    pred [K, n], score [K, n] float32, labels [n] (None: unlabelled).  L is the binding module (its EM_* slots).
    Returns {'counts' [EM_COUNTS] int64, 'sums' [EM_SUMS] float64, 'sums_abs' (the sum of |terms| per slot),
    'ens32', 'ens64' [n, 4], 'ens_pred', 'ens_score64', 'votes', 'vote_pred', 'n_correct', 'member_pred' [K+2, n]}."""
    probs = np.asarray(probs, np.float32)
    pred = np.asarray(pred, np.int64)
    K, n = pred.shape
    labels = np.full(n, -1, np.int64) if labels is None else np.asarray(labels, np.int64)
    lab = (labels >= 0) & (labels < 4)
    wn = norm_weights(weights, K)
    ens32 = ensemble_chain32(probs, wn)
    ens64 = ensemble64(probs, wn)
    ens_pred = np.argmax(ens32, 1).astype(np.int64)
    votes, vote_pred = vote(pred, variant)
    nc = n_correct(pred, labels)
    mp = np.concatenate([pred, ens_pred[None], vote_pred[None]])
    M = K + 2
    counts = np.zeros(L.EM_COUNTS, np.int64)
    for m in range(M):
        cm = np.zeros((4, 4), np.int64)
        np.add.at(cm, (labels[lab], mp[m][lab]), 1)
        counts[L.EM_CONF + 16 * m:L.EM_CONF + 16 * (m + 1)] = cm.reshape(-1)
    right = (mp == labels[None]) & lab[None]
    for a in range(M):
        for b in range(M):
            dis = mp[a] != mp[b]
            if variant == "disagree_labelled":
                dis = dis & lab
            counts[L.EM_DISAGREE + a * MEMBERS + b] = dis.sum()
            only = right[a] & (lab & ~right[b] if a != b else True)
            if variant == "only_transposed":
                only = right[b] & (lab & ~right[a] if a != b else True)
            counts[L.EM_ONLY + a * MEMBERS + b] = only.sum()
    counts[L.EM_HIST:L.EM_HIST + K + 1] = np.bincount(nc[lab], minlength=K + 1)
    counts[L.EM_N], counts[L.EM_N_LABELLED], counts[L.EM_N_SKIPPED], counts[L.EM_K] = n, lab.sum(), (~lab).sum(), K
    if bad is not None:
        counts[L.EM_NONFINITE:L.EM_NONFINITE + K] = np.asarray(bad).reshape(K, n).astype(bool).sum(1)
    sums = np.zeros(L.EM_SUMS, np.float64)
    sums_abs = np.zeros(L.EM_SUMS, np.float64)
    ens_score64 = certainty64(ens32, use_entropy)
    for m in range(K + 1):
        p = probs[m] if m < K else ens32
        sc = np.asarray(score[m], np.float64) if m < K else None
        ent, nll, brier = terms(p, labels)
        for slot, t in ((L.EM_SUM_SCORE, sc), (L.EM_SUM_ENTROPY, ent), (L.EM_SUM_NLL, nll), (L.EM_SUM_BRIER, brier)):
            if t is None:
                continue                  # the ensemble's score sum is checked against the device's own ens_score
            sums[slot + m] = t.sum()
            sums_abs[slot + m] = np.abs(t).sum()
    return {"counts": counts, "sums": sums, "sums_abs": sums_abs, "ens32": ens32, "ens64": ens64,
            "ens_pred": ens_pred, "ens_score64": ens_score64, "votes": votes, "vote_pred": vote_pred,
            "n_correct": nc, "member_pred": mp, "wn": wn}


def softmax32(z):
    """float32 softmax rows (for CPU cases that need plausible probabilities)"""
    z = np.asarray(z, np.float32)
    e = np.exp(z - z.max(-1, keepdims=True))
    return (e / e.sum(-1, keepdims=True)).astype(np.float32)


def cpu_case(K, n=41, seed=5):
    """A seeded case for the CPU tests: (probs [K, n, 4] f32, pred, score, labels with two unlabelled entries).  The
    models share a per-utterance signal, so they agree often but not always, and the vote has ties."""
    rs = np.random.RandomState(seed + 17 * K)
    base = rs.standard_normal((n, 4))
    z = base[None] + 1.2 * rs.standard_normal((K, n, 4))
    probs = softmax32(z)
    pred = probs.argmax(-1).astype(np.int64)
    score = certainty64(probs).astype(np.float32)
    labels = base.argmax(1).astype(np.int64)
    labels[[3, n - 2]] = -1
    return probs, pred, score, labels
