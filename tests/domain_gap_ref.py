"""NumPy restatements of the clean-noisy domain gap of include/dad.h (dad_domain_gap): ECDALoss (I/utils.py:510-652)
on whole sets of embeddings.

  domain_gap_ref      float64, squared distances from the differences x_i - x_j, row-chunked (no [m, m, 256]
                      temporary, no Gram identity)
  gaussian_terms_f32  _gaussian_kernel's three terms and bandwidth in float32 from Gram-form distances on centred
                      rows: the device's arithmetic on the CPU, for judging what rounding alone does
"""
import numpy as np

NUM_CLASSES = 4
KERNEL_NUM, KERNEL_MUL = 5, 2.0


def _sqdist(x, rows=32):
    """[m, m] float64 |x_i - x_j|^2 from the differences, `rows` rows at a time; the diagonal is exactly 0."""
    m = x.shape[0]
    d = np.empty((m, m))
    for i0 in range(0, m, rows):
        d[i0:i0 + rows] = ((x[i0:i0 + rows, None, :] - x[None, :, :]) ** 2).sum(2)
    return d


def gaussian_terms(xs, xt, ws, wt):
    """_gaussian_kernel (I/utils.py:521-563) in float64: (term_ss, term_tt, term_st, bandwidth), bandwidth the
    smallest of the five (sum(L2) / (m^2 - m) / kernel_mul^(kernel_num // 2))."""
    ns, m = len(xs), len(xs) + len(xt)
    d = _sqdist(np.concatenate([xs, xt]))
    bw = d.sum() / (m * m - m) / KERNEL_MUL ** (KERNEL_NUM // 2) if m > 1 else 0.0
    k = sum(np.exp(-d / (bw * KERNEL_MUL ** b + 1e-8)) for b in range(KERNEL_NUM))
    ss = (k[:ns, :ns] * np.outer(ws, ws)).sum() / (ws.sum() ** 2 + 1e-8)
    tt = (k[ns:, ns:] * np.outer(wt, wt)).sum() / (wt.sum() ** 2 + 1e-8)
    st = (k[:ns, ns:] * np.outer(ws, wt)).sum() / (ws.sum() * wt.sum() + 1e-8)
    return float(ss), float(tt), float(st), float(bw)


def gaussian_terms_f32(xs, xt, ws, wt, mu):
    """The same in float32 as the device forms it: rows centred on `mu` (float32), D = max(|a_i|^2 + |a_j|^2 -
    2 a_i.a_j, 0) with a zero diagonal, the bandwidth from float32 row sums added in float64, float32 coefficients
    -log2(e) / (bw 2^b + 1e-8), float32 exponentials and row sums, everything across rows in float64."""
    f = np.float32
    a = np.concatenate([xs, xt]).astype(f) - np.asarray(mu, f)
    ns, m = len(xs), len(a)
    g = a @ a.T
    nrm = np.diag(g).copy()
    d = np.maximum((nrm[:, None] + nrm[None, :]) - f(2) * g, f(0)).astype(f)
    np.fill_diagonal(d, 0)
    bw = float(d.sum(1, dtype=f).astype(np.float64).sum()) / (m * m - m) / 4.0 if m > 1 else 0.0
    k = np.zeros((m, m), f)
    for b in range(KERNEL_NUM):
        k += np.exp2(d * f(-1.4426950408889634 / (bw * 2.0 ** b + 1e-8))).astype(f)
    w = np.concatenate([ws, wt]).astype(f)
    kw = k * w[None, :]
    row = lambda cols: kw[:, cols].sum(1, dtype=f).astype(np.float64) * w.astype(np.float64)
    rs, rt = row(slice(0, ns)), row(slice(ns, m))
    sws, swt = float(np.asarray(ws, np.float64).sum()), float(np.asarray(wt, np.float64).sum())
    return (float(rs[:ns].sum() / (sws * sws + 1e-8)), float(rt[ns:].sum() / (swt * swt + 1e-8)),
            float(rt[:ns].sum() / (sws * swt + 1e-8)), bw)


def domain_gap_ref(emb, labels, domain, weights=None, class_weights=None, lam=1.0, gamma=0.1, delta=0.1,
                   terms=gaussian_terms):
    """The dict of evaluate.domain_gap (without 'block') in float64 from emb [n, 256], labels [n], domain [n]
    (0 = clean, else noisy), weights [n] (None: ones; the clean rows' are used as given), class_weights [4] (None:
    ones).  Rows with a label outside [0, 4) take no part."""
    x = np.asarray(emb, np.float64)
    y = np.asarray(labels, np.int64).reshape(-1)
    dom = np.asarray(domain).reshape(-1) != 0
    n = len(y)
    w = np.ones(n) if weights is None else np.asarray(weights, np.float64).reshape(-1)
    cw = np.ones(NUM_CLASSES) if class_weights is None else np.asarray(class_weights, np.float64)
    part = (y >= 0) & (y < NUM_CLASSES)
    src = [np.where(part & ~dom & (y == c))[0] for c in range(NUM_CLASSES)]
    tgt = [np.where(part & dom & (y == c))[0] for c in range(NUM_CLASSES)]
    zeros = lambda: [0.0] * NUM_CLASSES
    per = {k: zeros() for k in ("bandwidth", "term_ss", "term_tt", "term_st", "mmd", "compactness", "centroid_shift")}
    per["gate"] = [len(src[c]) >= 2 and len(tgt[c]) >= 2 for c in range(NUM_CLASSES)]
    per["n_clean"] = [len(s) for s in src]
    per["n_noisy"] = [len(t) for t in tgt]
    per["weight_noisy"] = [float(w[t].sum()) for t in tgt]
    per["attention"] = [float(v) for v in np.exp(lam * (cw.mean() - cw))]
    cents = [x[t].mean(0) for t in tgt if len(t)]
    pairs = [np.sqrt(((cents[a] - cents[b]) ** 2).sum()) for a in range(len(cents)) for b in range(a + 1, len(cents))]
    rep = -float(np.mean(pairs)) if pairs else 0.0
    loss, mmds = 0.0, []
    for c in range(NUM_CLASSES):
        if not per["gate"][c]:
            continue
        ss, tt, st, bw = terms(x[src[c]], x[tgt[c]], w[src[c]], w[tgt[c]])
        cen = x[tgt[c]].mean(0)
        per["bandwidth"][c], per["term_ss"][c], per["term_tt"][c], per["term_st"][c] = bw, ss, tt, st
        per["mmd"][c] = (ss + tt) - 2.0 * st
        per["compactness"][c] = float(((x[tgt[c]] - cen) ** 2).sum(1).mean())
        per["centroid_shift"][c] = float(np.sqrt(((x[src[c]].mean(0) - cen) ** 2).sum()))
        loss += per["attention"][c] * ((per["mmd"][c] + gamma * per["compactness"][c]) + delta * rep)
        mmds.append(per["mmd"][c])
    s_all, t_all = np.where(part & ~dom)[0], np.where(part & dom)[0]
    glob = {"gate": len(s_all) >= 2 and len(t_all) >= 2, "bandwidth": 0.0, "term_ss": 0.0, "term_tt": 0.0,
            "term_st": 0.0, "mmd": 0.0}
    if glob["gate"]:
        ss, tt, st, bw = terms(x[s_all], x[t_all], np.ones(len(s_all)), np.ones(len(t_all)))
        glob.update(bandwidth=bw, term_ss=ss, term_tt=tt, term_st=st, mmd=(ss + tt) - 2.0 * st)
    return {"valid": bool(glob["gate"] or any(per["gate"])), "n_clean": len(s_all), "n_noisy": len(t_all),
            "global": glob, "per_class": per, "repulsion": rep, "ecda_loss": float(loss),
            "mmd_class_mean": float(np.mean(mmds)) if mmds else 0.0,
            "nonfinite": int((~np.isfinite(x[part])).any(1).sum())}
