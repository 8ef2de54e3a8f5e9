"""Float64 NumPy restatement of the class-separation scores of include/dad.h (dad_cluster_metrics):
scikit-learn's silhouette and Calinski-Harabasz meaning over the rows with a label in [0, 4), from
direct differences x_i - x_j (no Gram identity, no scikit-learn)."""
import numpy as np

NUM_CLASSES = 4


def cluster_ref(emb, labels):
    """{'silhouette_score', 'calinski_harabasz_score', 'valid', 'n_labelled', 'classes_present',
    'class_counts' [4], 'silhouette_per_class' [4], 'within', 'between', 'silhouette_samples' [n]}.
    An invalid label configuration (classes present outside [2, labelled rows - 1]) gives both scores
    and every sample 0.0; 'within' / 'between' are reported whenever a row is labelled."""
    x = np.asarray(emb, dtype=np.float64)
    y = np.asarray(labels, dtype=np.int64).reshape(-1)
    n = x.shape[0]
    assert y.shape == (n,)
    lab = (y >= 0) & (y < NUM_CLASSES)
    counts = np.array([int(np.sum(lab & (y == c))) for c in range(NUM_CLASSES)])
    m, k = int(counts.sum()), int(np.sum(counts > 0))
    valid = 2 <= k <= m - 1
    sil = np.zeros(n)
    within = between = 0.0
    if m > 0:
        mu = x[lab].sum(0) / m
        for c in range(NUM_CLASSES):
            if counts[c]:
                xc = x[lab & (y == c)]
                mc = xc.sum(0) / counts[c]
                within += float(((xc - mc) ** 2).sum())
                between += counts[c] * float(((mc - mu) ** 2).sum())
    if valid:
        for i in np.where(lab)[0]:
            d = np.sqrt(((x - x[i]) ** 2).sum(1))
            d[i] = 0.0
            c = y[i]
            if counts[c] == 1:
                continue
            a = d[lab & (y == c)].sum() / (counts[c] - 1)
            b = min(d[lab & (y == o)].sum() / counts[o] for o in range(NUM_CLASSES) if o != c and counts[o])
            sil[i] = (b - a) / max(a, b) if max(a, b) > 0 else 0.0
    per_class = [float(sil[lab & (y == c)].sum() / counts[c]) if valid and counts[c] else 0.0
                 for c in range(NUM_CLASSES)]
    if valid:
        score = float(sil[lab].sum() / m)
        ch = 1.0 if within == 0.0 else between * (m - k) / (within * (k - 1.0))
    else:
        score = ch = 0.0
    return {"silhouette_score": score, "calinski_harabasz_score": float(ch), "valid": bool(valid), "n_labelled": m,
            "classes_present": k, "class_counts": counts.tolist(), "silhouette_per_class": per_class,
            "within": within, "between": between, "silhouette_samples": sil}
