"""Writes tests/golden/eval_cluster_metrics.npz: scikit-learn's silhouette_samples, silhouette_score and
calinski_harabasz_score (float32 input, as calculate_cluster_metrics feeds it, I/iemocap_plot_tsne.py:
390-398) on three seeded cases, for tests/test_cluster_ref_cpu.py and tests/test_gpu_cluster.py.

Each case: n = 37, 65 or 129 post-ReLU-like embeddings 0.5 + 0.1 |N(0, 1)| plus a class offset, three of
the four classes present, one of them with a single member, two rows labelled -1 (they take no part:
scikit-learn sees the labelled rows only, and their sample value is recorded as 0), and one exact
duplicate of a row inside a class.  Generated with scikit-learn 1.7.2:

    python tests/golden/gen_cluster_golden.py

(The eval_ prefix keeps the file out of tests/goldens.py's list of step fixtures.)
"""
import os

import numpy as np
from sklearn.metrics import calinski_harabasz_score, silhouette_samples, silhouette_score

CASES = ((37, 101, 2, 3), (65, 102, 0, 1), (129, 103, 3, 0))     # n, seed, absent class, single-member class


def make_case(n, seed, absent, single):
    rs = np.random.RandomState(seed)
    big = [c for c in range(4) if c not in (absent, single)]
    labels = np.array([big[i % 2] for i in range(n)], dtype=np.int64)
    rs.shuffle(labels)
    spots = rs.permutation(n)
    labels[spots[0]] = single
    labels[spots[1:3]] = -1
    offsets = 0.08 * rs.standard_normal((4, 256))
    emb = 0.5 + 0.1 * np.abs(rs.standard_normal((n, 256))) + offsets[np.maximum(labels, 0)]
    emb = emb.astype(np.float32)
    src, dst = [i for i in spots[3:] if labels[i] == big[0]][:2]
    emb[dst] = emb[src]
    return emb, labels, np.array([src, dst], dtype=np.int64)


def main():
    out = {}
    for n, seed, absent, single in CASES:
        emb, labels, dup = make_case(n, seed, absent, single)
        keep = labels >= 0
        sil = np.zeros(n, dtype=np.float64)
        sil[keep] = silhouette_samples(emb[keep], labels[keep])
        key = "n%d_" % n
        out[key + "emb"] = emb
        out[key + "labels"] = labels
        out[key + "dup"] = dup
        out[key + "silhouette_samples"] = sil
        out[key + "silhouette_score"] = np.float64(silhouette_score(emb[keep], labels[keep]))
        out[key + "calinski_harabasz_score"] = np.float64(calinski_harabasz_score(emb[keep], labels[keep]))
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "eval_cluster_metrics.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
