"""Writes tests/golden/eval_knn.npz: scikit-learn 1.7.2's answers for three small splits (n = 37, 65, 129; k = 5).

Per case `n<N>_`: emb [n, 256] float32 (the recipe of the cluster tests under seeds of its own; no duplicate rows),
labels [n] int64, Y [n, 2] float32 (the centred rows on their top two principal axes), and from scikit-learn on the
float64 copies: nn_idx / nn_d2 (NearestNeighbors(algorithm='brute').kneighbors(), the squared distances), pred (the
mode of KNeighborsClassifier's leave-one-out neighbours' labels, smallest class first) and trustworthiness.

    python tests/golden/gen_knn_golden.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
from knn_ref import pca_map, synthetic  # noqa: E402

CASES, K = (37, 65, 129), 5


def main():
    from sklearn.manifold import trustworthiness
    from sklearn.neighbors import KNeighborsClassifier, NearestNeighbors
    out = {}
    for n in CASES:
        emb, labels = synthetic(n, 700 + n)
        assert len(np.unique(emb, axis=0)) == n
        Y = pca_map(emb)
        x = emb.astype(np.float64)
        dist, idx = NearestNeighbors(n_neighbors=K, algorithm="brute").fit(x).kneighbors()
        nb = KNeighborsClassifier(n_neighbors=K, algorithm="brute").fit(x, labels).kneighbors(return_distance=False)
        pred = np.array([np.bincount(labels[r], minlength=4).argmax() for r in nb], dtype=np.int64)
        key = "n%d_" % n
        out.update({key + "emb": emb, key + "labels": labels, key + "Y": Y, key + "nn_idx": idx.astype(np.int32),
                    key + "nn_d2": dist ** 2, key + "pred": pred,
                    key + "trustworthiness": np.float64(trustworthiness(x, Y.astype(np.float64), n_neighbors=K))})
    out["k"] = np.int64(K)
    np.savez(os.path.join(HERE, "eval_knn.npz"), **out)


if __name__ == "__main__":
    main()
