"""Writes tests/golden/eval_tsne.npz: scikit-learn 1.7.2's exact t-SNE on three seeded cases, and what rounding alone
does to it, for tests/test_tsne_ref_cpu.py and tests/test_gpu_tsne.py.

Each case: n = 65 (perplexity 5), 129 or 257 (perplexity 30) post-ReLU-like embeddings 0.5 + 0.1 |N(0, 1)| plus a
class offset, with one exact duplicate of a row, and a seeded Y0 = 1e-4 N(0, 1).  Stored per case (prefix n<n>_):

  emb, dup, perplexity, y0
  p                     scikit-learn's _joint_probabilities of the float64 distances (n = 65, 129 only, for size)
  kl0, grad0            scikit-learn's _kl_divergence at y0 with exaggeration 12
  ylate, kl1, grad1     the embedding TSNE(method='exact', init=y0) ends with, and _kl_divergence there, exaggeration 1
  kl_final, n_iter      that run's kl_divergence_ and n_iter_
  pca                   scikit-learn's init='pca' embedding (randomized solver, random_state 42)
  traj5                 the float64 restatement's Y after 5 iterations from y0 (tests/tsne_ref.py)
  dev_p                 float32 restatement against float64, max |P32 - P| / row maximum
  dev_p_rel             the same, relative, over the entries above 1e-3 of the matrix's maximum
  dev_h                 float32 restatement: max |H_i - log(perplexity)| recomputed in float64 from its beta
  dev_traj5             float32 restatement against traj5, max |dY| / max |Y|
  kl_final_f32          the float64 KL of the final Y of eight float32 restatement runs from y0 (1 + 1e-6 N(0, 1))
  kl_explore            the float64 KL (exaggeration 1) after the 250 exploration iterations

The float32 restatement is the device's arithmetic on the CPU: Gram-form float32 distances on centred rows, a double
search on them, P rounded to float32, float32 forces and updates.  Its deviations are what rounding alone does; the
GPU tests' bounds are built from them.  Generated with scikit-learn 1.7.2:

    python tests/golden/gen_tsne_golden.py

(The eval_ prefix keeps the file out of tests/goldens.py's list of step fixtures.)
"""
import os
import sys

import numpy as np
from scipy.spatial.distance import squareform
from sklearn.decomposition import PCA
from sklearn.manifold import TSNE, _t_sne

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import tsne_ref as R      # noqa: E402

CASES = ((65, 5.0, 301), (129, 30.0, 302), (257, 30.0, 303))       # n, perplexity, seed


def make_case(n, seed):
    rs = np.random.RandomState(seed)
    labels = rs.randint(0, 4, n)
    offsets = 0.08 * rs.standard_normal((4, 256))
    emb = (0.5 + 0.1 * np.abs(rs.standard_normal((n, 256))) + offsets[labels]).astype(np.float32)
    src, dst = rs.permutation(n)[:2]
    emb[dst] = emb[src]
    y0 = (1e-4 * rs.standard_normal((n, 2))).astype(np.float32)
    return emb, np.array([src, dst], dtype=np.int64), y0


def main():
    out = {}
    for n, perplexity, seed in CASES:
        emb, dup, y0 = make_case(n, seed)
        key = "n%d_" % n
        D = R.sq_distances(emb)
        P, _ = R.joint_probabilities(D, perplexity)
        Psk = squareform(_t_sne._joint_probabilities(D.astype(np.float32), perplexity, 0))
        out[key + "emb"], out[key + "dup"], out[key + "y0"] = emb, dup, y0
        out[key + "perplexity"] = np.float64(perplexity)
        if n <= 129:
            out[key + "p"] = Psk
        kl0, g0 = _t_sne._kl_divergence(y0.astype(np.float64).ravel(), squareform(Psk) * 12.0, 1.0, n, 2)
        ts = TSNE(n_components=2, perplexity=perplexity, max_iter=1000, init=y0, learning_rate="auto", method="exact",
                  random_state=42)
        ylate = ts.fit_transform(emb).astype(np.float32)
        kl1, g1 = _t_sne._kl_divergence(ylate.astype(np.float64).ravel(), squareform(Psk), 1.0, n, 2)
        out[key + "kl0"], out[key + "grad0"] = np.float64(kl0), g0.reshape(n, 2)
        out[key + "ylate"], out[key + "kl1"], out[key + "grad1"] = ylate, np.float64(kl1), g1.reshape(n, 2)
        out[key + "kl_final"], out[key + "n_iter"] = np.float64(ts.kl_divergence_), np.int64(ts.n_iter_)
        pca = PCA(n_components=2, svd_solver="randomized", random_state=42)
        yp = pca.fit_transform(emb).astype(np.float32, copy=False)
        out[key + "pca"] = yp / np.std(yp[:, 0]) * 1e-4
        # what rounding alone does
        P32, beta32 = R.joint_probabilities_f32(emb, perplexity)
        out[key + "dev_p"] = np.float64(R.p_deviation(P32, P))
        big = P > 1e-3 * P.max()
        out[key + "dev_p_rel"] = np.float64((np.abs(P32 - P)[big] / P[big]).max())
        out[key + "dev_h"] = np.float64(np.abs(R.entropy_of_rows(D, beta32) - np.log(perplexity)).max())
        t64 = R.descend(P, y0, max_iter=5, snapshots=(5,))["snapshots"][5]
        t32 = R.descend(P32, y0, max_iter=5, dtype=np.float32, snapshots=(5,))["snapshots"][5]
        out[key + "traj5"] = t64
        out[key + "dev_traj5"] = np.float64(np.abs(t32 - t64).max() / np.abs(t64).max())
        if n >= 129:
            rs = np.random.RandomState(seed + 1000)
            finals = []
            for _ in range(8):
                yp0 = (y0 * (1.0 + 1e-6 * rs.standard_normal(y0.shape))).astype(np.float32)
                yf = R.descend(P32, yp0, dtype=np.float32)["Y"]
                finals.append(R.kl_and_gradient(P, yf, sums=False)["kl"])
            out[key + "kl_final_f32"] = np.array(finals)
            ye = R.descend(P32, y0, max_iter=250, dtype=np.float32)["Y"]
            out[key + "kl_explore"] = np.float64(R.kl_and_gradient(P, ye, sums=False)["kl"])
        print(n, {k[len(key):]: (v if np.ndim(v) == 0 else (v if v.size <= 8 else v.shape)) for k, v in out.items()
                  if k.startswith(key) and k[len(key):] not in ("emb", "y0")})
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "eval_tsne.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
