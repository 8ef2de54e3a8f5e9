"""tests/knn_ref.py against scikit-learn 1.7.2 on tie-free inputs, the fixture tests/golden/eval_knn.npz, and the two
input conditions of the GPU tests' float cases (few ambiguous rows, few possible rank changes), asserted from the
restatement alone."""
import functools
import os

import numpy as np
import pytest

import knn_ref as kr

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "eval_knn.npz")
CASES = (37, 65, 129)


@functools.lru_cache(None)
def _synth(n):
    emb, labels = kr.synthetic(n, 200 + n)
    return emb, labels, kr.pair_d2(emb)


@pytest.mark.parametrize("n", [127, 257, 1100])
@pytest.mark.parametrize("k", [1, 5, 15])
def test_knn_equals_sklearn_brute(n, k):
    from sklearn.neighbors import NearestNeighbors
    emb, _, D = _synth(n)
    idx, d2 = kr.knn_ref(emb, k, D=D)
    dist, want = NearestNeighbors(n_neighbors=k, algorithm="brute").fit(emb.astype(np.float64)).kneighbors()
    np.testing.assert_array_equal(idx, want)
    np.testing.assert_allclose(d2, dist ** 2, rtol=1e-9)
    assert (np.diff(d2, axis=1) >= 0).all()


def test_vote_equals_sklearn_neighbours_then_mode():
    from sklearn.neighbors import KNeighborsClassifier
    emb, labels, D = _synth(257)
    idx, _ = kr.knn_ref(emb, 5, D=D)
    pred, block = kr.vote_ref(idx, labels)
    nb = KNeighborsClassifier(n_neighbors=5, algorithm="brute").fit(emb.astype(np.float64), labels) \
        .kneighbors(return_distance=False)
    want = np.array([np.bincount(labels[r], minlength=4).argmax() for r in nb])
    np.testing.assert_array_equal(pred, want)
    cm = block[:16].reshape(4, 4)
    assert cm.sum() == 257 == block[kr.KV_QUERIES] and block[kr.KV_NO_VOTE] == 0 and not block[16:32].any()
    assert np.trace(cm) == int((want == labels).sum())


def test_trustworthiness_equals_sklearn():
    from sklearn.manifold import trustworthiness
    emb, _, D = _synth(257)
    Y = kr.pca_map(emb)
    for k in (1, 5, 15):
        got = kr.trustworthiness_ref(emb, Y, k, D=D)
        want = trustworthiness(emb.astype(np.float64), Y.astype(np.float64), n_neighbors=k)
        assert abs(got["trustworthiness"] - want) <= 1e-12, (k, got["trustworthiness"], want)
        assert got["penalty_sum"] == int(got["penalty"].sum())


def test_groups_modes_and_padding():
    emb, _, D = _synth(127)
    group = np.arange(127) % 3
    group[[5, 70]] = -1
    for mode in (kr.SAME, kr.OTHER):
        idx, d2 = kr.knn_ref(emb, 5, group, mode, D=D)
        assert (idx[[5, 70]] == -1).all() and np.isinf(d2[[5, 70]]).all()
        rows = np.where(group >= 0)[0]
        assert not np.isin(idx[rows], [5, 70]).any()
        same = group[idx[rows]] == group[rows][:, None]
        assert same.all() if mode == kr.SAME else not same.any()
    one = np.array([0, 1, 1, 1])
    idx, d2 = kr.knn_ref(emb[:4], 5, one, kr.SAME)
    assert (idx[0] == -1).all() and (idx[1:, :2] >= 0).all() and (idx[1:, 2:] == -1).all() and np.isinf(d2[1:, 2:]).all()
    pred, block = kr.vote_ref(idx, np.array([0, 1, 2, 3]), one)
    assert pred[0] == -1 and block[kr.KV_NO_VOTE] == 1 and block[kr.KV_QUERIES + 1] == 3


@pytest.mark.parametrize("n", CASES)
def test_fixture_is_the_restatement(n):
    g = np.load(GOLDEN)
    key, k = "n%d_" % n, int(g["k"])
    emb, labels, Y = g[key + "emb"], g[key + "labels"], g[key + "Y"]
    assert len(np.unique(emb, axis=0)) == n
    D = kr.pair_d2(emb)
    idx, d2 = kr.knn_ref(emb, k, D=D)
    np.testing.assert_array_equal(idx, g[key + "nn_idx"])
    np.testing.assert_allclose(d2, g[key + "nn_d2"], rtol=1e-9)
    np.testing.assert_array_equal(kr.vote_ref(idx, labels)[0], g[key + "pred"])
    assert abs(kr.trustworthiness_ref(emb, Y, k, D=D)["trustworthiness"] - float(g[key + "trustworthiness"])) <= 1e-12


def _float_inputs():
    g = np.load(GOLDEN)
    for n in CASES:
        yield "fixture n=%d" % n, g["n%d_emb" % n], g["n%d_Y" % n], (int(g["k"]),)
    for name, n, seed in kr.FLOAT_CASES:
        emb, _ = kr.synthetic(n, seed)
        yield name, emb, kr.pca_map(emb), kr.FLOAT_KS


def test_input_conditions_of_the_gpu_float_cases():
    """At most 2 % of rows ambiguous (257 rows at k = 32: the stated ceiling) and at most 1 % of the n k (row, map
    neighbour) pairs open to a rank change, for every float input tests/test_gpu_knn.py compares lists and penalty
    sums on, under the bound that file asserts."""
    for name, emb, Y, ks in _float_inputs():
        n = len(emb)
        D = kr.pair_d2(emb)
        for k in ks:
            amb = int(kr.ambiguous_rows(D, k, kr.D2_BOUND).sum())
            assert amb <= kr.ambiguous_limit(n, k) * n, (name, k, amb)
            a = kr.rank_changes(D, kr.map_neighbours(Y, k, np.float32), kr.D2_BOUND)
            assert a <= kr.RANK_LIMIT * n * k, (name, k, a)


def test_input_condition_of_the_large_and_the_small_cases():
    for (_, n, seed), k in [(kr.LARGE_CASE, kr.LARGE_K)] + [(c, kr.SMALL_K) for c in kr.SMALL_CASES]:
        emb, _ = kr.synthetic(n, seed)
        amb = int(kr.ambiguous_rows(kr.pair_d2(emb), k, kr.D2_BOUND).sum())
        assert amb <= kr.AMBIGUOUS_LIMIT * n, (n, amb)
