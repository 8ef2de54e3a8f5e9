"""Class-separation scores without a GPU: the float64 restatement (tests/cluster_ref.py) against the
scikit-learn fixture (tests/golden/eval_cluster_metrics.npz), the label configurations the scores are not
defined for, separation_report's arithmetic, and the DAD_CM_* slots of header and binding."""
import os
import re

import numpy as np
import pytest

import dadpkg
from cluster_ref import cluster_ref

PKG = dadpkg.pkg()
E = PKG.evaluate
L = PKG._lib
GOLDEN = os.path.join(dadpkg.ROOT, "tests", "golden", "eval_cluster_metrics.npz")
CASES = (37, 65, 129)
TILE = L.CM_TILE      # (the binding's DAD_CM_* mirror: every test of this file needs the feature)

# Worst gap between the restatement and scikit-learn 1.7.2 (float32 input: float32 distances and centroids
# there) over the three fixture cases, measured when the fixture was generated: 9.14e-8 per sample, 4.73e-8 on the
# silhouette score, 9.54e-8 relative on CH.  The bounds are 10 x that.
SAMPLE_MEASURED, SCORE_MEASURED, CH_REL_MEASURED = 9.14e-8, 4.73e-8, 9.54e-8
SAMPLE_BOUND, SCORE_BOUND, CH_REL_BOUND = 10 * SAMPLE_MEASURED, 10 * SCORE_MEASURED, 10 * CH_REL_MEASURED


@pytest.mark.parametrize("n", CASES)
def test_restatement_reproduces_scikit_learn(n):
    g = np.load(GOLDEN)
    key = "n%d_" % n
    emb, labels = g[key + "emb"], g[key + "labels"]
    assert emb.shape == (n, 256) and emb.dtype == np.float32
    r = cluster_ref(emb, labels)
    # the fixture holds what the issue asks of it
    assert r["valid"] and r["classes_present"] == 3 and sorted(r["class_counts"])[:2] == [0, 1]
    assert int((labels == -1).sum()) == 2 and r["n_labelled"] == n - 2
    i, j = g[key + "dup"]
    assert labels[i] == labels[j] >= 0 and np.array_equal(emb[i], emb[j])
    es = float(np.abs(r["silhouette_samples"] - g[key + "silhouette_samples"]).max())
    sc = abs(r["silhouette_score"] - float(g[key + "silhouette_score"]))
    ch = abs(r["calinski_harabasz_score"] / float(g[key + "calinski_harabasz_score"]) - 1.0)
    print("n=%d: restatement - scikit-learn: sample %.3e  score %.3e  CH rel %.3e" % (n, es, sc, ch))
    assert es <= SAMPLE_BOUND and sc <= SCORE_BOUND and ch <= CH_REL_BOUND
    assert not r["silhouette_samples"][labels < 0].any()
    assert r["silhouette_samples"][labels == r["class_counts"].index(1)] == 0.0      # the single member
    per = [r["silhouette_samples"][labels == c].mean() if r["class_counts"][c] else 0.0 for c in range(4)]
    np.testing.assert_allclose(r["silhouette_per_class"], per, rtol=1e-12, atol=0)


@pytest.mark.parametrize("labels", [
    [1, 1, 1, 1, 1],          # one class only
    [0, 1, 2, 3],             # k = m
    [0, 3],                   # m = 2 with two classes
    [2, -1, 7, 0],            # the same after the unlabelled rows are dropped
    [-1, 4],                  # nothing labelled
], ids=["one_class", "k_equals_m", "m2_k2", "m2_k2_unlabelled", "none"])
def test_invalid_label_configurations(labels):
    emb = np.random.RandomState(5).rand(len(labels), 256).astype(np.float32)
    r = cluster_ref(emb, labels)
    assert r["valid"] is False
    assert r["silhouette_score"] == 0.0 and r["calinski_harabasz_score"] == 0.0
    assert not r["silhouette_samples"].any() and not any(r["silhouette_per_class"])


def test_smallest_valid_and_degenerate_values():
    emb = np.zeros((3, 256), np.float32)
    emb[2, 0] = 2.0
    r = cluster_ref(emb, [0, 0, 1])
    # rows 0, 1 coincide: a = 0, b = 2 -> s = 1; the single member of class 1: s = 0; W = 0 -> CH = 1
    assert r["valid"] and r["silhouette_samples"].tolist() == [1.0, 1.0, 0.0]
    assert r["silhouette_score"] == pytest.approx(2.0 / 3.0) and r["calinski_harabasz_score"] == 1.0
    # every row the same point: max(a, b) = 0 -> s = 0
    r = cluster_ref(np.ones((4, 256), np.float32), [0, 0, 1, 1])
    assert r["valid"] and not r["silhouette_samples"].any() and r["calinski_harabasz_score"] == 1.0


def test_separation_report_arithmetic():
    r = E.separation_from_metrics({"silhouette_score": -0.05, "calinski_harabasz_score": 12.5},
                                  {"silhouette_score": 0.15, "calinski_harabasz_score": 40.0})
    assert r["initial_weights"] == {"silhouette_score": -0.05, "calinski_harabasz_score": 12.5}
    assert r["trained_weights"] == {"silhouette_score": 0.15, "calinski_harabasz_score": 40.0}
    imp = r["improvement"]
    assert imp["silhouette_improvement"] == pytest.approx(0.2, abs=1e-15)
    assert imp["calinski_improvement"] == 27.5
    assert imp["silhouette_percentage"] == pytest.approx(400.0, abs=1e-10)     # over |initial|, as the reference
    z = E.separation_from_metrics((np.float32(0.0), np.float64(0.0)), (0.25, 3.0))
    assert z["improvement"] == {"silhouette_improvement": 0.25, "calinski_improvement": 3.0,
                                "silhouette_percentage": 0.0}
    for block in list(r.values()) + list(z.values()):
        assert all(type(v) is float for v in block.values())


def test_header_slots_equal_the_binding():
    hdr = open(os.path.join(dadpkg.ROOT, "include", "dad.h")).read()
    defs = {k: int(v) for k, v in re.findall(r"^#define DAD_CM_([A-Z_]+) (\d+)", hdr, flags=re.M)}
    names = {"SILHOUETTE", "CH", "VALID", "M", "K", "COUNTS", "SIL_CLASS", "W", "B", "NONFINITE", "SLOTS", "MAX_N",
             "TILE", "MAX_CHUNKS"}
    assert set(defs) == names
    for k, v in defs.items():
        assert getattr(L, "CM_" + k) == v, k
    # the slots tile the block: 4 counts, 4 per-class means
    order = sorted((defs[k], k) for k in names - {"SLOTS", "MAX_N", "TILE", "MAX_CHUNKS"})
    assert [v for v, _ in order] == [0, 1, 2, 3, 4, 5, 9, 13, 14, 15] and defs["SLOTS"] == 16
    assert defs["MAX_N"] >= 2 ** 16 and defs["MAX_N"] & (defs["MAX_N"] - 1) == 0


@pytest.mark.parametrize("n,cus", [(1, 256), (37, 256), (1100, 256), (5531, 256), (5531, 8), (65536, 256), (65536, 304)])
def test_plan_covers_every_column_tile_once(n, cus):
    import ctypes
    PKG.build(verbose=False)
    fn = L.require("dad_cluster_plan", "the plan")
    rt, ch, per = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    assert fn(n, cus, ctypes.byref(rt), ctypes.byref(ch), ctypes.byref(per)) == 0
    assert rt.value == -(-n // L.CM_TILE)
    assert 1 <= ch.value <= min(rt.value, L.CM_MAX_CHUNKS)
    assert (ch.value - 1) * per.value < rt.value <= ch.value * per.value        # every tile once, no empty chunk
    assert L.lib().dad_cluster_workspace_bytes(n) > 0
    assert L.lib().dad_cluster_workspace_bytes(0) == 0 and L.lib().dad_cluster_workspace_bytes(L.CM_MAX_N + 1) == 0
    assert fn(0, cus, ctypes.byref(rt), ctypes.byref(ch), ctypes.byref(per)) == L.E_SHAPE


def test_argument_errors_come_before_any_launch():
    import ctypes
    PKG.build(verbose=False)
    fn = L.require("dad_cluster_metrics", "the test")
    p = ctypes.c_void_p(256)        # never dereferenced: every call below fails its checks first
    for args in ((None, p, 4, p, None, p, None), (p, None, 4, p, None, p, None), (p, p, 4, None, None, p, None),
                 (p, p, 4, p, None, None, None)):
        assert fn(*args) == L.E_ARG
    for n in (0, -3, L.CM_MAX_N + 1):
        assert fn(p, p, n, p, None, p, None) == L.E_SHAPE
