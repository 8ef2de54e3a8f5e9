"""Class-separation scores on the MI355X (evaluate.cluster_metrics* + csrc/cluster.hip) against the float64
restatement tests/cluster_ref.py (computed once per input on the CPU) and the scikit-learn fixture
tests/golden/eval_cluster_metrics.npz: the fixture cases, the tile edges and the chunked summation, the smallest
inputs, unlabelled / permuted rows, poison and padding, the store path, graph capture and determinism."""
import functools
import os
import warnings

import numpy as np
import pytest
import torch

import dadpkg
import gpu_harness as gh
from cluster_ref import cluster_ref
from oracle import data_oracle as do

pytestmark = pytest.mark.gpu
PKG = dadpkg.pkg()
D = PKG.data
E = PKG.evaluate
T = PKG._lib.CM_TILE
GOLDEN = os.path.join(dadpkg.ROOT, "tests", "golden", "eval_cluster_metrics.npz")
CASES = (37, 65, 129)
DTYPES = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}

# Worst |kernel - cluster_ref| measured on the MI355X over the inputs this file compares with cluster_ref.  What is
# left is the fp32 Gram form's cancellation in |a|^2 + |b|^2 - 2 a.b on the centred rows (uncentred rows gave
# 1.0e-5 per sample on the same inputs).  Per input: sample / score / per-class mean / CH, W, B relative
#   fixture n=37   2.33e-7  7.3e-9  4.2e-8  4.4e-16      fixture n=65   1.62e-7  1.7e-9  2.3e-8  6.7e-16
#   fixture n=129  1.91e-7  3.2e-9  5.8e-9  4.4e-16      n=3 [0, 0, 1]  4.9e-8   2.7e-8  4.1e-8  2.4e-15
#   n=127          2.28e-7  1.2e-8  1.8e-8  2.2e-16      n=128          2.16e-7  9.5e-9  4.5e-8  0
#   n=129          2.15e-7  2.2e-8  3.8e-8  4.4e-16      n=257          2.63e-7  8.8e-9  5.9e-8  4.4e-16
# (each the worst of 1 chunk, 3 chunks and the planner's count).  The score of n=3 is a mean of three samples, so it
# errs like one; CH, W and B are double arithmetic on the fp32 inputs.  The kernel is deterministic; the factor 2
# guards against a recompilation's summation order.
MEASURED_SAMPLE = 2.633e-7
MEASURED_SCORE = 2.746e-8
MEASURED_CLASS = 5.878e-8
MEASURED_CH_REL = 2.442e-15
# The two exact-duplicate rows of each fixture case.  |a|^2 is the diagonal of the pair kernel's own Gram block (the
# same MFMA chain on the same operands), so their mutual distance comes out as exactly 0, not as sqrt(eps) |a|, and
# they err like any other row: 9.58e-8, 7.84e-8, 6.68e-8 for n = 37, 65, 129.
MEASURED_DUP = 9.582e-8
SAMPLE_BOUND, SCORE_BOUND, CLASS_BOUND = 2 * MEASURED_SAMPLE, 2 * MEASURED_SCORE, 2 * MEASURED_CLASS
CH_REL_BOUND, DUP_BOUND = 2 * MEASURED_CH_REL, 2 * MEASURED_DUP
# restatement against scikit-learn's float32 arithmetic (tests/test_cluster_ref_cpu.py): added where the kernel
# is compared with the fixture's own numbers
SK_SAMPLE, SK_SCORE, SK_CH_REL = 9.14e-7, 4.73e-7, 9.54e-7


def _synthetic(n, seed, labels=None):
    """Post-ReLU-like embeddings 0.5 + 0.1 |N(0, 1)| plus a class offset; labels in [0, 4) unless given."""
    rs = np.random.RandomState(seed)
    if labels is None:
        labels = rs.randint(0, 4, n)
    labels = np.asarray(labels, dtype=np.int64)
    offsets = 0.08 * rs.standard_normal((4, 256))
    emb = 0.5 + 0.1 * np.abs(rs.standard_normal((n, 256))) + offsets[np.clip(labels, 0, 3)]
    return emb.astype(np.float32), labels


@functools.lru_cache(None)
def _case(name):
    """(emb, labels, dup rows or None, cluster_ref of them); computed once, never modified."""
    if isinstance(name, int) and name in CASES:
        g = np.load(GOLDEN)
        key = "n%d_" % name
        emb, labels, dup = g[key + "emb"], g[key + "labels"], g[key + "dup"]
    else:
        n, seed = name
        emb, labels = _synthetic(n, seed)
        dup = None
    return emb, labels, dup, cluster_ref(emb, labels)


def _run(emb, labels, chunks=0, samples=True):
    r = E.cluster_metrics(torch.from_numpy(np.ascontiguousarray(emb)).cuda(), labels, samples=samples, _chunks=chunks)
    if samples:
        r["silhouette_samples"] = r["silhouette_samples"].cpu().numpy()
    return r


def _errors(r, ref, dup=None):
    d = np.abs(r["silhouette_samples"].astype(np.float64) - ref["silhouette_samples"])
    rest = np.ones(len(d), bool)
    if dup is not None:
        rest[dup] = False
    rel = lambda a, b: abs(a / b - 1.0) if b else abs(a)
    return {"sample": float(d[rest].max()), "dup": float(d[~rest].max()) if dup is not None else 0.0,
            "score": abs(r["silhouette_score"] - ref["silhouette_score"]),
            "class": float(np.abs(np.array(r["silhouette_per_class"]) - ref["silhouette_per_class"]).max()),
            "ch_rel": max(rel(r["calinski_harabasz_score"], ref["calinski_harabasz_score"]),
                          rel(r["within"], ref["within"]), rel(r["between"], ref["between"]))}


def _check(r, ref, dup=None, what=""):
    e = _errors(r, ref, dup)
    print("%s: |kernel - cluster_ref|: sample %.3e  dup %.3e  score %.3e  class %.3e  CH/W/B rel %.3e"
          % (what, e["sample"], e["dup"], e["score"], e["class"], e["ch_rel"]))
    assert r["valid"] == ref["valid"] and r["n_labelled"] == ref["n_labelled"]
    assert r["classes_present"] == ref["classes_present"] and r["class_counts"] == ref["class_counts"]
    assert e["sample"] <= SAMPLE_BOUND and e["dup"] <= DUP_BOUND, e
    assert e["score"] <= SCORE_BOUND and e["class"] <= CLASS_BOUND and e["ch_rel"] <= CH_REL_BOUND, e
    return e


def _same_bits(a, b):
    return a["block"].tobytes() == b["block"].tobytes() and \
        np.array_equal(a["silhouette_samples"].view(np.uint32), b["silhouette_samples"].view(np.uint32))


# ---------------------------------------------------------------- 1. the fixture cases
@pytest.mark.parametrize("n", CASES)
def test_fixture_cases(n):
    emb, labels, dup, ref = _case(n)
    r = _run(emb, labels)
    _check(r, ref, dup, "fixture n=%d" % n)
    g = np.load(GOLDEN)
    key = "n%d_" % n
    sk = np.abs(r["silhouette_samples"] - g[key + "silhouette_samples"])
    assert sk.max() <= max(SAMPLE_BOUND, DUP_BOUND) + SK_SAMPLE
    assert abs(r["silhouette_score"] - float(g[key + "silhouette_score"])) <= SCORE_BOUND + SK_SCORE
    assert abs(r["calinski_harabasz_score"] / float(g[key + "calinski_harabasz_score"]) - 1) <= CH_REL_BOUND + SK_CH_REL
    assert not r["silhouette_samples"][labels < 0].any()
    assert r["silhouette_samples"][labels == r["class_counts"].index(1)] == 0.0      # the single member


# ---------------------------------------------------------------- 2. tile edges, chunked summation
# 2T - 1, 2T, 2T + 1 rows; 4T + 1 rows in 3 chunks of 2 column tiles leave the last chunk one single column
@pytest.mark.parametrize("n", [2 * T - 1, 2 * T, 2 * T + 1, 4 * T + 1])
def test_tile_edges_and_chunks(n):
    emb, labels, _, ref = _case((n, 200 + n))
    runs = {}
    for chunks in (1, 3):
        a, b = _run(emb, labels, chunks), _run(emb, labels, chunks)
        _check(a, ref, None, "n=%d chunks=%d" % (n, chunks))
        assert _same_bits(a, b), chunks
        runs[chunks] = a
    _check(_run(emb, labels), ref, None, "n=%d planned" % n)
    d = np.abs(runs[1]["silhouette_samples"].astype(np.float64) - runs[3]["silhouette_samples"]).max()
    assert d <= SAMPLE_BOUND and abs(runs[1]["silhouette_score"] - runs[3]["silhouette_score"]) <= SCORE_BOUND
    assert runs[1]["within"] == runs[3]["within"] and runs[1]["between"] == runs[3]["between"]


def test_single_column_chunk_really_is_one():
    """The geometry test 2 relies on, from the host plan's own rule."""
    n, want = 4 * T + 1, 3
    rt = -(-n // T)
    per = -(-rt // want)
    chunks = -(-rt // per)
    assert (rt, per, chunks) == (5, 2, 3) and n - T * per * (chunks - 1) == 1


# ---------------------------------------------------------------- 3. the smallest inputs
@pytest.mark.parametrize("labels", [[2], [0, 3], [1, 1, 1, 1, 1, 1, 1]], ids=["n1", "n2_two_classes", "one_class"])
def test_smallest_inputs_are_invalid(labels):
    emb, labels = _synthetic(len(labels), 31, labels)
    with pytest.warns(RuntimeWarning, match="both scores are 0.0"):
        r = _run(emb, labels)
    ref = cluster_ref(emb, labels)
    assert r["valid"] is False and ref["valid"] is False
    assert r["silhouette_score"] == 0.0 and r["calinski_harabasz_score"] == 0.0
    assert not r["silhouette_samples"].any() and not any(r["silhouette_per_class"])
    assert r["class_counts"] == ref["class_counts"] and r["n_labelled"] == len(labels)


def test_three_rows_two_classes_is_valid():
    emb, labels = _synthetic(3, 32, [0, 0, 1])
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        r = _run(emb, labels)
    _check(r, cluster_ref(emb, labels), None, "n=3")
    assert r["valid"] and r["silhouette_samples"][2] == 0.0


# ---------------------------------------------------------------- 4. unlabelled and permuted rows
def test_unlabelled_rows_are_ignored():
    emb, labels, _, _ = _case((2 * T + 1, 200 + 2 * T + 1))
    labels = labels.copy()
    labels[[3, 64, 100]] = -1
    labels[[0, 128]] = 7
    keep = (labels >= 0) & (labels < 4)
    full, part = _run(emb, labels), _run(emb[keep], labels[keep])
    ref = cluster_ref(emb[keep], labels[keep])
    _check(part, ref, None, "labelled rows alone")
    assert not full["silhouette_samples"][~keep].any()
    full["silhouette_samples"] = full["silhouette_samples"][keep]
    _check(full, ref, None, "with unlabelled rows")
    assert full["class_counts"] == part["class_counts"] and full["n_labelled"] == int(keep.sum())


def test_permuted_rows_permute_the_samples():
    emb, labels, _, ref = _case((2 * T + 1, 200 + 2 * T + 1))
    perm = np.random.RandomState(41).permutation(len(labels))
    r = _run(emb[perm], labels[perm])
    back = np.empty_like(r["silhouette_samples"])
    back[perm] = r["silhouette_samples"]
    r["silhouette_samples"] = back
    _check(r, ref, None, "permuted")


# ---------------------------------------------------------------- 5. poison and padding
def test_nan_in_a_labelled_row_raises_with_the_count():
    emb, labels, _, _ = _case(65)
    emb = emb.copy()
    rows = np.where(labels >= 0)[0][[1, 40]]
    emb[rows[0], 17] = np.nan
    emb[rows[1], 255] = np.inf
    with pytest.raises(PKG._lib.DadError, match="2 of 63 labelled row"):
        _run(emb, labels)


def test_nan_in_an_unlabelled_row_changes_nothing():
    emb, labels, _, _ = _case(65)
    want = _run(emb, labels)
    emb = emb.copy()
    emb[np.where(labels < 0)[0]] = np.nan
    assert _same_bits(_run(emb, labels), want)


def test_poison_past_row_n_changes_no_bit():
    emb, labels, _, _ = _case(37)
    n = len(labels)
    want = _run(emb, labels)
    big = torch.full((n + 2 * T, 256), float("nan"), device="cuda")
    big[:n] = torch.from_numpy(emb).cuda()
    lab = torch.full((n + 2 * T,), 1, dtype=torch.int64, device="cuda")
    lab[:n] = torch.from_numpy(labels).cuda()
    r = E.cluster_metrics(big[:n], lab[:n], samples=True)
    r["silhouette_samples"] = r["silhouette_samples"].cpu().numpy()
    assert _same_bits(r, want)
    assert torch.isnan(big[n:]).all()


# ---------------------------------------------------------------- 6. the store path
@functools.lru_cache(None)
def _model(seed=11):
    stu, tea = do.eval_weights(seed)
    model = PKG.SSRLModel().cuda()
    with torch.no_grad():
        model.student_flat.copy_(torch.from_numpy(gh.flat(stu)))
        model.teacher_flat.copy_(torch.from_numpy(gh.flat(tea)))
    return model


@functools.lru_cache(None)
def _store(dt):
    """The 37-utterance shuffled subset of tests/test_gpu_eval_split.py (39 rows, two samples twice, two
    labels of -1), rebuilt from its seeds."""
    sizes = np.concatenate([[0, 1, 3, 31, 32, 33, 63, 64, 65, 96], np.random.RandomState(13).randint(1, 71, 27)])
    labels = np.random.RandomState(14).randint(0, 4, len(sizes))
    labels[[5, 20]] = -1
    perm = np.random.RandomState(15).permutation(len(sizes))
    order = np.concatenate([perm[:30], [perm[3], perm[11]], perm[30:]])
    offsets = np.concatenate([[0], np.cumsum(sizes)[:-1]])
    feats = np.random.RandomState(12).standard_normal((int(sizes.sum()), 768)).astype(np.float32)
    return D.FeatureStore(feats, sizes, offsets, labels.astype(np.int64), dtype=DTYPES[dt]).subset(order)


@pytest.mark.parametrize("use_teacher", [False, True], ids=["student", "teacher"])
@pytest.mark.parametrize("dt", ["f32", "f16", "bf16"])
def test_store_path_equals_the_two_step_path(dt, use_teacher):
    model, store = _model(), _store(dt)
    got = E.cluster_metrics_store(model, store, use_teacher=use_teacher, samples=True)
    emb = E.embed_store(model, store, use_teacher=use_teacher)
    want = E.cluster_metrics(emb, store.labels, samples=True)
    assert got["valid"] and got["n_labelled"] == 37
    assert got["block"].tobytes() == want["block"].tobytes()
    assert torch.equal(got["silhouette_samples"].view(torch.int32), want["silhouette_samples"].view(torch.int32))
    ws = E.EvalPlan.of(store).cluster_buffers()[0].data_ptr()
    again = E.cluster_metrics_store(model, store, use_teacher=use_teacher)
    assert E.EvalPlan.of(store).cluster_buffers()[0].data_ptr() == ws
    assert again["block"].tobytes() == got["block"].tobytes()


@pytest.mark.parametrize("teacher_disagreement", [False, True])
def test_validate_store_carries_the_two_scores(teacher_disagreement):
    model, store = _model(), _store("f32")
    base = E.validate_store(model, store, teacher_disagreement=teacher_disagreement)
    r = E.validate_store(model, store, teacher_disagreement=teacher_disagreement, cluster_metrics=True)
    cm = E.cluster_metrics_store(model, store)
    assert r["silhouette_score"] == cm["silhouette_score"]
    assert r["calinski_harabasz_score"] == cm["calinski_harabasz_score"]
    assert sorted(r) == sorted(list(base) + ["silhouette_score", "calinski_harabasz_score"])
    for k, v in base.items():
        if k == "confusion_matrix":
            np.testing.assert_array_equal(r[k], v)
        else:
            assert r[k] == v, k


def test_store_without_labels_is_refused():
    sizes = np.array([3, 5])
    feats = np.zeros((8, 768), np.float32)
    store = D.FeatureStore(feats, sizes, np.array([0, 3]), None)
    with pytest.raises(ValueError, match="no labels"):
        E.cluster_metrics_store(_model(), store)
    with pytest.raises(ValueError, match="no labels"):
        E.validate_store(_model(), store, cluster_metrics=True)


def test_separation_report_of_two_models():
    model, store = _model(), _store("f32")
    other = PKG.SSRLModel().cuda()
    with torch.no_grad():
        other.student_flat.copy_(model.teacher_flat)
        other.teacher_flat.copy_(model.teacher_flat)
    rep = E.separation_report(model, other, store)
    a, b = E.cluster_metrics_store(model, store), E.cluster_metrics_store(model, store, use_teacher=True)
    assert rep == E.separation_from_metrics(a, b)
    assert rep["trained_weights"]["silhouette_score"] == b["silhouette_score"]


# ---------------------------------------------------------------- 7. graph capture
def test_captured_enqueue_replays_like_eager():
    model, store = _model(), _store("f32")
    plan = E.EvalPlan.of(store)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        want = E.cluster_metrics_store(model, store, samples=True)      # (lazy buffers, then the eager block)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    block_d = plan.cluster_buffers()[1]
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        emb, sil = E.enqueue_cluster_metrics_store(model, plan, samples=True)
    for _ in range(2):
        block_d.fill_(-1.0)
        sil.fill_(-1.0)
        g.replay()
        torch.cuda.synchronize()
        assert block_d.cpu().numpy().tobytes() == want["block"].tobytes()
        assert torch.equal(sil.view(torch.int32), want["silhouette_samples"].view(torch.int32))


# ---------------------------------------------------------------- 8. determinism
def test_two_runs_at_1100_rows_are_identical():
    emb, labels = _synthetic(1100, 51)
    x = torch.from_numpy(emb).cuda()
    a = E.cluster_metrics(x, labels, samples=True)
    b = E.cluster_metrics(x, labels, samples=True)
    assert a["valid"] and a["block"].tobytes() == b["block"].tobytes()
    assert torch.equal(a["silhouette_samples"].view(torch.int32), b["silhouette_samples"].view(torch.int32))
    c = E.cluster_metrics(x, labels, _chunks=1)       # (the planner cuts 18 row tiles into chunks; one chunk agrees)
    assert abs(c["silhouette_score"] - a["silhouette_score"]) <= SCORE_BOUND
