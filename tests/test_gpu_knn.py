"""Exact k-NN, the k-NN vote and trustworthiness on the MI355X (evaluate.knn* / trustworthiness + csrc/knn.hip) against
the float64 restatement tests/knn_ref.py (computed once per input on the CPU) and the scikit-learn fixture
tests/golden/eval_knn.npz: the fixture cases, the tile edges and the chunk counts, the smallest inputs, the modes,
an exactly representable problem with many ties, poison and padding, the vote alone, the store path, tsne_report and
graph capture."""
import ctypes
import functools
import os

import numpy as np
import pytest
import torch

import dadpkg
import gpu_harness as gh
import knn_ref as kr
from oracle import data_oracle as do

pytestmark = pytest.mark.gpu
PKG = dadpkg.pkg()
D = PKG.data
E = PKG.evaluate
L = PKG._lib
T = L.KNN_TILE
GOLDEN = os.path.join(dadpkg.ROOT, "tests", "golden", "eval_knn.npz")
CASES = (37, 65, 129)

# Worst |device d2 - restatement d2| over the sorted neighbour distances, measured on the MI355X over the float inputs
# this file compares with knn_ref (every chunk count gives the same bits).  Per input, k = 1 / 5 / 15 / 32:
#   n=127  2.43e-6  2.56e-6  2.74e-6  2.74e-6      n=128  2.61e-6  3.44e-6  3.44e-6  3.97e-6
#   n=129  2.06e-6  3.11e-6  3.51e-6  3.51e-6      n=257  3.02e-6  3.80e-6  3.96e-6  3.99e-6
# and at k = 5:
#   fixture  n=37 3.24e-6  n=65 2.68e-6  n=129 3.42e-6      n=2 3.91e-7  n=3 5.34e-7  n=1,100 3.71e-6
#   groups (n=129)  all 2.60e-6  same 3.03e-6  other 2.46e-6
# against neighbour distances of up to 5.2: the fp32 Gram form's cancellation in |a|^2 + |b|^2 - 2 a.b on the centred
# rows.  The penalty sums of trustworthiness equalled the restatement's on every input but n=257 at k = 32 (64,223
# against 64,224, with A = 39).
# knn_ref.MEASURED_D2 is the largest of them and D2_BOUND twice that (the kernel is deterministic; the factor guards
# against a recompilation's summation order).  Indices: a row is ambiguous when two consecutive entries among its first
# k + 1 sorted float64 distances lie within 2 * D2_BOUND; every other row's list must equal the restatement's.
# Trustworthiness: |penalty sum - restatement's| <= A, the (row, map neighbour) pairs whose float64 rank can change
# when D moves by +-D2_BOUND (knn_ref.rank_changes); T follows from the penalty sum.
D2_BOUND = kr.D2_BOUND


def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


@functools.lru_cache(None)
def _case(name):
    """(emb, labels, Y, D float64); computed once, never modified."""
    if isinstance(name, int):
        g = np.load(GOLDEN)
        key = "n%d_" % name
        emb, labels, Y = g[key + "emb"], g[key + "labels"], g[key + "Y"]
    else:
        n, seed = name
        emb, labels = kr.synthetic(n, seed)
        Y = kr.pca_map(emb)
    return emb, labels, Y, kr.pair_d2(emb)


def _knn(emb, k, group=None, mode="all", chunks=0):
    idx, d2 = E.knn(_dev(emb), k, None if group is None else _dev(np.asarray(group, np.int32)), mode, _chunks=chunks)
    return idx.cpu().numpy(), d2.cpu().numpy()


def _same_bits(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32))


def _check_lists(got, Dm, k, what, group=None, mode=kr.ALL):
    """The device's lists against the restatement's under D2_BOUND and the ambiguity rule; returns the worst d2 error."""
    idx, d2 = got
    n = len(Dm)
    ridx, rd2 = kr.knn_ref(np.empty((n, 0)), k, group, mode, D=Dm)
    pad = ridx < 0
    assert np.array_equal(idx < 0, pad) and np.isinf(d2[pad]).all() and (idx[pad] == -1).all(), what
    err = float(np.abs(d2.astype(np.float64)[~pad] - rd2[~pad]).max()) if (~pad).any() else 0.0
    amb = kr.ambiguous_rows(Dm, k, D2_BOUND, kr.candidates(n, group, mode))
    print("%s: worst |device d2 - knn_ref| %.3e  ambiguous rows %d of %d" % (what, err, int(amb.sum()), n))
    assert err <= D2_BOUND, (what, err)
    assert np.array_equal(idx[~amb], ridx[~amb]), what
    # an ambiguous row's own choices: candidates, distinct, and each as far as the restatement says, within the bound
    for i in np.where(amb)[0]:
        js = idx[i][idx[i] >= 0]
        assert len(set(js)) == len(js) and kr.candidates(n, group, mode)[i, js].all(), (what, i)
        assert np.abs(d2[i][idx[i] >= 0].astype(np.float64) - Dm[i, js]).max() <= D2_BOUND, (what, i)
    return err


def _trust(emb, Y, k, chunks=0):
    r = E.trustworthiness(_dev(emb), _dev(Y), k, samples=True, _chunks=chunks)
    r["penalty"] = r["penalty"].cpu().numpy()
    return r


def _check_trust(r, emb, Y, Dm, k, what):
    nbr = kr.map_neighbours(Y, k, np.float32)         # (the device's own fp32 operations on Y)
    ref = kr.trustworthiness_ref(emb, Y, k, nbr=nbr, D=Dm)
    a = kr.rank_changes(Dm, nbr, D2_BOUND)
    n = len(emb)
    print("%s: penalty sum %d (knn_ref %d, A = %d)  T %.12f (knn_ref %.12f)"
          % (what, r["penalty_sum"], ref["penalty_sum"], a, r["trustworthiness"], ref["trustworthiness"]))
    assert r["n"] == n and r["k"] == k and r["penalty_sum"] == int(r["penalty"].sum())
    assert abs(r["penalty_sum"] - ref["penalty_sum"]) <= a, what
    want_t = 1.0 - r["penalty_sum"] * (2.0 / (n * k * (2.0 * n - 3.0 * k - 1.0)))
    assert abs(r["trustworthiness"] - want_t) <= 1e-14
    return ref, a


# ---------------------------------------------------------------- 1. the fixture cases
@pytest.mark.parametrize("n", CASES)
def test_fixture_cases(n):
    emb, labels, Y, Dm = _case(n)
    g = np.load(GOLDEN)
    key, k = "n%d_" % n, int(g["k"])
    got = _knn(emb, k)
    _check_lists(got, Dm, k, "fixture n=%d" % n)
    amb = kr.ambiguous_rows(Dm, k, D2_BOUND)
    assert np.array_equal(got[0][~amb], g[key + "nn_idx"][~amb])
    assert np.abs(got[1].astype(np.float64) - g[key + "nn_d2"])[~amb].max() <= D2_BOUND + 1e-9 * g[key + "nn_d2"].max()
    r = E.knn_accuracy(_dev(emb), labels, k)
    pred = r["pred"].cpu().numpy()
    assert np.array_equal(pred[~amb], g[key + "pred"][~amb])
    assert r["n_queries"] == n and r["n_no_vote"] == 0 and r["confusion_matrix"].sum() == n
    tr = _trust(emb, Y, k)
    _, a = _check_trust(tr, emb, Y, Dm, k, "fixture n=%d" % n)
    assert np.array_equal(kr.map_neighbours(Y, k, np.float32), kr.map_neighbours(Y, k))   # (so the fixture's T applies)
    assert abs(tr["trustworthiness"] - float(g[key + "trustworthiness"])) <= a * 2.0 / (n * k * (2.0 * n - 3.0 * k - 1.0)) + 1e-12


# ---------------------------------------------------------------- 2. tile edges, chunk counts
@pytest.mark.parametrize("k", kr.FLOAT_KS)
@pytest.mark.parametrize("case", kr.FLOAT_CASES, ids=[c[0] for c in kr.FLOAT_CASES])
def test_tile_edges_and_chunks(case, k):
    _, n, seed = case
    emb, _, Y, Dm = _case((n, seed))
    runs = [_knn(emb, k, chunks=c) for c in (1, 1, 3, 3, 0)]
    for r in runs[1:]:
        assert _same_bits(r, runs[0])                 # every chunk count and both runs: the same bits
    _check_lists(runs[0], Dm, k, "n=%d k=%d" % (n, k))
    tr = [_trust(emb, Y, k, chunks=c) for c in (1, 1, 3, 0)]
    for r in tr[1:]:
        assert r["block"].tobytes() == tr[0]["block"].tobytes() and np.array_equal(r["penalty"], tr[0]["penalty"])
    _check_trust(tr[0], emb, Y, Dm, k, "n=%d k=%d" % (n, k))


def test_planned_chunks_at_1100_rows():
    """The planner cuts 18 row tiles into several chunks; one chunk gives the same bits, and the lists are the
    restatement's."""
    _, n, seed = kr.LARGE_CASE
    emb, _ = kr.synthetic(n, seed)
    x = _dev(emb)
    a, b, c = E.knn(x, kr.LARGE_K), E.knn(x, kr.LARGE_K), E.knn(x, kr.LARGE_K, _chunks=1)
    for other in (b, c):
        assert torch.equal(a[0], other[0]) and torch.equal(a[1].view(torch.int32), other[1].view(torch.int32))
    v = [ctypes.c_int() for _ in range(3)]
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    assert L.lib().dad_knn_plan(n, kr.LARGE_K, cus, *v) == 0 and v[0].value == 18 and v[1].value > 1
    _check_lists((a[0].cpu().numpy(), a[1].cpu().numpy()), kr.pair_d2(emb), kr.LARGE_K, "n=%d k=%d" % (n, kr.LARGE_K))


# ---------------------------------------------------------------- 3. the smallest inputs
def test_one_row_has_no_neighbour():
    emb, _ = kr.synthetic(1, 31)
    idx, d2 = _knn(emb, 5)
    assert (idx == -1).all() and np.isinf(d2).all() and idx.shape == (1, 5)
    with pytest.raises(ValueError, match="no row has a voting neighbour"):
        E.knn_accuracy(_dev(emb), [2], 5)


@pytest.mark.parametrize("case", kr.SMALL_CASES, ids=[c[0] for c in kr.SMALL_CASES])
def test_two_and_three_rows_pad_their_lists(case):
    _, n, seed = case
    emb, _ = kr.synthetic(n, seed)
    got = _knn(emb, kr.SMALL_K)
    assert (got[0][:, :n - 1] >= 0).all() and (got[0][:, n - 1:] == -1).all() and np.isinf(got[1][:, n - 1:]).all()
    _check_lists(got, kr.pair_d2(emb), kr.SMALL_K, "n=%d k=%d" % (n, kr.SMALL_K))


def test_a_group_of_one_has_no_candidate_of_its_own():
    emb, _ = kr.synthetic(4, 33)
    group = [0, 1, 1, 1]
    idx, d2 = _knn(emb, 5, group, "same")
    assert (idx[0] == -1).all() and np.isinf(d2[0]).all()
    assert np.array_equal(idx, kr.knn_ref(emb, 5, group, kr.SAME)[0])


# ---------------------------------------------------------------- 4. the modes
@functools.lru_cache(None)
def _grouped():
    _, n, seed = kr.FLOAT_CASES[2]
    emb, labels, _, Dm = _case((n, seed))
    group = np.where(np.arange(n) % 5 < 2, 0, 1)       # uneven: 2 / 5 against 3 / 5
    group[np.arange(n) % 17 == 3] = 2
    group[[3, 64, 100, 128]] = -1
    return emb, labels, Dm, group


@pytest.mark.parametrize("mode", ["all", "same", "other"])
def test_modes_with_uneven_groups_and_absent_rows(mode):
    emb, _, Dm, group = _grouped()
    m = {"all": kr.ALL, "same": kr.SAME, "other": kr.OTHER}[mode]
    runs = [_knn(emb, 5, group, mode, chunks=c) for c in (1, 3, 0)]
    assert _same_bits(runs[0], runs[1]) and _same_bits(runs[0], runs[2])
    idx, d2 = runs[0]
    out = group < 0
    assert (idx[out] == -1).all() and np.isinf(d2[out]).all()
    assert not np.isin(idx[~out], np.where(out)[0]).any()
    # the restatement over the participating rows alone is centred on the same mean: the bound holds
    _check_lists(runs[0], Dm, 5, "mode %s" % mode, group, m)


def test_a_row_permutation_permutes_the_lists():
    emb, _, Dm, group = _grouped()
    perm = np.random.RandomState(41).permutation(len(emb))
    base = _knn(emb, 5, group, "other")
    idx, d2 = _knn(emb[perm], 5, group[perm], "other")
    amb = kr.ambiguous_rows(Dm, 5, D2_BOUND, kr.candidates(len(emb), group, kr.OTHER))
    mapped = np.where(idx >= 0, perm[np.clip(idx, 0, None)], -1)      # row r of the permuted run is row perm[r]
    back_idx, back_d2 = np.empty_like(mapped), np.empty_like(d2)
    back_idx[perm], back_d2[perm] = mapped, d2
    assert np.array_equal(back_idx[~amb], base[0][~amb])
    fin = np.isfinite(base[1])
    assert np.array_equal(np.isfinite(back_d2), fin) and np.abs(back_d2[fin] - base[1][fin]).max() <= 2 * D2_BOUND


# ---------------------------------------------------------------- 5. an exactly representable problem
@functools.lru_cache(None)
def _exact(n):
    """Rows 8 + e with integer e in {-3 .. 3} and zero column sums: the mean is 8, and every centred entry, Gram entry
    and squared distance is an integer that fp32 holds exactly, with many ties.  Y on an integer grid ties too."""
    rs = np.random.RandomState(900 + n)
    m = n - 2                   # rows 1 and n - 2 are 8 throughout: leaving them out keeps the column sums at zero
    half = rs.randint(-3, 4, (m // 2, 256))
    e = np.concatenate([half, -half, np.zeros((m % 2, 256), np.int64)])
    for c in range(256):
        e[:, c] = e[rs.permutation(m), c]
    e = np.concatenate([e[:1], np.zeros((1, 256), np.int64), e[1:m - 1], np.zeros((1, 256), np.int64), e[m - 1:]])
    assert len(e) == n and not e.sum(0).any() and not e[[1, n - 2]].any()
    emb = (8.0 + e).astype(np.float32)
    labels = rs.randint(0, 4, n).astype(np.int64)
    labels[[1, n - 2]] = (-1, 7)     # (the vote's absent rows)
    Y = rs.randint(0, 12, (n, 2)).astype(np.float32)
    Dm = kr.pair_d2(emb)
    assert np.array_equal(Dm, np.round(Dm)) and Dm.max() < 2 ** 24
    return emb, labels, Y, Dm


@pytest.mark.parametrize("n", [2 * T + 1, 4 * T + 1])
def test_exact_problem_equals_the_restatement(n):
    emb, labels, Y, Dm = _exact(n)
    for k in (5, 32):
        ridx, rd2 = kr.knn_ref(emb, k, D=Dm)
        for chunks in (1, 3, 0):
            idx, d2 = _knn(emb, k, chunks=chunks)
            assert np.array_equal(idx, ridx) and np.array_equal(d2.astype(np.float64), rd2), (k, chunks)
        assert k < 32 or (np.diff(rd2, axis=1) == 0).any()          # (ties inside the lists)
        nbr = kr.map_neighbours(Y, k)
        assert np.array_equal(nbr, kr.map_neighbours(Y, k, np.float32))
        ref = kr.trustworthiness_ref(emb, Y, k, nbr=nbr, D=Dm)
        for chunks in (1, 3, 0):
            r = _trust(emb, Y, k, chunks)
            assert r["penalty_sum"] == ref["penalty_sum"] and np.array_equal(r["penalty"], ref["penalty"]), (k, chunks)
            assert abs(r["trustworthiness"] - ref["trustworthiness"]) <= 1e-14
    # the vote: rows with a label outside [0, 4) take no part
    group = np.where((labels >= 0) & (labels < 4), np.arange(n) % 2, -1)
    for mode, m in (("all", kr.ALL), ("other", kr.OTHER)):
        ridx, _ = kr.knn_ref(emb, 5, group, m, D=Dm)
        rpred, rblock = kr.vote_ref(ridx, labels, group)
        r = E.knn_accuracy(_dev(emb), labels, 5, domain=np.arange(n) % 2, mode=mode)
        assert np.array_equal(r[0]["pred"].cpu().numpy(), rpred)
        assert np.array_equal(r[0]["block"][:L.KV_SLOTS], rblock) and r[0]["block"][L.KV_SLOTS] == 0
        for q in (0, 1):
            assert np.array_equal(r[q]["confusion_matrix"], rblock[16 * q:16 * q + 16].reshape(4, 4))
            assert r[q]["n_queries"] == rblock[kr.KV_QUERIES + q]


# ---------------------------------------------------------------- 6. poison and padding
def test_poison_past_row_n_and_in_a_padded_buffer_changes_no_bit():
    emb, labels, Y, _ = _case(37)
    n = len(emb)
    want = _knn(emb, 5)
    want_t = _trust(emb, Y, 5)
    big = torch.full((n + 2 * T, 256), float("nan"), device="cuda")
    big[:n] = _dev(emb)
    bigy = torch.full((n + 2 * T, 2), float("nan"), device="cuda")
    bigy[:n] = _dev(Y)
    idx, d2 = E.knn(big[:n], 5)
    assert _same_bits((idx.cpu().numpy(), d2.cpu().numpy()), want)
    r = E.trustworthiness(big[:n], bigy[:n], 5)
    assert r["block"].tobytes() == want_t["block"].tobytes()
    assert torch.isnan(big[n:]).all()


def test_nan_in_an_absent_row_changes_nothing_and_in_a_present_row_is_counted():
    emb, _, Dm, group = _grouped()
    want = _knn(emb, 5, group, "all")
    bad = emb.copy()
    bad[group < 0] = np.nan
    assert _same_bits(_knn(bad, 5, group, "all"), want)
    bad = emb.copy()
    bad[7, 17], bad[90, 255] = np.nan, np.inf
    with pytest.raises(L.DadError, match="2 participating row"):
        _knn(bad, 5, group, "all")
    with pytest.raises(L.DadError, match="2 participating row"):
        E.knn_accuracy(_dev(bad), np.where(group >= 0, 1, -1), 5)
    Y = kr.pca_map(emb)
    with pytest.raises(L.DadError, match="2 row"):
        E.trustworthiness(_dev(bad), _dev(Y), 5)
    Y = Y.copy()
    Y[5, 1] = np.nan
    with pytest.raises(L.DadError, match="1 row"):
        E.trustworthiness(_dev(emb), _dev(Y), 5)


def test_limits_are_refused_before_any_launch():
    emb, _ = kr.synthetic(20, 35)
    x = _dev(emb)
    for k in (0, 33):
        with pytest.raises(ValueError, match="knn takes"):
            E.knn(x, k)
    with pytest.raises(ValueError, match="mode"):
        E.knn(x, 5, mode="nearest")
    for k in (0, 10, 33):                   # k >= n / 2 is scikit-learn's refusal
        with pytest.raises(ValueError, match="trustworthiness takes"):
            E.trustworthiness(x, x[:, :2].contiguous(), k)


# ---------------------------------------------------------------- 7. the vote on its own
def test_the_vote_equals_the_numpy_vote_on_the_kernels_own_lists():
    emb, labels, _, group = _grouped()
    labels = labels.copy()
    labels[[0, 11, 77]] = (-1, 7, 4)         # candidates without a vote, queries outside the confusion matrix
    labels_d, group_d = _dev(labels), _dev(group.astype(np.int32))
    for k in (1, 4, 32):
        idx, _ = E.knn(_dev(emb), k, group_d, "all")
        pred = torch.empty(len(emb), dtype=torch.int64, device="cuda")
        block = torch.empty(L.KV_SLOTS, dtype=torch.int64, device="cuda")
        L.check(L.lib().dad_knn_vote(L.ptr(idx), L.ptr(labels_d), L.ptr(group_d), len(emb), k, L.ptr(pred), L.ptr(block),
                                     torch.cuda.current_stream().cuda_stream))
        rpred, rblock = kr.vote_ref(idx.cpu().numpy(), labels, group)
        assert np.array_equal(pred.cpu().numpy(), rpred) and np.array_equal(block.cpu().numpy(), rblock), k
        assert rblock[16:32].any() and rblock[:16].any()


# ---------------------------------------------------------------- 8. the store path
@functools.lru_cache(None)
def _model(seed=11):
    stu, tea = do.eval_weights(seed)
    model = PKG.SSRLModel().cuda()
    with torch.no_grad():
        model.student_flat.copy_(torch.from_numpy(gh.flat(stu)))
        model.teacher_flat.copy_(torch.from_numpy(gh.flat(tea)))
    return model


def _store_parts(kind):
    seed, count = {"clean": (21, 33), "noisy": (31, 41)}[kind]
    rs = np.random.RandomState(seed)
    sizes = np.concatenate([[1, 31, 32, 33, 64, 65], rs.randint(1, 71, count - 6)])
    labels = rs.randint(0, 4, count)
    if kind == "noisy":
        labels[[4, 17]] = -1
    offsets = np.concatenate([[0], np.cumsum(sizes)[:-1]])
    feats = rs.standard_normal((int(sizes.sum()), 768)).astype(np.float32)
    return feats, sizes, offsets, labels.astype(np.int64)


@functools.lru_cache(None)
def _store(kind, dt="f32"):
    """Two small synthetic stores of different sizes: 'clean' 33 utterances, 'noisy' 41 (two labelled -1); 'f16': held
    as fp16; 'f16w': the f32 store of the fp16 values."""
    feats, sizes, offsets, labels = _store_parts(kind)
    if dt == "f16w":
        feats = feats.astype(np.float16).astype(np.float32)
    return D.FeatureStore(feats, sizes, offsets, labels, dtype=torch.float16 if dt == "f16" else torch.float32)


def _same_result(a, b):
    return a["block"].tobytes() == b["block"].tobytes() and torch.equal(a["pred"], b["pred"])


@pytest.mark.parametrize("use_teacher", [False, True], ids=["student", "teacher"])
def test_knn_store_equals_the_two_step_path(use_teacher):
    model, store = _model(), _store("noisy")
    got = E.knn_store(model, store, 5, use_teacher=use_teacher)
    want = E.knn_accuracy(E.embed_store(model, store, use_teacher=use_teacher), store.labels, 5)
    assert got["n_queries"] == 39 and got["confusion_matrix"].sum() == 39 and _same_result(got, want)
    assert (got["pred"][[4, 17]] == -1).all()
    plan = E.EvalPlan.of(store)
    bufs = plan._knn[(41, 5)]
    again = E.knn_store(model, store, 5, use_teacher=use_teacher)
    assert plan._knn[(41, 5)] is bufs and _same_result(again, got)


def test_cross_domain_knn_store_equals_the_two_step_path():
    model, clean, noisy = _model(), _store("clean"), _store("noisy")
    got = E.cross_domain_knn_store(model, clean, noisy, 5)
    emb = torch.cat([E.embed_store(model, clean), E.embed_store(model, noisy)])
    labels = np.concatenate([np.asarray(clean.labels), np.asarray(noisy.labels)])
    domain = np.concatenate([np.zeros(33, np.int64), np.ones(41, np.int64)])
    want = E.knn_accuracy(emb, labels, 5, domain=domain, mode="other")
    assert _same_result(got["noisy_to_clean"], want[1]) and _same_result(got["clean_to_noisy"], want[0])
    assert got["noisy_to_clean"]["n_queries"] == 39 and got["clean_to_noisy"]["n_queries"] == 33
    np.testing.assert_array_equal(got["noisy_to_clean"]["confusion_matrix"], want[1]["confusion_matrix"])
    assert got["noisy_to_clean"]["accuracy"] == want[1]["accuracy"]
    idx, _ = E.knn(emb, 5, _dev(np.where((labels >= 0) & (labels < 4), domain, -1).astype(np.int32)), "other")
    idx = idx.cpu().numpy()
    assert (idx[:33][idx[:33] >= 0] >= 33).all() and (idx[33:][idx[33:] >= 0] < 33).all()


def test_f16_store_gives_the_results_of_its_widened_copy():
    model = _model()
    got = E.knn_store(model, _store("noisy", "f16"), 5)
    want = E.knn_store(model, _store("noisy", "f16w"), 5)
    assert _same_result(got, want)
    cross = E.cross_domain_knn_store(model, _store("clean", "f16"), _store("noisy", "f16"), 5)
    wide = E.cross_domain_knn_store(model, _store("clean", "f16w"), _store("noisy", "f16w"), 5)
    assert _same_result(cross["noisy_to_clean"], wide["noisy_to_clean"])


def test_neighbourhood_report_of_two_models():
    model, clean, noisy = _model(), _store("clean"), _store("noisy")
    other = PKG.SSRLModel().cuda()
    with torch.no_grad():
        other.student_flat.copy_(model.teacher_flat)
        other.teacher_flat.copy_(model.teacher_flat)
    rep = E.neighbourhood_report(model, other, clean, noisy, k=3)
    assert PKG.neighbourhood_report is E.neighbourhood_report and PKG.knn is E.knn
    for side, m in (("initial_weights", model), ("trained_weights", other)):
        cross = E.cross_domain_knn_store(m, clean, noisy, 3)
        assert rep[side] == {"noisy_knn_accuracy": E.knn_store(m, noisy, 3)["accuracy"],
                             "noisy_to_clean_accuracy": cross["noisy_to_clean"]["accuracy"],
                             "clean_to_noisy_accuracy": cross["clean_to_noisy"]["accuracy"]}
    for key, v in rep["improvement"].items():
        name = key[:-len("_change")]
        assert v == rep["trained_weights"][name] - rep["initial_weights"][name]


# ---------------------------------------------------------------- 9. tsne_report
def test_tsne_report_carries_the_trustworthiness_of_its_maps():
    model, store = _model(), _store("noisy")
    other = PKG.SSRLModel().cuda()
    with torch.no_grad():
        other.student_flat.copy_(model.teacher_flat)
        other.teacher_flat.copy_(model.teacher_flat)
    base = E.tsne_report(model, other, store, perplexity=10.0, max_iter=60)
    assert sorted(base) == ["class_counts", "initial", "kl_divergence", "labels", "n_iter", "trained"]
    rep = E.tsne_report(model, other, store, trustworthiness_k=5, perplexity=10.0, max_iter=60)
    assert sorted(rep) == sorted(list(base) + ["trustworthiness"])
    for key in ("initial", "trained"):
        assert np.array_equal(rep[key], base[key])
    for side, m in enumerate((model, other)):
        t = E.trustworthiness(E.embed_store(m, store), _dev(rep["initial" if side == 0 else "trained"]), 5)
        assert rep["trustworthiness"][side] == t["trustworthiness"] and 0.0 < t["trustworthiness"] <= 1.0


# ---------------------------------------------------------------- 10. graph capture
def test_captured_knn_and_vote_replay_like_eager():
    model, store = _model(), _store("noisy")
    plan = E.EvalPlan.of(store)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        want = E.knn_store(model, store, 5)          # (lazy buffers, then the eager result)
        want_idx, want_d2 = plan._knn[(41, 5)]["idx"].clone(), plan._knn[(41, 5)]["d2"].clone()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        bufs = E.enqueue_knn_store(model, plan, 5)
    for _ in range(2):
        for key in ("result_d", "idx", "pred"):
            bufs[key].fill_(-7)
        bufs["d2"].fill_(-1.0)
        g.replay()
        torch.cuda.synchronize()
        assert bufs["result_d"].cpu().numpy().tobytes() == want["block"].tobytes()
        assert torch.equal(bufs["idx"], want_idx) and torch.equal(bufs["d2"].view(torch.int32), want_d2.view(torch.int32))
        assert torch.equal(bufs["pred"], want["pred"])


def test_captured_trustworthiness_replays_like_eager():
    emb, _, Y, _ = _case(129)
    x, y = _dev(emb), _dev(Y)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        want = E.trustworthiness(x, y, 5, samples=True)
        ws = E._knn_workspace(129, 5, x.device)
        out = torch.empty(L.TW_SLOTS, dtype=torch.float64, device="cuda")
        pen = torch.empty(129, dtype=torch.int32, device="cuda")
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        E._enqueue_trustworthiness(x, y, 5, out, pen, ws)
    for _ in range(2):
        out.fill_(-1.0)
        pen.fill_(-1)
        g.replay()
        torch.cuda.synchronize()
        assert out.cpu().numpy().tobytes() == want["block"].tobytes() and torch.equal(pen, want["penalty"])
