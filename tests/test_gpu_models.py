"""Several networks on one split on the MI355X (evaluate.py *_models* + csrc/eval_models.hip): every per-model output
against dad_eval_split with that network as student, bit for bit; the counts, the vote, the ensemble and the sums
against the float64 restatement tests/models_ref.py on the device's own probabilities; the reference model's golden
numbers (tests/golden/eval_models.npz); buffer hygiene and the error paths.

Bounds.  ens_probs: the fp32 chain of K fused multiply-adds on values in [0, 1] has at most K roundings of 2^-24
each against the float64 chain.  ens_score: 1e-6, the project's bound for dad_certainty_scores.  sums: the device
adds n float64 terms in a tree-like order (at most n roundings of relative 2^-53 on partial sums bounded by
sum |terms|), and each term carries a few ulp of its log and products: (n + 8) * 2^-53 * sum |terms|."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import dadpkg
import gpu_harness as gh
import models_ref as mr
from golden import gen_models_golden as gm
from oracle import data_oracle as do

pytestmark = pytest.mark.gpu
PKG = dadpkg.pkg()
D = PKG.data
E = PKG.evaluate
L_ = PKG._lib

DTYPES = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}
PER_MODEL = ("emb", "logits", "probs", "score", "pred")
PER_UTT = ("ens_probs", "ens_score", "ens_pred", "vote_pred", "votes", "n_correct")


@functools.lru_cache(None)
def _flats(which):
    """The networks as flat float32 device tensors: 'main' eight (student and teacher of eval_weights(11 .. 14)),
    'golden' the fixture's four."""
    nets = gm.networks() if which == "golden" else [p for s in (11, 12, 13, 14) for p in do.eval_weights(s)]
    return tuple(torch.from_numpy(gh.flat(p)).cuda() for p in nets)


def _nets(which, K):
    return list(_flats("golden" if which == "golden" else "main")[:K])


@functools.lru_cache(None)
def _inputs(which):
    """(feats f32 [frames, 768], sizes, offsets, labels, subset order).  'main': 39 rows over 37 utterances, lengths
    around every slab boundary plus 27 seeded draws, read through a shuffled subset that repeats two samples (rows
    neither sorted nor unique); 'odd': 'main' without one one-slab row (the other slab parity); 'single': one
    utterance of one frame (slabs = 1); 'empty': three rows without frames (slabs = 0); 'golden': the fixture."""
    if which == "golden":
        feats, sizes, offsets = gm.inputs()
        labels = np.array([0, 1, 2, 3, -1, 1, 2])
        return feats, sizes, offsets, labels.astype(np.int64), np.arange(len(sizes))
    if which == "single":
        sizes, order, labels = np.array([1]), np.array([0]), np.array([2])
    elif which == "empty":
        sizes, order, labels = np.array([0, 5, 0]), np.array([0, 2, 0]), np.array([1, 2, 3])
    else:
        sizes = np.concatenate([[0, 1, 3, 31, 32, 33, 63, 64, 65, 96], np.random.RandomState(13).randint(1, 71, 27)])
        labels = np.random.RandomState(14).randint(0, 4, len(sizes))
        labels[[5, 20]] = -1
        perm = np.random.RandomState(15).permutation(len(sizes))
        order = np.concatenate([perm[:30], [perm[3], perm[11]], perm[30:]])      # two samples twice
        if which == "odd":
            drop = int(np.where(sizes[order] == 3)[0][0])
            order = np.delete(order, drop)
    offsets = np.concatenate([[0], np.cumsum(sizes)[:-1]])
    feats = np.random.RandomState(12).standard_normal((int(sizes.sum()), 768)).astype(np.float32)
    return feats, sizes, offsets, labels.astype(np.int64), order


@functools.lru_cache(None)
def _store(which, dt, labelled=True):
    feats, sizes, offsets, labels, order = _inputs(which)
    base = D.FeatureStore(feats, sizes, offsets, labels if labelled else None, dtype=DTYPES[dt])
    return base.subset(order)


def test_the_splits_cover_both_slab_parities_and_the_edges():
    slabs = {w: E.EvalPlan.of(_store(w, "f32")).slabs for w in ("main", "odd", "single", "empty", "golden")}
    assert slabs["main"] % 2 != slabs["odd"] % 2 and slabs["odd"] == slabs["main"] - 1
    assert slabs["single"] == 1 and slabs["empty"] == 0 and slabs["golden"] == 10
    assert E.EvalPlan.of(_store("main", "f32")).n == 39


@functools.lru_cache(None)
def _scratch_model():
    return PKG.SSRLModel().cuda()


def _split_outputs(flat, plan, precision, use_entropy=True):
    """dad_eval_split with `flat` as student over the plan: its five per-utterance outputs on the host."""
    model = _scratch_model()
    with torch.no_grad():
        model.student_flat.copy_(flat)
    out = E.enqueue_eval_split(model, plan, False, use_entropy, precision, PER_MODEL)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


@functools.lru_cache(None)
def _split_reference(which, dt, precision, k):
    """Computed once per (split, store type, precision, network), never modified."""
    return _split_outputs(_flats("golden" if which == "golden" else "main")[k], E.EvalPlan.of(_store(which, dt)),
                          precision)


def _host(res, names):
    return {k: res[k].cpu().numpy() for k in names}


def _assert_per_model_identity(got, want_list):
    for k, want in enumerate(want_list):
        for name in PER_MODEL:
            assert got[name][k].tobytes() == want[name].tobytes(), (k, name)


CASES = [("main", 1), ("main", 2), ("main", 3), ("main", 8), ("odd", 1), ("odd", 3), ("odd", 8), ("single", 1),
         ("single", 2), ("empty", 3), ("golden", 4)]


@pytest.mark.parametrize("dt", ["f32", "f16", "bf16"])
@pytest.mark.parametrize("precision", ["fp32", "fp16"])
@pytest.mark.parametrize("which,K", CASES)
def test_every_model_equals_dad_eval_split_bit_for_bit(which, K, precision, dt):
    store = _store(which, dt)
    res = E.evaluate_models_store(_nets(which, K), store, precision=precision, outputs=PER_MODEL)
    got = _host(res, PER_MODEL)
    assert got["emb"].shape == (K, len(store), 256) and got["pred"].shape == (K, len(store))
    _assert_per_model_identity(got, [_split_reference(which, dt, precision, k) for k in range(K)])
    if which == "empty":
        for k, f in enumerate(_nets(which, K)):
            assert not got["emb"][k].any()
            np.testing.assert_array_equal(got["logits"][k], np.tile(f[-4:].cpu().numpy(), (3, 1)))    # logits = b2
    assert res["K"] == K and res["n"] == len(store) and not res["nonfinite"].any()


@pytest.mark.parametrize("precision", ["fp32", "fp16"])
def test_use_entropy_off_equals_dad_eval_split(precision):
    plan = E.EvalPlan.of(_store("main", "f32"))
    nets = _nets("main", 3)
    out = E.enqueue_eval_models(nets, plan, use_entropy=False, precision=precision, outputs=PER_MODEL)
    torch.cuda.synchronize()
    _assert_per_model_identity(_host(out, PER_MODEL), [_split_outputs(f, plan, precision, False) for f in nets])


@pytest.mark.parametrize("precision", ["fp32", "fp16"])
def test_inconsistent_slab_table_gives_a_zero_embedding(precision):
    """An utterance whose length disagrees with its table entries: a zero embedding and logits = b2, as
    dad_eval_split; its slabs without valid rows read nothing (they share waves with valid neighbours)."""
    store = _store("main", "f32")
    for short in (10, 40):
        plan = E.EvalPlan(store)
        i = int(np.where(store.sizes == 65)[0][0])              # three slabs in the table
        lens = plan.lens_d.clone()
        lens[i] = short                                         # one or two slabs by its length
        plan.lens_d = lens
        nets = _nets("main", 3)
        out = E.enqueue_eval_models(nets, plan, precision=precision, outputs=PER_MODEL + PER_UTT)
        torch.cuda.synchronize()
        got = _host(out, PER_MODEL)
        _assert_per_model_identity(got, [_split_outputs(f, plan, precision) for f in nets])
        for k, f in enumerate(nets):
            assert not got["emb"][k, i].any()
            np.testing.assert_array_equal(got["logits"][k, i], f[-4:].cpu().numpy())


def test_student_and_teacher_give_dad_eval_splits_counts():
    model = PKG.SSRLModel().cuda()
    flats = _flats("main")
    with torch.no_grad():
        model.student_flat.copy_(flats[0])
        model.teacher_flat.copy_(flats[1])
    for dt in ("f32", "bf16"):
        store = _store("main", dt)
        want = E.evaluate_store(model, store, use_teacher=True)
        res = E.evaluate_models_store([model, (model, "teacher")], store)
        np.testing.assert_array_equal(res["confusion"][0], want["confusion_student"])
        np.testing.assert_array_equal(res["confusion"][1], want["confusion_teacher"])
        assert res["disagree"][0, 1] == res["disagree"][1, 0] == want["disagree"] > 0
        assert (res["n"], res["n_labelled"], res["n_skipped"]) == (want["n"], want["n_labelled"], want["n_skipped"])
        assert res["n_skipped"] == 2


def test_the_same_network_twice():
    flats = _flats("main")
    res = E.evaluate_models_store([flats[0], flats[2], flats[0]], _store("main", "f32"), outputs=PER_MODEL)
    got = _host(res, PER_MODEL)
    for name in PER_MODEL:
        assert got[name][0].tobytes() == got[name][2].tobytes(), name
    assert res["disagree"][0, 2] == res["disagree"][2, 0] == 0 and res["only"][0, 2] == res["only"][2, 0] == 0
    assert res["disagree"][0, 1] > 0 and res["only"][0, 0] == res["only"][2, 2]
    np.testing.assert_array_equal(res["confusion"][0], res["confusion"][2])


@pytest.mark.parametrize("precision", ["fp32", "fp16"])
def test_permuting_the_models_permutes_their_outputs(precision):
    flats = _flats("main")
    perm = [2, 0, 3, 1]
    store = _store("main", "f16")
    a = E.evaluate_models_store([flats[k] for k in range(4)], store, precision=precision, outputs=PER_MODEL)
    ga = _host(a, PER_MODEL)
    b = E.evaluate_models_store([flats[k] for k in perm], store, precision=precision, outputs=PER_MODEL)
    gb = _host(b, PER_MODEL)
    for j, k in enumerate(perm):
        for name in PER_MODEL:
            assert gb[name][j].tobytes() == ga[name][k].tobytes(), (name, j)
        np.testing.assert_array_equal(b["confusion"][j], a["confusion"][k])
        assert b["nonfinite"][j] == a["nonfinite"][k]
        for name in ("sum_score", "sum_entropy", "sum_nll", "sum_brier"):
            assert b[name][j] == a[name][k], name                     # the same terms in the same order
    np.testing.assert_array_equal(b["disagree"][:4, :4], a["disagree"][:4, :4][np.ix_(perm, perm)])
    np.testing.assert_array_equal(b["only"][:4, :4], a["only"][:4, :4][np.ix_(perm, perm)])
    np.testing.assert_array_equal(b["hist"], a["hist"])
    np.testing.assert_array_equal(b["confusion"][5], a["confusion"][5])          # the vote does not depend on the order


def ref_labels(labels, n):
    return np.full(n, -1, np.int64) if labels is None else labels


def _check_against_reference(res, labels, K, weights, use_entropy=True):
    got = _host(res, PER_MODEL + PER_UTT)
    n = got["pred"].shape[1]
    ref = mr.block(L_, got["probs"], got["pred"], got["score"], labels, weights, use_entropy)
    counts = res["block"][:L_.EM_COUNTS]
    np.testing.assert_array_equal(counts, ref["counts"])
    np.testing.assert_array_equal(got["votes"], ref["votes"])
    np.testing.assert_array_equal(got["vote_pred"], ref["vote_pred"])
    np.testing.assert_array_equal(got["n_correct"], ref["n_correct"])
    np.testing.assert_array_equal(got["ens_pred"], ref["ens_pred"])
    np.testing.assert_array_equal(got["ens_pred"], got["ens_probs"].argmax(1))
    err = np.abs(got["ens_probs"].astype(np.float64) - ref["ens64"]).max()
    print("K=%d: worst |ens_probs - float64 chain| = %.3e (bound %.3e)" % (K, err, K * 2.0 ** -24))
    assert err <= K * 2.0 ** -24
    serr = np.abs(got["ens_score"].astype(np.float64) - mr.certainty64(got["ens_probs"], use_entropy)).max()
    print("K=%d: worst |ens_score - float64| = %.3e" % (K, serr))
    assert serr <= 1e-6
    # sums: the ensemble's terms from the device's own ens_probs / ens_score
    sums = res["block"][L_.EM_COUNTS:].view(np.float64)
    want, wabs = ref["sums"].copy(), ref["sums_abs"].copy()
    ent, nll, brier = mr.terms(got["ens_probs"], ref_labels(labels, n))
    for slot, t in ((L_.EM_SUM_SCORE, got["ens_score"].astype(np.float64)), (L_.EM_SUM_ENTROPY, ent),
                    (L_.EM_SUM_NLL, nll), (L_.EM_SUM_BRIER, brier)):
        want[slot + K], wabs[slot + K] = t.sum(), np.abs(t).sum()
    lim = (n + 8) * 2.0 ** -53 * wabs
    worst = np.max(np.abs(sums - want) / np.maximum(lim, 1e-300))
    print("K=%d: worst |sum - float64| / bound = %.3f" % (K, worst))
    assert np.all(np.abs(sums - want) <= lim), (sums - want, lim)
    for m in range(K + 1, L_.EM_MEMBERS):
        assert not sums[m::L_.EM_MEMBERS].any()
    return ref


@pytest.mark.parametrize("precision", ["fp32", "fp16"])
@pytest.mark.parametrize("which,K,weights", [("main", 1, None), ("main", 2, [1.0, 3.0]), ("main", 3, None),
                                             ("main", 8, None), ("odd", 8, [1, 2, 3, 4, 5, 6, 7, 0]),
                                             ("golden", 4, None), ("empty", 3, None)])
def test_counts_vote_ensemble_and_sums_match_the_reference(which, K, weights, precision):
    store = _store(which, "f32")
    res = E.evaluate_models_store(_nets(which, K), store, weights=weights, precision=precision,
                                  outputs=PER_MODEL + PER_UTT)
    ref = _check_against_reference(res, store.labels, K, weights)
    if which == "main" and K >= 3:
        # the case is not trivial: the models disagree, the vote has ties, some utterance splits the models
        assert res["disagree"][0, 1] > 0 and (ref["votes"].max(1) < K).any()
        assert ((ref["votes"] == ref["votes"].max(1, keepdims=True)).sum(1) > 1).any()
        assert res["hist"][1:K].sum() > 0


def test_use_entropy_off_ensemble_score():
    store = _store("main", "f32")
    res = E.evaluate_models_store(_nets("main", 3), store, use_entropy=False, outputs=PER_MODEL + PER_UTT)
    _check_against_reference(res, store.labels, 3, None, use_entropy=False)
    np.testing.assert_array_equal(res["ens_score"].cpu().numpy(), res["ens_probs"].cpu().numpy().max(1))


def test_golden_logits_probabilities_and_every_argmax():
    g = np.load(dadpkg.ROOT + "/tests/golden/eval_models.npz")
    res = E.evaluate_models_store(_nets("golden", 4), _store("golden", "f32"),
                                  outputs=("logits", "probs", "pred", "ens_probs", "ens_pred"))
    np.testing.assert_allclose(res["logits"].cpu().numpy(), g["logits"], rtol=1e-5, atol=1e-4)
    np.testing.assert_allclose(res["probs"].cpu().numpy(), g["probs"], rtol=0, atol=1e-6)
    np.testing.assert_allclose(res["ens_probs"].cpu().numpy(), g["ens_probs"], rtol=0, atol=1e-6)
    np.testing.assert_array_equal(res["pred"].cpu().numpy(), g["pred"])
    np.testing.assert_array_equal(res["ens_pred"].cpu().numpy(), g["ens_pred"])


@pytest.mark.parametrize("precision", ["fp32", "fp16"])
def test_one_model_is_its_own_ensemble_and_vote(precision):
    store = _store("main", "bf16")
    res = E.evaluate_models_store(_nets("main", 1), store, weights=[2.5], precision=precision,
                                  outputs=PER_MODEL + PER_UTT)
    got = _host(res, PER_MODEL + PER_UTT)
    assert got["ens_probs"].tobytes() == got["probs"][0].tobytes()
    np.testing.assert_array_equal(got["ens_pred"], got["pred"][0])
    np.testing.assert_array_equal(got["vote_pred"], got["pred"][0])
    np.testing.assert_array_equal(res["confusion"][0], res["confusion"][1])
    np.testing.assert_array_equal(res["confusion"][0], res["confusion"][2])
    assert not res["disagree"].any()


# ---------------------------------------------------------------- the C entry point with the test's own buffers
GUARD = 256
_SPECS = (("emb", 256 * 4, True), ("logits", 16, True), ("probs", 16, True), ("score", 4, True), ("pred", 8, True),
          ("ens_probs", 16, False), ("ens_score", 4, False), ("ens_pred", 8, False), ("vote_pred", 8, False),
          ("votes", 16, False), ("n_correct", 4, False), ("counts", 8 * L_.EM_COUNTS, None),
          ("sums", 8 * L_.EM_SUMS, None))


def _raw_call(plan, flats, precision, want, ws_fill=None):
    """dad_eval_models on buffers carved from one arena pre-filled with 0xA5, GUARD bytes around each: returns
    ({name: host bytes}, guards intact).  `want` names the optional outputs to pass (the others are NULL)."""
    K, n = len(flats), plan.n
    layout, off = {}, GUARD
    for name, per, per_model in _SPECS:
        if per_model is None or name in want:
            size = per if per_model is None else per * n * (K if per_model else 1)
            layout[name] = (off, size)
            off = (off + size + GUARD + 255) // 256 * 256
    arena = torch.full((off + GUARD,), 0xA5, dtype=torch.uint8, device=plan.device)
    prec = {"fp32": L_.PREC_FP32, "fp16": L_.PREC_FP16}[precision]
    need = int(L_.lib().dad_eval_models_workspace_bytes(n, plan.slabs, K, prec))
    ws = torch.empty(need + 2 * GUARD, dtype=torch.uint8, device=plan.device)
    ws.fill_(0xA5 if ws_fill is None else ws_fill)
    a = L_.DadModelsArgs()
    a.store = plan.store.feats.data_ptr()
    a.rows, a.lens, a.slab_off = plan.rows_d.data_ptr(), plan.lens_d.data_ptr(), plan.slab_off_d.data_ptr()
    a.labels = None if plan.labels_d is None else plan.labels_d.data_ptr()
    a.n, a.slabs, a.K = n, plan.slabs, K
    a.store_dtype, a.use_entropy, a.precision = D.STORE_DTYPES[plan.store.feats.dtype], 1, prec
    for k, f in enumerate(flats):
        a.models[k], a.weight[k] = f.data_ptr(), 1.0
    for name, (o, _) in layout.items():
        setattr(a, name, arena.data_ptr() + o)
    L_.check(L_.lib().dad_eval_models(a, ctypes.c_void_p(ws.data_ptr() + GUARD),
                                      torch.cuda.current_stream(plan.device).cuda_stream), "dad_eval_models")
    torch.cuda.synchronize()
    host, wh = arena.cpu().numpy(), ws.cpu().numpy()
    keep = np.ones(len(host), bool)
    for o, size in layout.values():
        keep[o:o + size] = False
    intact = bool((host[keep] == 0xA5).all())
    if ws_fill is None:
        intact = intact and bool((wh[:GUARD] == 0xA5).all() and (wh[GUARD + need:] == 0xA5).all())
    return {name: host[o:o + size].tobytes() for name, (o, size) in layout.items()}, intact


@pytest.mark.parametrize("precision", ["fp32", "fp16"])
@pytest.mark.parametrize("which,K", [("main", 3), ("odd", 8), ("single", 1)])
def test_buffer_hygiene(which, K, precision):
    """Two calls give the same bits; a workspace pre-filled with 0xFF bytes gives the same bits (nothing of it is
    read before it is written); the guard bytes around every output and the workspace stay intact; leaving the
    optional outputs NULL changes nothing else."""
    plan = E.EvalPlan.of(_store(which, "f32"))
    flats = _nets(which, K)
    everything = [s[0] for s in _SPECS]
    a, ok_a = _raw_call(plan, flats, precision, everything)
    b, ok_b = _raw_call(plan, flats, precision, everything, ws_fill=0xFF)
    c, ok_c = _raw_call(plan, flats, precision, ())
    d, ok_d = _raw_call(plan, flats, precision, ("pred", "votes"))
    assert ok_a and ok_b and ok_c and ok_d
    assert sorted(a) == sorted(everything) and sorted(c) == ["counts", "sums"]
    for name in everything:
        assert a[name] == b[name], name
    for name in ("counts", "sums"):
        assert a[name] == c[name] == d[name], name
    assert d["pred"] == a["pred"] and d["votes"] == a["votes"]
    # and the Python path agrees with the raw call
    res = E.evaluate_models_store(flats, plan, precision=precision, outputs=("emb",))
    assert res["block"].tobytes() == a["counts"] + a["sums"]
    assert res["emb"].cpu().numpy().tobytes() == a["emb"]


def test_unlabelled_store_skips_every_utterance():
    store = _store("main", "f32", False)
    res = E.evaluate_models_store(_nets("main", 3), store, outputs=PER_MODEL + PER_UTT)
    assert res["n_skipped"] == res["n"] == 39 and res["n_labelled"] == 0
    assert not res["confusion"].any() and not res["only"].any() and not res["hist"].any()
    assert (res["n_correct"].cpu().numpy() == -1).all()
    assert not res["sum_nll"].any() and not res["sum_brier"].any() and res["sum_entropy"].all()
    lab = E.evaluate_models_store(_nets("main", 3), _store("main", "f32"))
    np.testing.assert_array_equal(res["disagree"], lab["disagree"])
    _check_against_reference(res, None, 3, None)


def test_nonfinite_features_are_counted_per_model_and_raise():
    rs = np.random.RandomState(3)
    sizes = np.array([5, 40, 2, 33, 7])
    offsets = np.concatenate([[0], np.cumsum(sizes)[:-1]])
    feats = rs.standard_normal((int(sizes.sum()), 768)).astype(np.float32)
    labels = np.array([0, 1, 2, 3, 0])
    nets = _nets("main", 3)
    assert not E.evaluate_models_store(nets, D.FeatureStore(feats, sizes, offsets, labels))["nonfinite"].any()
    feats[offsets[3] + 32, 100] = np.inf        # the one frame of utterance 3's second slab
    feats[offsets[0] + 1, 7] = np.nan
    store = D.FeatureStore(feats, sizes, offsets, labels)
    with pytest.raises(L_.DadError, match=r"model\(s\) \[0, 1, 2\].*\[2, 2, 2\] of 5 utterance"):
        E.evaluate_models_store(nets, store)
    plan = E.EvalPlan.of(store)
    E.enqueue_eval_models(nets, plan)
    torch.cuda.synchronize()
    block = E._models_buffers(plan)["result_d"].cpu().numpy()
    np.testing.assert_array_equal(block[L_.EM_NONFINITE:L_.EM_NONFINITE + 8], [2, 2, 2, 0, 0, 0, 0, 0])


def test_model_forms_and_the_report(tmp_path):
    """SSRLModels, (model, role) pairs, flat tensors and checkpoint paths name the same weights; ensemble_report
    reads one block."""
    flats = _flats("main")
    model = PKG.SSRLModel().cuda()
    with torch.no_grad():
        model.student_flat.copy_(flats[0])
        model.teacher_flat.copy_(flats[1])
    other = PKG.SSRLModel().cuda()
    with torch.no_grad():
        other.student_flat.copy_(flats[2])
    path = tmp_path / "best_model_fold_0.ckpt"
    torch.save({"epoch": 3, "model_state_dict": {k: v.detach().cpu() for k, v in other.state_dict().items()}}, path)
    store = _store("main", "f32")
    a = E.evaluate_models_store([model, (model, "teacher"), str(path)], store, outputs=("logits",))
    b = E.evaluate_models_store(list(flats[:3]), store, outputs=("logits",))
    assert a["block"].tobytes() == b["block"].tobytes() and torch.equal(a["logits"], b["logits"])
    rep = E.ensemble_report([model, (model, "teacher"), str(path)], store, weights=[2, 1, 1])
    want = E.ensemble_from_block(E.evaluate_models_store(list(flats[:3]), store, weights=[2, 1, 1]))
    assert rep["diversity"] == want["diversity"] > 0 and rep["best_single"] == want["best_single"]
    assert rep["oracle_accuracy"] >= max(m["accuracy"] for m in rep["members"][:3])
    assert 0.0 <= rep["pairs"][0]["p_value"] <= 1.0 and len(rep["pairs"]) == 10
    with pytest.raises(ValueError):
        E.evaluate_models_store([], store)
    with pytest.raises(ValueError):
        E.evaluate_models_store([model] * 9, store)
    with pytest.raises(L_.DadError, match="DAD_E_UNSUPPORTED"):
        E.evaluate_models_store([model], store, precision="bf16")
