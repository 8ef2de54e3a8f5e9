"""Whole-split evaluator on the MI355X (evaluate.py *_store + csrc/eval_split.hip): per-utterance
outputs against a torch fp32 restatement (the one of test_predict_head_matches_torch_fp32, per
utterance on its valid rows, computed once on the CPU), the result block against NumPy on the
kernel's own outputs, the reference trainer's golden numbers (tests/golden/eval_iemocap.npz), the
FP16 operand mode's error, determinism / plan reuse, and the error paths."""
import functools

import numpy as np
import pytest
import torch

import dadpkg
import gpu_harness as gh
from oracle import data_oracle as do
from split_scale import block_from_outputs as _block_from_outputs
from test_data_cpu import _golden

pytestmark = pytest.mark.gpu
PKG = dadpkg.pkg()
D = PKG.data
E = PKG.evaluate

DTYPES = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}
# FP16 operand mode: worst |logit - torch fp32| / max |torch logit| over student and teacher on the f32 store
# of _inputs(), measured on the MI355X: 5.79e-4 (the teacher; the student 2.74e-4.  f16 store 4.21e-4, bf16
# store 4.20e-4: rows exact there, only W1 is rounded).  A float64 CPU simulation with fp16-rounded rows and W1
# gives 5.78e-4, so this is the operands' rounding, not the kernel's summation.  The kernel is deterministic;
# the factor 2 guards against a recompilation's summation order.
FP16_MEASURED = 5.79e-4
FP16_BOUND = 2 * FP16_MEASURED


@functools.lru_cache(None)
def _model(seed=11):
    stu, tea = do.eval_weights(seed)
    model = PKG.SSRLModel().cuda()
    with torch.no_grad():
        model.student_flat.copy_(torch.from_numpy(gh.flat(stu)))
        model.teacher_flat.copy_(torch.from_numpy(gh.flat(tea)))
    return model


@functools.lru_cache(None)
def _inputs(which):
    """(feats f32 [frames, 768], sizes, offsets, labels, subset order).  'main': 37 utterances, lengths
    around every slab boundary plus 27 seeded draws, read through a shuffled subset that repeats two
    samples (rows neither sorted nor unique); 'single': one utterance of one frame."""
    if which == "single":
        sizes = np.array([1])
        order = np.array([0])
        labels = np.array([2])
    else:
        sizes = np.concatenate([[0, 1, 3, 31, 32, 33, 63, 64, 65, 96], np.random.RandomState(13).randint(1, 71, 27)])
        labels = np.random.RandomState(14).randint(0, 4, len(sizes))
        labels[[5, 20]] = -1
        perm = np.random.RandomState(15).permutation(len(sizes))
        order = np.concatenate([perm[:30], [perm[3], perm[11]], perm[30:]])      # two samples twice
        assert labels[perm[3]] >= 0 and labels[perm[11]] >= 0
    offsets = np.concatenate([[0], np.cumsum(sizes)[:-1]])
    feats = np.random.RandomState(12).standard_normal((int(sizes.sum()), 768)).astype(np.float32)
    return feats, sizes, offsets, labels.astype(np.int64), order


@functools.lru_cache(None)
def _store(which, dt):
    feats, sizes, offsets, labels, order = _inputs(which)
    base = D.FeatureStore(feats, sizes, offsets, labels, dtype=DTYPES[dt])
    return base.subset(order)


@functools.lru_cache(None)
def _reference(which, dt):
    """torch fp32 on the CPU, per utterance of the subset on its valid rows (widened store values):
    {'s' | 't': {emb, logits, probs, pred, score_entropy, score_max}}; computed once, never modified."""
    feats, sizes, offsets, _, order = _inputs(which)
    x = torch.from_numpy(feats).to(DTYPES[dt]).float()
    out = {}
    for key, params in zip("st", do.eval_weights(11)):
        W1, b1, W2, b2 = (torch.from_numpy(np.asarray(a, np.float32)) for a in params)
        with torch.no_grad():
            embs = []
            for i in order:
                rows = x[offsets[i]:offsets[i] + sizes[i]]
                h = torch.relu(rows @ W1.T + b1)
                embs.append(h.sum(0) / max(int(sizes[i]), 1))
            e = torch.stack(embs)
            z = e @ W2.T + b2
            p = torch.softmax(z, dim=1)
            mp, pred = torch.max(p, dim=1)
            ent = -(p * torch.log2(p + 1e-8)).sum(1)
        top2 = torch.sort(z, dim=1, descending=True).values
        out[key] = {"emb": e, "logits": z, "probs": p, "pred": pred, "score_entropy": mp * (1 - ent / np.log2(4)),
                    "score_max": mp, "gap": (top2[:, 0] - top2[:, 1]).numpy()}
    return out


def _decided(ref, min_gap):
    """Utterances whose torch prediction a logit error below min_gap / 2 cannot change; the filter may
    drop at most 5 % of them (asserted on the reference alone)."""
    ok = ref["gap"] > min_gap
    assert (~ok).mean() <= 0.05, "the reference itself has %d of %d near-ties" % ((~ok).sum(), len(ok))
    return torch.from_numpy(ok)


def _check_block(res, labels, with_teacher):
    cs, ct, dis, nl, nskip, mom = _block_from_outputs(res, labels, with_teacher)
    np.testing.assert_array_equal(res["confusion_student"], cs)
    np.testing.assert_array_equal(res["confusion_teacher"], ct)
    assert res["disagree"] == dis
    assert (res["n"], res["n_labelled"], res["n_skipped"], res["n_nonfinite"]) == (len(labels), nl, nskip, 0)
    np.testing.assert_array_equal(res["moments"][:, 0], mom[:, 0])
    np.testing.assert_allclose(res["moments"][:, 1:], mom[:, 1:], rtol=1e-12, atol=0)


ALL_S = ("emb", "logits", "probs", "score", "pred")
ALL_T = ("t_emb", "t_logits", "t_pred")


@pytest.mark.parametrize("with_teacher", [False, True])
@pytest.mark.parametrize("use_entropy", [True, False])
@pytest.mark.parametrize("dt", ["f32", "f16", "bf16"])
@pytest.mark.parametrize("which", ["main", "single"])
def test_fp32_matches_torch_fp32(which, dt, use_entropy, with_teacher):
    model, store, ref = _model(), _store(which, dt), _reference(which, dt)
    labels = store.labels
    res = E.evaluate_store(model, store, use_teacher=with_teacher, use_entropy=use_entropy,
                           outputs=ALL_S + (ALL_T if with_teacher else ()))
    for key, pre in (("s", ""),) + ((("t", "t_"),) if with_teacher else ()):
        r = ref[key]
        torch.testing.assert_close(res[pre + "emb"].cpu(), r["emb"], rtol=1e-5, atol=1e-4)
        torch.testing.assert_close(res[pre + "logits"].cpu(), r["logits"], rtol=1e-5, atol=1e-4)
        pred = res[pre + "pred"].cpu()
        assert torch.equal(pred, torch.argmax(res[pre + "logits"].cpu(), 1))
        ok = _decided(r, 2e-4)
        assert torch.equal(pred[ok], r["pred"][ok])
    r = ref["s"]
    torch.testing.assert_close(res["probs"].cpu(), r["probs"], rtol=1e-5, atol=1e-6)
    torch.testing.assert_close(res["score"].cpu(), r["score_entropy" if use_entropy else "score_max"],
                               rtol=1e-5, atol=1e-6)
    _check_block(res, labels, with_teacher)
    if which == "main":
        assert res["n"] == 39 and res["n_skipped"] == 2
        # the empty utterance: a zero embedding and logits = b2 (the reference's formula)
        i0 = int(np.where(store.sizes == 0)[0][0])
        assert torch.count_nonzero(res["emb"][i0]) == 0
        assert torch.equal(res["logits"][i0], model.student_classifier.fc_layer.bias.detach())


def test_unlabelled_store_skips_every_utterance():
    feats, sizes, offsets, _, order = _inputs("main")
    store = D.FeatureStore(feats, sizes, offsets, None).subset(order)
    res = E.evaluate_store(_model(), store, use_teacher=True)
    assert res["n_skipped"] == res["n"] == 39 and res["n_labelled"] == 0
    assert res["confusion_student"].sum() == 0 and res["confusion_teacher"].sum() == 0
    assert not res["moments"].any()
    assert res["disagree"] == E.evaluate_store(_model(), _store("main", "f32"), use_teacher=True)["disagree"]


def _golden_loaders(tmp_path, g):
    seed, bs, fold = int(g["seed"]), int(g["batch_size"]), int(g["fold"])
    do.write_synthetic_split(str(tmp_path), seed, n_utt=160, max_len=40, flavor="iemocap")
    _, cval, ctest, _, _ = D.get_cv_dataloaders(str(tmp_path), bs, fold_id=fold)
    nval = D.get_cv_dataloaders_noisy(str(tmp_path), bs, fold_id=fold)[2]
    ctrain = D.get_cv_dataloaders(str(tmp_path), 2 * bs, fold_id=fold)[0]
    return _model(seed), cval, ctest, nval, ctrain


def test_golden_validate_and_calibration(tmp_path):
    """The reference trainer's own validate() / _run_anchor_calibration() numbers, at the tolerances of
    test_validate_and_calibration_match_reference, and equality with the per-batch validate()."""
    g = _golden("eval_iemocap")
    model, cval, ctest, nval, ctrain = _golden_loaders(tmp_path, g)
    for name, ld, noisy in (("clean_val", cval, False), ("clean_test", ctest, False), ("noisy_val", nval, True)):
        r = E.validate_store(model, ld, teacher_disagreement=noisy)
        for k in ("accuracy", "weighted_accuracy", "f1_weighted", "f1_macro"):
            assert r[k] == pytest.approx(float(g["%s_%s" % (name, k)]), abs=1e-9), (name, k)
        for k in ("precision_per_class", "recall_per_class", "f1_per_class", "support_per_class"):
            np.testing.assert_allclose(r[k], g["%s_%s" % (name, k)], atol=1e-12, err_msg="%s %s" % (name, k))
        np.testing.assert_array_equal(r["confusion_matrix"], g[name + "_confusion_matrix"])
        if noisy:
            assert r["disagreement_rate"] == pytest.approx(float(g["noisy_val_disagreement_rate"]), abs=1e-12)
        old = E.validate(model, ld, teacher_disagreement=noisy)
        assert sorted(old) == sorted(r)
        for k in old:
            if k == "confusion_matrix":
                np.testing.assert_array_equal(r[k], old[k])
            elif isinstance(old[k], list):
                np.testing.assert_allclose(r[k], old[k], rtol=0, atol=1e-12, err_msg=k)
            else:
                assert r[k] == pytest.approx(old[k], abs=1e-9), k
    model.train()
    anchors = E.calibrate_anchors_store(model, ctrain, nval, anchor_std_k=float(g["anchor_std_k"]))
    assert model.training                                  # left as calibrate_anchors leaves it
    np.testing.assert_allclose(anchors.cpu().numpy(), g["calibrated_anchors"], rtol=1e-4, atol=1e-8)
    old = E.calibrate_anchors(model, ctrain, nval, anchor_std_k=float(g["anchor_std_k"]))
    np.testing.assert_allclose(anchors.cpu().numpy(), old.cpu().numpy(), rtol=1e-6, atol=1e-9)
    E.validate_store(model, cval)
    assert not model.training                              # validate() leaves eval mode on


def test_golden_fp16(tmp_path):
    """FP16 operands on the golden split: the student's confusion matrices are the golden ones (simulated
    worst logit error 1.1e-4 against a smallest top-two gap of 1.2e-3), the disagreement rate within two
    utterances of the golden one (two teacher utterances have a gap under twice the simulated error)."""
    g = _golden("eval_iemocap")
    model, cval, ctest, nval, _ = _golden_loaders(tmp_path, g)
    for name, ld, noisy in (("clean_val", cval, False), ("clean_test", ctest, False), ("noisy_val", nval, True)):
        r = E.validate_store(model, ld, teacher_disagreement=noisy, precision="fp16")
        np.testing.assert_array_equal(r["confusion_matrix"], g[name + "_confusion_matrix"])
        if noisy:
            n = len(ld.store)
            assert abs(r["disagreement_rate"] - float(g["noisy_val_disagreement_rate"])) <= 2.0 / n + 1e-12


@pytest.mark.parametrize("dt", ["f32", "f16", "bf16"])
def test_fp16_operands_error_bound(dt):
    model, store, ref = _model(), _store("main", dt), _reference("main", dt)
    res = E.evaluate_store(model, store, use_teacher=True, precision="fp16", outputs=ALL_S + ALL_T)
    worst = 0.0
    for key, pre in (("s", ""), ("t", "t_")):
        z = ref[key]["logits"]
        err = float((res[pre + "logits"].cpu() - z).abs().max() / z.abs().max())
        print("fp16 operands, %s store, %s: worst |logit - torch fp32| / max|logit| = %.3e" % (dt, key, err))
        worst = max(worst, err)
    assert worst <= FP16_BOUND, worst
    for key, pre in (("s", ""), ("t", "t_")):
        z = ref[key]["logits"]
        pred = res[pre + "pred"].cpu()
        assert torch.equal(pred, torch.argmax(res[pre + "logits"].cpu(), 1))
        ok = _decided(ref[key], 2 * FP16_BOUND * float(z.abs().max()))
        assert torch.equal(pred[ok], ref[key]["pred"][ok])
    _check_block(res, store.labels, True)


def test_deterministic_and_plans_do_not_interfere():
    model, store, other = _model(), _store("main", "f32"), _store("single", "f32")
    plan = E.EvalPlan.of(store)
    assert E.EvalPlan.of(store) is plan and E.EvalPlan.of(D.DeviceLoader(store, 8)) is plan
    assert E.EvalPlan.of(other) is not plan
    outs = ALL_S + ALL_T
    for precision in ("fp32", "fp16"):
        a = E.evaluate_store(model, plan, use_teacher=True, precision=precision, outputs=outs)
        mid = E.evaluate_store(model, other, use_teacher=True, precision=precision, outputs=outs)
        b = E.evaluate_store(model, store, use_teacher=True, precision=precision, outputs=outs)
        assert a["block"].tobytes() == b["block"].tobytes()
        assert mid["n"] == 1 and b["n"] == 39
        for k in outs:
            assert a[k].data_ptr() != b[k].data_ptr()
            assert torch.equal(a[k].view(torch.uint8), b[k].view(torch.uint8)), (precision, k)   # bit for bit
    a = E.evaluate_store(model, plan, use_teacher=True, outputs=("emb", "t_emb"))
    assert torch.equal(E.embed_store(model, store), a["emb"])
    assert torch.equal(E.embed_store(model, D.DeviceLoader(store, 8), use_teacher=True), a["t_emb"])


def test_fp32_embeddings_equal_the_per_batch_path():
    """FP32 keeps dad_encode_f32's k order, epilogue order and slab-order pooling, so the embeddings are the
    per-batch path's (collated batch -> SSRLModel.get_embeddings) bit for bit, the empty utterance included."""
    model, store = _model(), _store("main", "f32")
    batch = store.collate(np.arange(len(store)))
    ni = batch["net_input"]
    for use_teacher in (False, True):
        want = model.get_embeddings(ni["feats"], ni["padding_mask"], use_teacher=use_teacher)
        got = E.embed_store(model, store, use_teacher=use_teacher)
        assert torch.equal(got.view(torch.int32), want.view(torch.int32))


def test_bf16_operands_are_unsupported():
    with pytest.raises(PKG._lib.DadError, match="DAD_E_UNSUPPORTED"):
        E.evaluate_store(_model(), _store("main", "f32"), precision="bf16")


def test_nonfinite_features_are_reported_not_classified():
    rs = np.random.RandomState(3)
    sizes = np.array([5, 40, 2, 33, 7])
    offsets = np.concatenate([[0], np.cumsum(sizes)[:-1]])
    feats = rs.standard_normal((int(sizes.sum()), 768)).astype(np.float32)
    labels = np.array([0, 1, 2, 3, 0])
    assert E.evaluate_store(_model(), D.FeatureStore(feats, sizes, offsets, labels))["n_nonfinite"] == 0
    feats[offsets[3] + 32, 100] = np.inf        # the one frame of utterance 3's second slab
    with pytest.raises(PKG._lib.DadError, match="1 of 5 utterance"):
        E.evaluate_store(_model(), D.FeatureStore(feats, sizes, offsets, labels), use_teacher=True)
