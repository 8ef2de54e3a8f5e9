"""Eval path: validation metrics and anchor calibration on the device.

  validate            Trainer.validate                 I/train.py:522-564
  calibrate_anchors   Trainer._run_anchor_calibration  I/train.py:317-357
  predict_head        SSRLModel.predict + softmax + DACPManager.calculate_certainty_scores
                      (I/model.py:225-245, I/utils.py:401-430)

Every batch runs the HIP encoder forward (dad_encoder_forward, fp32 as the reference's eval) and
dad_predict_head (csrc/eval.hip: classifier, softmax, certainty score, argmax); predictions,
scores and labels stay on the device until one copy at the end of the loader, where the metrics
are computed with the same scikit-learn calls the reference makes.

For a split held in a FeatureStore, the whole-split forms do the same in one fused pass
(dad_eval_split, csrc/eval_split.hip) and report the same values:

  validate_store, calibrate_anchors_store, embed_store, evaluate_store, EvalPlan, metrics_from_confusion

and the class separation of a split's embeddings (dad_cluster_metrics, csrc/cluster.hip):

  cluster_metrics, cluster_metrics_store, separation_report
                      calculate_cluster_metrics / generate_analysis_report's `cluster_analysis`
                      (I/iemocap_plot_tsne.py:390-398, 428-442)

and the 2-D picture those scores describe (dad_tsne_*, csrc/tsne.hip):

  tsne_affinities, tsne_gradient, tsne, tsne_store, tsne_report
                      run_tsne: scikit-learn's TSNE(method='exact') (I/iemocap_plot_tsne.py:310-323, 524-525)

and the clean-noisy domain gap of two splits, the quantity the ECDA loss shrinks (dad_domain_gap, csrc/domain_gap.hip):

  domain_gap, domain_gap_store, enqueue_domain_gap_store, alignment_report
                      ECDALoss._gaussian_kernel / forward on whole splits (I/utils.py:510-652)

and the neighbour structure of a split's embeddings (dad_knn, dad_knn_vote, dad_trustworthiness, csrc/knn.hip):

  knn, knn_accuracy, knn_store, cross_domain_knn_store, trustworthiness, neighbourhood_report
                      not in the reference: scikit-learn's NearestNeighbors(brute), KNeighborsClassifier's vote and
                      sklearn.manifold.trustworthiness

and emotion over time, every sliding window or prefix of every utterance in one pass (dad_eval_windows,
csrc/eval_windows.hip):

  windows_host, window_frames, enqueue_eval_windows, evaluate_windows_store, early_decision_curve, duration_report,
  windows             SSRLModel.predict / get_embeddings (I/model.py:225-265) on the features cropped to each window

and the response to additive noise, every noise level of a draw in one pass (dad_eval_noise, csrc/eval_noise.hip):

  noise_draws, enqueue_eval_noise, evaluate_noise_store, noise_response_curve, robustness_report
                      SSRLModel.predict / get_embeddings on x + sigma * N, the perturbation of
                      DataAugmentation.weak_augment / strong_augment's noise term (I/utils.py:328-350)

and the worst perturbation of the same size, the gradient with respect to the stored rows (dad_input_grad,
csrc/input_grad.hip):

  enqueue_input_grad, input_gradients, evaluate_adversarial_store, adversarial_response_curve, worst_case_report
                      not in the reference (its inputs do not require grad): autograd of SSRLModel.predict with respect
                      to x, FGSM (Goodfellow et al. 2015) and PGD (Madry et al. 2018)

and why a split is classified as it is, exact integrated gradients of the stored rows (dad_attribution,
csrc/attribution.hip):

  enqueue_attribution, attribution_plan, integrated_gradients, saliency_report, saliency_from_attributions
                      not in the reference: integrated gradients (Sundararajan et al. 2017) of a fixed logit
                      cotangent along the straight path from a baseline frame, in closed form

and whether the certainty score that gates the pseudo-labels is any good, a split ranked by it (dad_rank_metrics,
dad_rank_eval_columns, csrc/rank.hip):

  rank_metrics, risk_coverage, roc_points, enqueue_certainty_ranking, certainty_ranking_store, firewall_report,
  reliability_report  DACPManager.calculate_mask's gate on a whole split (I/utils.py:449-507), confidence_stats
                      (I/inference.py:361-369); scikit-learn's roc_auc_score and average_precision_score, which the
                      reference does not call

and several networks on one split, up to 8 checkpoints in one store pass (dad_eval_models, csrc/eval_models.hip):

  enqueue_eval_models, evaluate_models_store, ensemble_report
                      what the reference does one network at a time: the fold checkpoints (best_model_fold_k.ckpt),
                      the ablation runners' BEST checkpoints, inference.py's weights over the same test sets
"""
import ctypes
import math
import warnings

import numpy as np
import torch

from . import _lib
from .data import STORE_DTYPES, StoreFeats


def _feats_mask(batch, device):
    ni = batch["net_input"]
    x = ni["feats"]
    if isinstance(x, StoreFeats):
        x = x.materialize()
    x = x.to(device=device, dtype=torch.float32).contiguous()
    pm = ni.get("padding_mask")
    pad = (torch.zeros(x.shape[0], x.shape[1], dtype=torch.bool, device=device) if pm is None
           else pm.to(device=device, dtype=torch.bool).contiguous())
    return x, pad


def predict_head(model, x, padding_mask=None, use_teacher=False, use_entropy=True):
    """Eval-mode logits, softmax probs, certainty scores and argmax preds of one batch (device)."""
    enc = model.teacher_encoder if use_teacher else model.student_encoder
    cls = model.teacher_classifier if use_teacher else model.student_classifier
    with torch.no_grad():
        e = enc(x, padding_mask).contiguous()
        B = e.shape[0]
        out = {"logits": torch.empty(B, 4, device=e.device), "probs": torch.empty(B, 4, device=e.device),
               "score": torch.empty(B, device=e.device), "pred": torch.empty(B, dtype=torch.int64, device=e.device)}
        w2 = cls.fc_layer.weight.detach().contiguous()
        b2 = cls.fc_layer.bias.detach().contiguous()
        _lib.check(_lib.lib().dad_predict_head(
            _lib.ptr(e), B, _lib.ptr(w2), _lib.ptr(b2), int(bool(use_entropy)), _lib.ptr(out["logits"]),
            _lib.ptr(out["probs"]), _lib.ptr(out["score"]), _lib.ptr(out["pred"]),
            torch.cuda.current_stream(e.device).cuda_stream), "dad_predict_head")
    return out


def _collect(model, loader, use_teacher, want_labels, use_entropy=True):
    dev = model.student_flat.device
    preds, scores, labels = [], [], []
    for batch in loader:
        x, pad = _feats_mask(batch, dev)
        o = predict_head(model, x, pad, use_teacher=use_teacher, use_entropy=use_entropy)
        preds.append(o["pred"])
        scores.append(o["score"])
        if want_labels:
            labels.append(batch["labels"].to(device=dev, dtype=torch.int64))
    cat = lambda ts: torch.cat(ts).cpu().numpy() if ts else np.zeros(0)
    return cat(preds), cat(scores), (cat(labels) if want_labels else None)


def validate(model, data_loader, domain_name="unknown", num_classes=4, teacher_disagreement=False):
    """Trainer.validate (I/train.py:522-564): student predictions over the loader; with
    teacher_disagreement (the reference does it for noisy domains after warm-up) also the
    fraction of utterances where the teacher's argmax differs ('disagreement_rate')."""
    from sklearn.metrics import (accuracy_score, balanced_accuracy_score, confusion_matrix, f1_score,
                                 precision_recall_fscore_support)
    model.eval()
    preds, _, labels = _collect(model, data_loader, False, True)
    res = {}
    if teacher_disagreement:
        tp, _, _ = _collect(model, data_loader, True, False)
        if len(tp) == len(preds):
            res["disagreement_rate"] = float(np.mean(preds != tp))
    labs = range(num_classes)
    cm = confusion_matrix(labels, preds, labels=labs)
    prec, rec, f1, sup = precision_recall_fscore_support(labels, preds, average=None, zero_division=0, labels=labs)
    res.update({
        "accuracy": accuracy_score(labels, preds) * 100,
        "weighted_accuracy": balanced_accuracy_score(labels, preds) * 100,
        "f1_weighted": f1_score(labels, preds, average="weighted", zero_division=0) * 100,
        "f1_macro": f1_score(labels, preds, average="macro", zero_division=0) * 100,
        "precision_per_class": prec.tolist(), "recall_per_class": rec.tolist(),
        "f1_per_class": f1.tolist(), "support_per_class": sup.tolist(), "confusion_matrix": cm,
    })
    return res


def calibrate_anchors(model, clean_loader, noisy_loader, num_classes=4, anchor_std_k=1.5, use_entropy=True):
    """Trainer._run_anchor_calibration (I/train.py:317-357): per-class mean / std of the student's
    certainty scores on labeled clean and noisy data; anchors = clamp(mu_clean - k sigma_clean, 0)
    * mu_noisy / (mu_clean + 1e-8), float32 on the model's device (the `calibrated_anchors` input
    of DADStep).  Statistics in float64 over the float32 scores, as np.mean / np.std of .item()s."""
    model.eval()
    dev = model.student_flat.device
    stats = {}
    for name, loader in (("clean", clean_loader), ("noisy", noisy_loader)):
        _, s, y = _collect(model, loader, False, True, use_entropy=use_entropy)
        per = [s[y == c].astype(np.float64) for c in range(num_classes)]
        stats[name] = ([float(np.mean(v)) if len(v) else 0.0 for v in per],
                       [float(np.std(v)) if len(v) else 0.0 for v in per])
    mu_c = torch.tensor(stats["clean"][0], device=dev)
    mu_n = torch.tensor(stats["noisy"][0], device=dev)
    sd_c = torch.tensor(stats["clean"][1], device=dev)
    shift = mu_n / (mu_c + 1e-8)
    base = torch.clamp(mu_c - anchor_std_k * sd_c, min=0)
    model.train()
    return base * shift


# ------------------------------------------------------------------ whole-split, store-fed
# The functions above take any loader and work batch by batch (a padded batch, four output
# tensors and three launches per batch, a second sweep for the teacher, scikit-learn on
# per-utterance arrays).  Those below take a FeatureStore split: dad_eval_split
# (csrc/eval_split.hip) reads every utterance's rows in place, runs student and teacher on one
# read, and builds the confusion matrices, the disagreement count and the per-class score
# moments on the device; one copy of 52 words returns them.

_PRECISIONS = {"fp32": _lib.PREC_FP32, "fp16": _lib.PREC_FP16, "bf16": _lib.PREC_BF16}
_OUTPUTS = {"emb": ((256,), torch.float32), "logits": ((4,), torch.float32), "probs": ((4,), torch.float32),
            "score": ((), torch.float32), "pred": ((), torch.int64), "t_emb": ((256,), torch.float32),
            "t_logits": ((4,), torch.float32), "t_pred": ((), torch.int64)}
_RESULT_WORDS = _lib.EV_COUNTS + 4 * _lib.EV_MOMENTS


def plan_host(sizes, offsets):
    """The host side of an EvalPlan, a pure function of a store's per-sample sizes / offsets:
    (rows int64 [n], lens int32 [n], slab_off int32 [n + 1]).  Utterance i is store rows
    [rows[i], rows[i] + lens[i]) (row 0 for an empty one: nothing of it is read) and owns the
    32-frame slab jobs [slab_off[i], slab_off[i + 1]), ceil(lens[i] / 32) of them."""
    sizes = np.asarray(sizes, dtype=np.int64).reshape(-1)
    offsets = np.asarray(offsets, dtype=np.int64).reshape(-1)
    if sizes.shape != offsets.shape:
        raise ValueError("sizes and offsets differ in length")
    if len(sizes) and (sizes.min() < 0 or sizes.max() >= 2 ** 31):
        raise ValueError("sample sizes must be in [0, 2^31)")
    nslab = (sizes + 31) // 32
    slab_off = np.concatenate([[0], np.cumsum(nslab)])
    if slab_off[-1] >= 2 ** 31:
        raise ValueError("the split holds %d slabs; the evaluator indexes them with 32 bits" % slab_off[-1])
    rows = np.where(sizes > 0, offsets, 0).astype(np.int64)
    return rows, sizes.astype(np.int32), slab_off.astype(np.int32)


def slab_jobs(slab_off):
    """(utterance, slab within it) of every job of a plan_host prefix, by the kernel's rule: job j
    belongs to the largest i < n with slab_off[i] <= j."""
    slab_off = np.asarray(slab_off, dtype=np.int64)
    jobs = np.arange(slab_off[-1], dtype=np.int64)
    utt = np.searchsorted(slab_off[:-1], jobs, side="right") - 1
    return utt, jobs - slab_off[utt]


class EvalPlan:
    """Everything dad_eval_split needs about one split that does not change between epochs: the
    per-utterance rows / lengths / slab prefix on the device (built once with NumPy from the
    store's host sizes / offsets), the labels, and the reusable workspace and result buffers.
    Accepts a FeatureStore or a DeviceLoader over one (its .store; sample order is the store's
    and is irrelevant to every split-wide output).  EvalPlan.of caches the plan on the store."""

    def __init__(self, store_or_loader):
        store = getattr(store_or_loader, "store", store_or_loader)
        if not hasattr(store, "feats") or not hasattr(store, "offsets"):
            raise TypeError("EvalPlan needs a FeatureStore or a DeviceLoader over one, got %s"
                            % type(store_or_loader).__name__)
        rows, lens, slab_off = plan_host(store.sizes, store.offsets)
        if len(lens) == 0:
            raise ValueError("the split is empty")
        self.store = store
        self.n = len(lens)
        self.slabs = int(slab_off[-1])
        self.frames = int(lens.astype(np.int64).sum())
        dev = torch.device(store.device)
        self.device = dev
        self.rows_d = torch.from_numpy(rows).to(dev)
        self.lens_d = torch.from_numpy(lens).to(dev)
        self.slab_off_d = torch.from_numpy(slab_off).to(dev)
        self.labels_d = store.labels_d
        self.result_d = torch.zeros(_RESULT_WORDS, dtype=torch.int64, device=dev)
        self.result_h = torch.zeros(_RESULT_WORDS, dtype=torch.int64).pin_memory()
        self._ws = None
        self._cm = None
        self._win = {}
        self._noise = {}

    @classmethod
    def of(cls, x):
        if isinstance(x, cls):
            return x
        store = getattr(x, "store", x)
        plan = getattr(store, "_eval_plan", None)
        if plan is None:
            plan = cls(store)
            store._eval_plan = plan
        return plan

    def workspace(self, precision, with_teacher):
        need = int(_lib.lib().dad_eval_workspace_bytes(self.n, self.slabs, precision, int(with_teacher)))
        if self._ws is None or self._ws.numel() < need:
            self._ws = torch.empty(need, dtype=torch.uint8, device=self.device)
        return self._ws

    def cluster_buffers(self):
        """(workspace, result block on the device, pinned host copy) of dad_cluster_metrics over this
        split, allocated at the first call and reused."""
        if self._cm is None:
            self._cm = (_cluster_workspace(self.n, self.device),
                        torch.zeros(_lib.CM_SLOTS, dtype=torch.float64, device=self.device),
                        torch.zeros(_lib.CM_SLOTS, dtype=torch.float64).pin_memory())
        return self._cm

    def window_buffers(self, hop, span=1, mode="sliding"):
        """What dad_eval_windows needs about this split for one (hop, span, mode), built at the first call and
        reused: {'win_off' / 'piece_off' host int32 [n + 1] (windows_host), 'win_off_d' / 'piece_off_d' their
        device copies, 'windows', 'pieces', 'result_d' / 'result_h' the DAD_EW_* block and its pinned host copy,
        'ws' the workspace (grown on demand by enqueue_eval_windows)}."""
        key = (int(hop), int(span), str(mode))
        b = self._win.get(key)
        if b is None:
            win_off, piece_off = windows_host(self.store.sizes, hop, span, mode)
            b = {"win_off": win_off, "piece_off": piece_off,
                 "win_off_d": torch.from_numpy(win_off).to(self.device),
                 "piece_off_d": torch.from_numpy(piece_off).to(self.device),
                 "windows": int(win_off[-1]), "pieces": int(piece_off[-1]),
                 "result_d": torch.zeros(_lib.EW_SLOTS, dtype=torch.int64, device=self.device),
                 "result_h": torch.zeros(_lib.EW_SLOTS, dtype=torch.int64).pin_memory(), "ws": None}
            self._win[key] = b
        return b


def enqueue_eval_split(model, plan, use_teacher=False, use_entropy=True, precision="fp32", outputs=()):
    """dad_eval_split on the current stream, enqueue only (no copy, no synchronisation): the result
    block lands in plan.result_d.  Returns the {name: device tensor} of the requested outputs."""
    prec = _PRECISIONS[precision] if isinstance(precision, str) else int(precision)
    dev = plan.device
    if model.student_flat.device != dev:
        raise RuntimeError("model on %s, store on %s" % (model.student_flat.device, dev))
    out = {}
    for name in outputs:
        if name not in _OUTPUTS:
            raise ValueError("unknown output %r (one of %s)" % (name, ", ".join(_OUTPUTS)))
        if name.startswith("t_") and not use_teacher:
            raise ValueError("output %r needs use_teacher=True" % name)
        shape, dt = _OUTPUTS[name]
        out[name] = torch.empty((plan.n,) + shape, dtype=dt, device=dev)
    store = plan.store
    a = _lib.DadEvalArgs()
    a.store = store.feats.data_ptr()
    a.rows, a.lens, a.slab_off = plan.rows_d.data_ptr(), plan.lens_d.data_ptr(), plan.slab_off_d.data_ptr()
    a.labels = None if plan.labels_d is None else plan.labels_d.data_ptr()
    a.student = model.student_flat.data_ptr()
    a.teacher = model.teacher_flat.data_ptr() if use_teacher else None
    for name, t in out.items():
        setattr(a, name, t.data_ptr())
    a.counts = plan.result_d.data_ptr()
    a.moments = plan.result_d.data_ptr() + 8 * _lib.EV_COUNTS
    a.n, a.slabs = plan.n, plan.slabs
    a.store_dtype = STORE_DTYPES[store.feats.dtype]
    a.use_entropy = int(bool(use_entropy))
    a.precision = prec
    ws = plan.workspace(prec, use_teacher)
    stream = torch.cuda.current_stream(dev)
    _lib.check(_lib.lib().dad_eval_split(a, _lib.ptr(ws), stream.cuda_stream), "dad_eval_split")
    return out


def evaluate_store(model, plan_or_store, use_teacher=False, use_entropy=True, precision="fp32", outputs=()):
    """One dad_eval_split over the whole split and one device-to-host copy of its result block.
    Returns {'confusion_student' [4,4], 'confusion_teacher' [4,4], 'disagree', 'n', 'n_labelled',
    'n_skipped', 'n_nonfinite', 'moments' [4,3] (count, mean, population variance of the student's
    certainty score per true class)} as NumPy values, plus a device tensor per name in `outputs`
    ('emb', 'logits', 'probs', 'score', 'pred', 't_emb', 't_logits', 't_pred'; store sample order).
    precision 'fp32' (the reference's eval arithmetic) or 'fp16'.  Raises DadError when any
    utterance has a non-finite logit."""
    plan = EvalPlan.of(plan_or_store)
    out = enqueue_eval_split(model, plan, use_teacher, use_entropy, precision, outputs)
    return _read_eval_block(plan, out)


def _read_eval_block(plan, out):
    stream = torch.cuda.current_stream(plan.device)
    plan.result_h.copy_(plan.result_d, non_blocking=True)
    stream.synchronize()
    host = plan.result_h.numpy().copy()
    counts = host[:_lib.EV_COUNTS]
    res = {
        "confusion_student": counts[_lib.EV_CONF_STUDENT:_lib.EV_CONF_STUDENT + 16].reshape(4, 4).copy(),
        "confusion_teacher": counts[_lib.EV_CONF_TEACHER:_lib.EV_CONF_TEACHER + 16].reshape(4, 4).copy(),
        "disagree": int(counts[_lib.EV_DISAGREE]), "n": int(counts[_lib.EV_N]),
        "n_labelled": int(counts[_lib.EV_N_LABELLED]), "n_skipped": int(counts[_lib.EV_N_SKIPPED]),
        "n_nonfinite": int(counts[_lib.EV_N_NONFINITE]),
        "moments": host[_lib.EV_COUNTS:].view(np.float64).reshape(4, _lib.EV_MOMENTS).copy(),
        "block": host,
    }
    if res["n_nonfinite"] > 0:
        raise _lib.DadError("dad_eval_split: %d of %d utterance(s) have a non-finite logit (fp16: an operand beyond "
                            "+-65504; any precision: non-finite features)" % (res["n_nonfinite"], res["n"]))
    res.update(out)
    return res


def metrics_from_confusion(cm):
    """Every key validate() returns (but 'disagreement_rate'), from the confusion matrix alone
    (row = label, column = prediction), with scikit-learn's conventions: zero_division = 0;
    balanced accuracy averages recall over the classes present in y_true; the macro / weighted F1
    (no labels= argument) average over the classes present in y_true or y_pred; the *_per_class
    arrays cover range(num_classes)."""
    cm = np.asarray(cm)
    if cm.ndim != 2 or cm.shape[0] != cm.shape[1]:
        raise ValueError("confusion matrix must be square")
    cm = cm.astype(np.int64)
    total = int(cm.sum())
    if total == 0:
        raise ValueError("no labelled utterances")
    tp = np.diag(cm).astype(np.float64)
    sup = cm.sum(1)
    npred = cm.sum(0)
    div = lambda a, b: np.divide(a, b, out=np.zeros(len(a), np.float64), where=b > 0)
    prec = div(tp, npred.astype(np.float64))
    rec = div(tp, sup.astype(np.float64))
    f1 = div(2.0 * tp, (sup + npred).astype(np.float64))      # 2tp / (2tp + fp + fn)
    present = (sup > 0) | (npred > 0)
    return {
        "accuracy": float(tp.sum() / total) * 100,
        "weighted_accuracy": float(np.mean(rec[sup > 0])) * 100,
        "f1_weighted": float(np.sum(f1[present] * sup[present]) / sup[present].sum()) * 100,
        "f1_macro": float(np.mean(f1[present])) * 100,
        "precision_per_class": prec.tolist(), "recall_per_class": rec.tolist(),
        "f1_per_class": f1.tolist(), "support_per_class": sup.tolist(), "confusion_matrix": cm,
    }


def validate_store(model, store_or_loader, domain_name="unknown", num_classes=4, teacher_disagreement=False,
                   precision="fp32", cluster_metrics=False, ranking=False):
    """validate() over a FeatureStore split in one fused pass: the same dict, 'disagreement_rate'
    from the same pass (the teacher runs on the student's row reads).  With cluster_metrics the dict
    gains 'silhouette_score' and 'calinski_harabasz_score' of the same pass's student embeddings
    (dad_cluster_metrics behind dad_eval_split on the stream; (0.0, 0.0) and a warning for a label
    configuration the scores are not defined for).  With ranking it gains 'auroc_ovr_macro' (scikit-learn's
    roc_auc_score(y, probs, multi_class='ovr')), 'aurc' (the area under the risk-coverage curve of the certainty score)
    and 'confidence_stats' (I/inference.py:361-369) of the same pass (dad_rank_eval_columns and dad_rank_metrics behind
    dad_eval_split); without it nothing of that is launched or allocated."""
    if num_classes != 4:
        raise ValueError("the MI355X kernels are built for 4 classes")
    model.eval()
    if not cluster_metrics and not ranking:
        r = evaluate_store(model, store_or_loader, use_teacher=teacher_disagreement, precision=precision)
    else:
        plan = EvalPlan.of(store_or_loader)
        if plan.labels_d is None:
            raise ValueError("the split has no labels")
        names = (("emb",) if cluster_metrics else ()) + (("score", "probs", "pred") if ranking else ())
        out = enqueue_eval_split(model, plan, teacher_disagreement, True, precision, names)
        if cluster_metrics:
            ws, block_d, block_h = plan.cluster_buffers()
            _enqueue_cluster(out["emb"], plan.labels_d, block_d, None, ws)
            block_h.copy_(block_d, non_blocking=True)
        if ranking:
            rb = _ranking_buffers(plan, 0, 0)
            rb["thr"].fill_(float("nan"))
            _lib.check(_lib.require("dad_rank_eval_columns", "validate_store(ranking=True)")(
                _lib.ptr(out["score"]), _lib.ptr(out["probs"]), _lib.ptr(out["pred"]), _lib.ptr(plan.labels_d), plan.n,
                _lib.ptr(rb["key"]), _lib.ptr(rb["flags"]), torch.cuda.current_stream(plan.device).cuda_stream),
                "dad_rank_eval_columns")
            _enqueue_rank(rb["key"], rb["flags"], rb)
            rb["block_h"].copy_(rb["block_d"], non_blocking=True)
        r = _read_eval_block(plan, {})          # (synchronises the stream: every block is on the host)
        if cluster_metrics:
            cm = _cluster_result(block_h.numpy().copy())
    res = {}
    if teacher_disagreement:
        res["disagreement_rate"] = r["disagree"] / r["n"]
    res.update(metrics_from_confusion(r["confusion_student"]))
    if cluster_metrics:
        res["silhouette_score"] = cm["silhouette_score"]
        res["calinski_harabasz_score"] = cm["calinski_harabasz_score"]
    if ranking:
        rk = _certainty_result(_rank_columns(_rank_blocks(rb, rb["block_h"].numpy().copy())), (), 0)
        res["auroc_ovr_macro"] = rk["ovr"]["auroc_macro"]
        res["aurc"] = rk["selective"]["overall"]["aurc"]
        res["confidence_stats"] = rk["confidence_stats"]
    return res


def calibrate_anchors_store(model, clean, noisy, num_classes=4, anchor_std_k=1.5, use_entropy=True):
    """calibrate_anchors() over two FeatureStore splits, from the moments block of one
    dad_eval_split each (float64 mean / population std of the float32 scores, as np.mean / np.std)."""
    if num_classes != 4:
        raise ValueError("the MI355X kernels are built for 4 classes")
    model.eval()
    dev = model.student_flat.device
    mom = {name: evaluate_store(model, s, use_entropy=use_entropy)["moments"]
           for name, s in (("clean", clean), ("noisy", noisy))}
    mu_c = torch.tensor(mom["clean"][:, _lib.EV_M_MEAN].tolist(), device=dev)
    mu_n = torch.tensor(mom["noisy"][:, _lib.EV_M_MEAN].tolist(), device=dev)
    sd_c = torch.tensor(np.sqrt(mom["clean"][:, _lib.EV_M_VAR]).tolist(), device=dev)
    shift = mu_n / (mu_c + 1e-8)
    base = torch.clamp(mu_c - anchor_std_k * sd_c, min=0)
    model.train()
    return base * shift


def _enqueue_embeddings(model, plan, use_teacher, precision):
    """enqueue_eval_split for the split's embeddings alone (the teacher's with use_teacher): the device tensor."""
    name = "t_emb" if use_teacher else "emb"
    return enqueue_eval_split(model, plan, use_teacher=use_teacher, precision=precision, outputs=(name,))[name]


def embed_store(model, store_or_loader, use_teacher=False):
    """Eval-mode embeddings [n, 256] of every utterance of the split, in the store's sample order
    (the split-wide use of SSRLModel.get_embeddings, I/model.py:247-265), on the device."""
    model.eval()
    plan = EvalPlan.of(store_or_loader)
    emb = _enqueue_embeddings(model, plan, use_teacher, "fp32")
    _read_eval_block(plan, {})              # (raises on a non-finite logit, as evaluate_store does)
    return emb


def _check_emb(emb):
    if not torch.is_tensor(emb) or not emb.is_cuda or emb.dtype != torch.float32 or emb.dim() != 2 \
            or emb.shape[1] != 256:
        raise ValueError("emb must be a float32 device tensor [n, 256]")
    return emb.contiguous()


def _workspace(symbol, feature, n, lo, hi, device):
    need = int(_lib.require(symbol, feature)(int(n)))
    if need == 0:           # (the library's answer for n outside [lo, hi])
        takes = "t-SNE takes" if feature == "tsne" else "cluster metrics take"
        raise ValueError("%s %d <= n <= %d rows, got %d" % (takes, lo, hi, n))
    return torch.empty(need, dtype=torch.uint8, device=device)


# ------------------------------------------------------------------ class separation of a split
# calculate_cluster_metrics (I/iemocap_plot_tsne.py:390-398) copies the embeddings to the host and
# calls scikit-learn's silhouette_score and calinski_harabasz_score, O(n^2 * 256) each weight set.
# dad_cluster_metrics (csrc/cluster.hip) computes both on the device from the embeddings
# dad_eval_split leaves there; one copy of 16 doubles returns them.

def _cluster_workspace(n, device):
    return _workspace("dad_cluster_workspace_bytes", "cluster_metrics", n, 1, _lib.CM_MAX_N, device)


def _enqueue_cluster(emb, labels, block, sil, ws, chunks=0):
    """dad_cluster_metrics on the current stream, enqueue only.  chunks > 0 asks for that many column
    chunks per row tile instead of the planner's (dad_cluster_metrics_chunked: the tests' way to run
    the chunked summation at small n)."""
    n = emb.shape[0]
    stream = torch.cuda.current_stream(emb.device).cuda_stream
    if chunks:
        fn = _lib.require("dad_cluster_metrics_chunked", "cluster_metrics")
        rc = fn(_lib.ptr(emb), _lib.ptr(labels), n, _lib.ptr(block), _lib.ptr(sil), int(chunks), _lib.ptr(ws), stream)
    else:
        fn = _lib.require("dad_cluster_metrics", "cluster_metrics")
        rc = fn(_lib.ptr(emb), _lib.ptr(labels), n, _lib.ptr(block), _lib.ptr(sil), _lib.ptr(ws), stream)
    _lib.check(rc, "dad_cluster_metrics")


def _cluster_result(block):
    """The dict of cluster_metrics from the host copy of the DAD_CM_* block."""
    nbad = int(block[_lib.CM_NONFINITE])
    if nbad > 0:
        raise _lib.DadError("dad_cluster_metrics: %d of %d labelled row(s) have a non-finite embedding component"
                            % (nbad, int(block[_lib.CM_M])))
    valid = bool(block[_lib.CM_VALID])
    res = {
        "silhouette_score": float(block[_lib.CM_SILHOUETTE]),
        "calinski_harabasz_score": float(block[_lib.CM_CH]),
        "valid": valid, "n_labelled": int(block[_lib.CM_M]), "classes_present": int(block[_lib.CM_K]),
        "class_counts": [int(v) for v in block[_lib.CM_COUNTS:_lib.CM_COUNTS + 4]],
        "silhouette_per_class": [float(v) for v in block[_lib.CM_SIL_CLASS:_lib.CM_SIL_CLASS + 4]],
        "within": float(block[_lib.CM_W]), "between": float(block[_lib.CM_B]),
        "block": block,
    }
    if not valid:
        # scikit-learn raises here; calculate_cluster_metrics logs the warning and returns (0.0, 0.0)
        warnings.warn("cluster metrics need 2 <= classes present <= labelled rows - 1, got %d classes over %d rows: "
                      "both scores are 0.0" % (res["classes_present"], res["n_labelled"]), RuntimeWarning,
                      stacklevel=3)
    return res


def cluster_metrics(emb, labels, samples=False, _chunks=0):
    """calculate_cluster_metrics (I/iemocap_plot_tsne.py:390-398) on the device: scikit-learn's
    silhouette_score and calinski_harabasz_score of emb [n, 256] (float32, device) under labels [n]
    (int64; a host array is moved to the device), over the rows with a label in [0, 4).
    Returns {'silhouette_score', 'calinski_harabasz_score', 'valid', 'n_labelled', 'classes_present',
    'class_counts', 'silhouette_per_class', 'within', 'between'}; samples=True adds the device tensor
    'silhouette_samples' [n] (0 for an unlabelled row).  Where scikit-learn would raise (fewer than 2
    classes present, or as many classes as labelled rows) both scores are 0.0, 'valid' is False and a
    RuntimeWarning is issued.  Raises DadError when a labelled row has a non-finite component."""
    emb = _check_emb(emb)
    labels = torch.as_tensor(labels).to(device=emb.device, dtype=torch.int64).contiguous()
    if labels.shape != (emb.shape[0],):
        raise ValueError("labels must be [n]")
    n = emb.shape[0]
    ws = _cluster_workspace(n, emb.device)
    block = torch.empty(_lib.CM_SLOTS, dtype=torch.float64, device=emb.device)
    sil = torch.empty(n, dtype=torch.float32, device=emb.device) if samples else None
    _enqueue_cluster(emb, labels, block, sil, ws, _chunks)
    res = _cluster_result(block.cpu().numpy())
    if samples:
        res["silhouette_samples"] = sil
    return res


def enqueue_cluster_metrics_store(model, plan, use_teacher=False, precision="fp32", samples=False):
    """The enqueue part of cluster_metrics_store (no copy, no synchronisation; graph-capturable):
    dad_eval_split for the embeddings, dad_cluster_metrics behind it on the current stream against the
    plan's device labels.  The block lands in plan.cluster_buffers()[1].  Returns (emb, sil or None)."""
    if plan.labels_d is None:
        raise ValueError("the split has no labels")
    emb = _enqueue_embeddings(model, plan, use_teacher, precision)
    ws, block_d, _ = plan.cluster_buffers()
    sil = torch.empty(plan.n, dtype=torch.float32, device=plan.device) if samples else None
    _enqueue_cluster(emb, plan.labels_d, block_d, sil, ws)
    return emb, sil


def cluster_metrics_store(model, store_or_loader, use_teacher=False, precision="fp32", samples=False):
    """cluster_metrics of the split's eval-mode embeddings (the teacher's with use_teacher) without
    their leaving the device: one dad_eval_split, one dad_cluster_metrics, one copy of the block.
    The workspace is cached on the split's EvalPlan."""
    model.eval()
    plan = EvalPlan.of(store_or_loader)
    _, sil = enqueue_cluster_metrics_store(model, plan, use_teacher, precision, samples)
    _, block_d, block_h = plan.cluster_buffers()
    block_h.copy_(block_d, non_blocking=True)
    torch.cuda.current_stream(plan.device).synchronize()
    res = _cluster_result(block_h.numpy().copy())
    if samples:
        res["silhouette_samples"] = sil
    return res


def separation_from_metrics(initial, trained):
    """generate_analysis_report's `cluster_analysis` block (I/iemocap_plot_tsne.py:428-442) from the
    two (silhouette, CH) pairs or cluster_metrics dicts; every value a Python float."""
    pair = lambda r: ((r["silhouette_score"], r["calinski_harabasz_score"]) if isinstance(r, dict) else r)
    (si, ci), (st, ct) = pair(initial), pair(trained)
    si, ci, st, ct = float(si), float(ci), float(st), float(ct)
    return {
        "initial_weights": {"silhouette_score": si, "calinski_harabasz_score": ci},
        "trained_weights": {"silhouette_score": st, "calinski_harabasz_score": ct},
        "improvement": {"silhouette_improvement": st - si, "calinski_improvement": ct - ci,
                        "silhouette_percentage": (st - si) / abs(si) * 100 if si != 0 else 0.0},
    }


def separation_report(initial_model, trained_model, store_or_loader):
    """The reference's `cluster_analysis` block for one split under the initial and the trained
    weights (student embeddings, as iemocap_plot_tsne.py embeds with)."""
    return separation_from_metrics(cluster_metrics_store(initial_model, store_or_loader),
                                   cluster_metrics_store(trained_model, store_or_loader))


# ------------------------------------------------------------------ exact t-SNE of a split
# run_tsne (I/iemocap_plot_tsne.py:310-323) copies the embeddings to the host and runs scikit-learn's TSNE,
# once per weight set.  dad_tsne_* (csrc/tsne.hip) is scikit-learn's method='exact' in its three stages on the
# device: the joint distribution P, one evaluation of the error and its gradient, and the 1,000-iteration
# descent, which the host only enqueues.

def _tsne_workspace(n, device):
    return _workspace("dad_tsne_workspace_bytes", "tsne", n, 2, _lib.TS_MAX_N, device)


def _check_p(P):
    if not torch.is_tensor(P) or not P.is_cuda or P.dtype != torch.float32 or P.dim() != 2 \
            or P.shape[1] != _lib.ts_ld(P.shape[0]) or not P.is_contiguous():
        raise ValueError("P must be a contiguous float32 device tensor [n, n rounded up to %d] (tsne_affinities)"
                         % _lib.TS_TILE)
    return P


def _enqueue_tsne_affinities(emb, perplexity, P, beta, ws):
    fn = _lib.require("dad_tsne_affinities", "tsne")
    _lib.check(fn(_lib.ptr(emb), emb.shape[0], float(perplexity), _lib.ptr(P), _lib.ptr(beta), _lib.ptr(ws),
                  torch.cuda.current_stream(emb.device).cuda_stream), "dad_tsne_affinities")


def tsne_affinities(emb, perplexity=30.0, beta=False, _ws=None):
    """scikit-learn's _joint_probabilities of emb [n, 256] (float32, device) on the device: the dense symmetric
    joint distribution P as a float32 device tensor [n, n rounded up to 64] (P[:, :n] is the matrix; the padding
    columns are 0).  beta=True returns (P, the float64 precision the search found for each row).  Raises
    ValueError for n < 2, n > 16384 or a perplexity outside (0, n), before any launch, and DadError when a row
    has a non-finite component."""
    emb = _check_emb(emb)
    n = emb.shape[0]
    ws = _tsne_workspace(n, emb.device) if _ws is None else _ws
    if not 0.0 < float(perplexity) < n:
        raise ValueError("perplexity must be in (0, n = %d), got %r" % (n, perplexity))
    P = torch.empty(n, _lib.ts_ld(n), dtype=torch.float32, device=emb.device)
    b = torch.empty(n, dtype=torch.float64, device=emb.device) if beta else None
    _enqueue_tsne_affinities(emb, perplexity, P, b, ws)
    nbad = int(ws[4 * _lib.TS_WS_NONFINITE:4 * _lib.TS_WS_NONFINITE + 4].view(torch.int32).item())
    if nbad > 0:
        raise _lib.DadError("dad_tsne_affinities: %d of %d row(s) have a non-finite embedding component" % (nbad, n))
    return (P, b) if beta else P


def tsne_gradient(P, Y, exaggeration=1.0, _chunks=0, _ws=None):
    """scikit-learn's _kl_divergence (one degree of freedom) at Y [n, 2] (float32, device) against
    exaggeration * P (tsne_affinities' tensor): {'kl_divergence', 'z', 'grad_norm', 'grad' [n, 2] device
    tensor}.  _chunks > 0 asks for that many column chunks per row tile instead of the planner's."""
    P = _check_p(P)
    n = P.shape[0]
    if not torch.is_tensor(Y) or Y.device != P.device or Y.dtype != torch.float32 or tuple(Y.shape) != (n, 2):
        raise ValueError("Y must be a float32 tensor [n, 2] on P's device")
    Y = Y.contiguous()
    ws = _tsne_workspace(n, P.device) if _ws is None else _ws
    out = torch.empty(_lib.TS_SLOTS, dtype=torch.float64, device=P.device)
    grad = torch.empty(n, 2, dtype=torch.float32, device=P.device)
    fn = _lib.require("dad_tsne_gradient_chunked", "tsne")
    _lib.check(fn(_lib.ptr(P), n, _lib.ptr(Y), float(exaggeration), _lib.ptr(out), _lib.ptr(grad), int(_chunks),
                  _lib.ptr(ws), torch.cuda.current_stream(P.device).cuda_stream), "dad_tsne_gradient")
    o = out.cpu().numpy()
    return {"kl_divergence": float(o[_lib.TS_KL]), "z": float(o[_lib.TS_Z]), "grad_norm": float(o[_lib.TS_GRAD_NORM]),
            "grad": grad}


def tsne_pca_init(emb):
    """TSNE's init='pca' with the exact components: the top two principal components of the centred rows, from an
    eigendecomposition of the 256 x 256 covariance in float64 (scikit-learn draws them from its randomized solver,
    which agrees to 3e-10 at a scale of 1.8e-4), each signed so that its largest-magnitude loading is positive
    (svd_flip(u_based_decision=False)), cast to float32 and scaled so that column 0 has standard deviation 1e-4."""
    x = emb.to(torch.float64)
    xc = x - x.mean(0, keepdim=True)
    _, v = torch.linalg.eigh(xc.T @ xc)
    v = v[:, [-1, -2]]
    big = v.gather(0, v.abs().argmax(0, keepdim=True))
    v = v * torch.sign(big)
    y = (xc @ v).to(torch.float32)
    return (y / y[:, 0].std(unbiased=False) * 1e-4).contiguous()


def tsne_run_buffers(n, max_iter, device):
    """(history [max_iter // 50 + 1, 2], out [8]) float64 device tensors of dad_tsne_run."""
    return (torch.zeros(int(max_iter) // 50 + 1, 2, dtype=torch.float64, device=device),
            torch.zeros(_lib.TS_SLOTS, dtype=torch.float64, device=device))


def enqueue_tsne_run(P, Y, history, out, ws, max_iter=1000, learning_rate="auto", early_exaggeration=12.0,
                     min_grad_norm=1e-7, n_iter_without_progress=300):
    """dad_tsne_run on the current stream, enqueue only (no copy, no synchronisation; graph-capturable): Y [n, 2]
    holds the initial embedding and receives the result."""
    n = P.shape[0]
    a = _lib.DadTsneArgs()
    a.max_iter, a.n_iter_without_progress = int(max_iter), int(n_iter_without_progress)
    a.early_exaggeration = float(early_exaggeration)
    a.learning_rate = (max(n / float(early_exaggeration) / 4.0, 50.0) if isinstance(learning_rate, str)
                       else float(learning_rate))
    a.min_grad_norm = float(min_grad_norm)
    fn = _lib.require("dad_tsne_run", "tsne")
    _lib.check(fn(_lib.ptr(P), n, _lib.ptr(Y), a, _lib.ptr(history), _lib.ptr(out), _lib.ptr(ws),
                  torch.cuda.current_stream(P.device).cuda_stream), "dad_tsne_run")


def tsne(emb, perplexity=30.0, max_iter=1000, init="pca", learning_rate="auto", early_exaggeration=12.0,
         min_grad_norm=1e-7, n_iter_without_progress=300, history=False, _P=None):
    """scikit-learn's TSNE(n_components=2, method='exact') of emb [n, 256] (float32, device) on the device, with
    scikit-learn's parameters and defaults.  init: 'pca' (tsne_pca_init) or an [n, 2] tensor, used as given and
    never modified ('random' is not offered).  learning_rate 'auto' = max(n / early_exaggeration / 4, 50).
    Returns {'embedding' [n, 2] float32 device tensor, 'kl_divergence', 'n_iter'}; history=True adds 'history', the
    (error, gradient norm) of every 50th iteration's check as a float64 array.  max_iter below 250 shortens the
    exploration phase to max_iter iterations (scikit-learn refuses such a value)."""
    emb = _check_emb(emb)
    n = emb.shape[0]
    if isinstance(init, str):
        if init != "pca":
            raise ValueError("init must be 'pca' or an [n, 2] tensor, got %r" % (init,))
    elif not torch.is_tensor(init) or tuple(init.shape) != (n, 2):
        raise ValueError("init must be 'pca' or an [n, 2] tensor")
    if isinstance(learning_rate, str) and learning_rate != "auto":
        raise ValueError("learning_rate must be 'auto' or a number")
    if int(max_iter) < 1:
        raise ValueError("max_iter must be at least 1")
    ws = _tsne_workspace(n, emb.device)
    P = tsne_affinities(emb, perplexity, _ws=ws) if _P is None else _check_p(_P)
    Y = (tsne_pca_init(emb) if isinstance(init, str)
         else init.detach().to(device=emb.device, dtype=torch.float32, copy=True).contiguous())
    hist, out = tsne_run_buffers(n, max_iter, emb.device)
    enqueue_tsne_run(P, Y, hist, out, ws, max_iter, learning_rate, early_exaggeration, min_grad_norm,
                     n_iter_without_progress)
    o = out.cpu().numpy()
    res = {"embedding": Y, "kl_divergence": float(o[_lib.TS_KL]), "n_iter": int(o[_lib.TS_N_ITER])}
    if history:
        res["history"] = hist[:int(o[_lib.TS_N_CHECKS])].cpu().numpy()
    return res


def _tsne_store(model, plan, use_teacher=False, precision="fp32", **tsne_args):
    """(the split's eval-mode embeddings on the device, tsne of them): what tsne_store runs."""
    model.eval()
    emb = _enqueue_embeddings(model, plan, use_teacher, precision)
    return emb, tsne(emb, **tsne_args)


def tsne_store(model, store_or_loader, use_teacher=False, precision="fp32", **tsne_args):
    """tsne of the split's eval-mode embeddings (the teacher's with use_teacher), which dad_eval_split leaves on the
    device: the embeddings never reach the host."""
    return _tsne_store(model, EvalPlan.of(store_or_loader), use_teacher, precision, **tsne_args)[1]


def tsne_report(initial_model, trained_model, store_or_loader, trustworthiness_k=None, **tsne_args):
    """The inputs of the reference's plot_tsne_comparison (I/iemocap_plot_tsne.py:524-525 and the plot call) for
    one split: {'initial' [n, 2], 'trained' [n, 2] NumPy float32 embeddings under the two weight sets (student
    embeddings, as iemocap_plot_tsne.py embeds with), 'labels' [n], 'class_counts' [4], 'kl_divergence' (initial,
    trained), 'n_iter' (initial, trained)}.  With trustworthiness_k the report gains 'trustworthiness' (initial,
    trained): scikit-learn's trustworthiness of each map against the embeddings it was made from, n_neighbors =
    trustworthiness_k (trustworthiness(); unlike the error, a number two runs can be compared by)."""
    plan = EvalPlan.of(store_or_loader)
    if plan.labels_d is None:
        raise ValueError("the split has no labels")
    sides = []
    for model in (initial_model, trained_model):
        emb, r = _tsne_store(model, plan, **tsne_args)
        if trustworthiness_k is not None:
            r["trustworthiness"] = trustworthiness(emb, r["embedding"], k=trustworthiness_k)["trustworthiness"]
        sides.append(r)
    a, b = sides
    labels = plan.labels_d.cpu().numpy()
    rep = {"initial": a["embedding"].cpu().numpy(), "trained": b["embedding"].cpu().numpy(), "labels": labels,
           "class_counts": [int((labels == c).sum()) for c in range(4)],
           "kl_divergence": (a["kl_divergence"], b["kl_divergence"]), "n_iter": (a["n_iter"], b["n_iter"])}
    if trustworthiness_k is not None:
        rep["trustworthiness"] = (a["trustworthiness"], b["trustworthiness"])
    return rep


# ------------------------------------------------------------------ the clean-noisy domain gap of two splits
# ECDALoss (I/utils.py:510-652) is the quantity the method shrinks, computed by the train step on one batch of 64;
# _gaussian_kernel's [m, m, 256] temporaries rule out a whole split.  dad_domain_gap (csrc/domain_gap.hip) computes
# it for the embeddings of two splits on the device; one copy of 64 doubles returns every term.

_DG_GLOBAL = (("gate", _lib.DG_G_GATE), ("bandwidth", _lib.DG_G_BANDWIDTH), ("term_ss", _lib.DG_G_SS),
              ("term_tt", _lib.DG_G_TT), ("term_st", _lib.DG_G_ST), ("mmd", _lib.DG_G_MMD))
_DG_CLASS = (("gate", _lib.DG_C_GATE), ("bandwidth", _lib.DG_C_BANDWIDTH), ("term_ss", _lib.DG_C_SS),
             ("term_tt", _lib.DG_C_TT), ("term_st", _lib.DG_C_ST), ("mmd", _lib.DG_C_MMD),
             ("n_clean", _lib.DG_C_N_SRC), ("n_noisy", _lib.DG_C_N_TGT), ("weight_noisy", _lib.DG_C_W_TGT),
             ("compactness", _lib.DG_C_COMPACTNESS), ("centroid_shift", _lib.DG_C_SHIFT),
             ("attention", _lib.DG_C_ATTENTION))
_DG_COUNTS = ("gate", "n_clean", "n_noisy")


def _domain_gap_workspace(n, device):
    need = int(_lib.require("dad_domain_gap_workspace_bytes", "domain_gap")(int(n)))
    if need == 0:           # (the library's answer for n outside [1, DG_MAX_N])
        raise ValueError("the domain gap takes 1 <= rows of both domains together <= %d, got %d" % (_lib.DG_MAX_N, n))
    return torch.empty(need, dtype=torch.uint8, device=device)


def _domain_gap_args(class_weights, cfg):
    """dad_domain_gap_args from class_weights [4] (None: ones) and a ConfigView (None: the IEMOCAP defaults)."""
    from .config import ConfigView
    view = ConfigView(flavor="iemocap") if cfg is None else cfg
    a = _lib.DadDomainGapArgs()
    cw = [1.0] * 4 if class_weights is None else [float(v) for v in torch.as_tensor(class_weights).reshape(-1).tolist()]
    if len(cw) != 4:
        raise ValueError("class_weights must be [4]")
    a.class_weights[:] = cw
    a.lam = float(view.ECDA_CLASS_ATTENTION_LAMBDA)
    a.gamma = float(view.ECDA_COMPACTNESS_WEIGHT_GAMMA)
    a.delta = float(view.ECDA_REPULSION_WEIGHT_DELTA)
    return a


def _enqueue_domain_gap(emb, labels, domain, weights, args, block, ws, chunks=0):
    """dad_domain_gap on the current stream, enqueue only.  chunks > 0 asks for that many column chunks per row
    tile instead of the planner's (dad_domain_gap_chunked)."""
    n = emb.shape[0]
    stream = torch.cuda.current_stream(emb.device).cuda_stream
    if chunks:
        fn = _lib.require("dad_domain_gap_chunked", "domain_gap")
        rc = fn(_lib.ptr(emb), _lib.ptr(labels), _lib.ptr(domain), _lib.ptr(weights), n, args, _lib.ptr(block),
                int(chunks), _lib.ptr(ws), stream)
    else:
        fn = _lib.require("dad_domain_gap", "domain_gap")
        rc = fn(_lib.ptr(emb), _lib.ptr(labels), _lib.ptr(domain), _lib.ptr(weights), n, args, _lib.ptr(block),
                _lib.ptr(ws), stream)
    _lib.check(rc, "dad_domain_gap")


def _domain_gap_result(block):
    """The dict of domain_gap from the host copy of the DAD_DG_* block."""
    nbad = int(block[_lib.DG_NONFINITE])
    n_clean, n_noisy = int(block[_lib.DG_N_SRC]), int(block[_lib.DG_N_TGT])
    if nbad > 0:
        raise _lib.DadError("dad_domain_gap: %d of %d participating row(s) have a non-finite embedding component"
                            % (nbad, n_clean + n_noisy))
    num = lambda k, v: (bool(v) if k == "gate" else int(v)) if k in _DG_COUNTS else float(v)
    res = {
        "valid": bool(block[_lib.DG_VALID]), "n_clean": n_clean, "n_noisy": n_noisy,
        "global": {k: num(k, block[s]) for k, s in _DG_GLOBAL},
        "per_class": {k: [num(k, v) for v in block[s:s + 4]] for k, s in _DG_CLASS},
        "repulsion": float(block[_lib.DG_REPULSION]), "ecda_loss": float(block[_lib.DG_ECDA_LOSS]),
        "mmd_class_mean": float(block[_lib.DG_MMD_CLASS_MEAN]), "nonfinite": nbad, "block": block,
    }
    if not res["valid"]:
        warnings.warn("the domain gap needs 2 clean and 2 noisy rows, in one class or overall; got %d clean and %d "
                      "noisy participating rows and no class with 2 of each: every term is 0.0" % (n_clean, n_noisy),
                      RuntimeWarning, stacklevel=3)
    return res


def domain_gap(emb_clean, labels_clean, emb_noisy, labels_noisy, weights_noisy=None, class_weights=None, cfg=None,
               _chunks=0):
    """ECDALoss (I/utils.py:510-652) over two whole sets of embeddings on the device: emb_clean [n_c, 256] and
    emb_noisy [n_n, 256] (float32, device) under labels_clean / labels_noisy (int64; a row with a label outside
    [0, 4) takes no part, which is how to apply a DACP mask), weights_noisy [n_n] the noisy rows' sample weights
    (None: ones; the clean rows' are ones, as in the reference), class_weights [4] DACP's class weights (None:
    ones), cfg a ConfigView for ECDA_CLASS_ATTENTION_LAMBDA / ECDA_COMPACTNESS_WEIGHT_GAMMA /
    ECDA_REPULSION_WEIGHT_DELTA (None: the IEMOCAP values).
    Returns {'valid' (any gate open), 'n_clean', 'n_noisy' (participating rows), 'global': {'gate', 'bandwidth',
    'term_ss', 'term_tt', 'term_st', 'mmd'} (every participating row, unit weights), 'per_class': the same keys plus
    'n_clean', 'n_noisy', 'weight_noisy', 'compactness', 'centroid_shift', 'attention', each a list of 4,
    'repulsion', 'ecda_loss' (ECDALoss.forward), 'mmd_class_mean' (over the open gates), 'nonfinite', 'block'}.
    A class's gate is open with at least 2 clean and 2 noisy rows; a closed gate's terms are 0.0.  With no gate open
    'valid' is False and a RuntimeWarning is issued.  Raises DadError when a participating row has a non-finite
    component, ValueError for mismatched lengths or more than 65,536 rows, before any launch."""
    emb_clean, emb_noisy = _check_emb(emb_clean), _check_emb(emb_noisy)
    dev = emb_clean.device
    if emb_noisy.device != dev:
        raise ValueError("emb_clean on %s, emb_noisy on %s" % (dev, emb_noisy.device))
    nc, nn = emb_clean.shape[0], emb_noisy.shape[0]
    lc = torch.as_tensor(labels_clean).to(device=dev, dtype=torch.int64)
    ln = torch.as_tensor(labels_noisy).to(device=dev, dtype=torch.int64)
    if lc.shape != (nc,) or ln.shape != (nn,):
        raise ValueError("labels_clean must be [%d] and labels_noisy [%d]" % (nc, nn))
    weights = None
    if weights_noisy is not None:
        wn = torch.as_tensor(weights_noisy).to(device=dev, dtype=torch.float32)
        if wn.shape != (nn,):
            raise ValueError("weights_noisy must be [%d]" % nn)
    n = nc + nn
    if n < 1 or n > _lib.DG_MAX_N:
        raise ValueError("the domain gap takes 1 <= rows of both domains together <= %d, got %d" % (_lib.DG_MAX_N, n))
    args = _domain_gap_args(class_weights, cfg)
    ws = _domain_gap_workspace(n, dev)
    emb = torch.cat([emb_clean, emb_noisy])
    labels = torch.cat([lc, ln])
    domain = torch.zeros(n, dtype=torch.uint8, device=dev)
    domain[nc:] = 1
    if weights_noisy is not None:
        weights = torch.cat([torch.ones(nc, dtype=torch.float32, device=dev), wn])
    block = torch.empty(_lib.DG_SLOTS, dtype=torch.float64, device=dev)
    _enqueue_domain_gap(emb, labels, domain, weights, args, block, ws, _chunks)
    return _domain_gap_result(block.cpu().numpy())


def _domain_gap_buffers(plan, n_clean):
    """The buffers of domain_gap_store on the noisy split's plan for a clean split of n_clean rows, allocated at
    the first call and reused: workspace, the concatenated embeddings / labels / domain / weights, the teacher's
    scores, the result block on the device and its pinned host copy."""
    cache = plan.__dict__.setdefault("_dg", {})
    b = cache.get(n_clean)
    if b is None:
        n, dev = n_clean + plan.n, plan.device
        if n > _lib.DG_MAX_N:
            raise ValueError("the domain gap takes 1 <= rows of both domains together <= %d, got %d"
                             % (_lib.DG_MAX_N, n))
        b = {"ws": _domain_gap_workspace(n, dev),
             "emb": torch.empty(n, 256, dtype=torch.float32, device=dev),
             "labels": torch.empty(n, dtype=torch.int64, device=dev),
             "domain": torch.cat([torch.zeros(n_clean, dtype=torch.uint8, device=dev),
                                  torch.ones(plan.n, dtype=torch.uint8, device=dev)]),
             "weights": torch.ones(n, dtype=torch.float32, device=dev),
             "score": torch.empty(plan.n, dtype=torch.float32, device=dev),
             "block_d": torch.zeros(_lib.DG_SLOTS, dtype=torch.float64, device=dev),
             "block_h": torch.zeros(_lib.DG_SLOTS, dtype=torch.float64).pin_memory()}
        cache[n_clean] = b
    return b


def enqueue_domain_gap_store(model, clean_plan, noisy_plan, assign="labels", thresholds=None, class_weights=None,
                             precision="fp32", cfg=None):
    """The enqueue part of domain_gap_store (no copy to the host, no synchronisation; graph-capturable): one
    dad_eval_split per split for the student embeddings (the noisy one with the teacher for assign='teacher'),
    dad_certainty_scores for the teacher's scores, dad_domain_gap behind them on the current stream.  Returns the
    buffers (_domain_gap_buffers): the block lands in ['block_d']."""
    if assign not in ("labels", "teacher"):
        raise ValueError("assign must be 'labels' or 'teacher', got %r" % (assign,))
    if clean_plan.labels_d is None or (assign == "labels" and noisy_plan.labels_d is None):
        raise ValueError("the split has no labels")
    if clean_plan.device != noisy_plan.device:
        raise ValueError("clean split on %s, noisy split on %s" % (clean_plan.device, noisy_plan.device))
    nc = clean_plan.n
    b = _domain_gap_buffers(noisy_plan, nc)
    args = _domain_gap_args(class_weights, cfg)
    b["emb"][:nc].copy_(_enqueue_embeddings(model, clean_plan, False, precision))
    b["labels"][:nc].copy_(clean_plan.labels_d)
    if assign == "labels":
        b["emb"][nc:].copy_(_enqueue_embeddings(model, noisy_plan, False, precision))
        b["labels"][nc:].copy_(noisy_plan.labels_d)
        b["weights"][nc:].fill_(1.0)
    else:
        from .config import ConfigView
        view = ConfigView(flavor="iemocap") if cfg is None else cfg
        out = enqueue_eval_split(model, noisy_plan, use_teacher=True, precision=precision,
                                 outputs=("emb", "t_pred", "t_logits"))
        b["emb"][nc:].copy_(out["emb"])
        probs = torch.softmax(out["t_logits"], dim=1).contiguous()
        stream = torch.cuda.current_stream(noisy_plan.device).cuda_stream
        _lib.check(_lib.lib().dad_certainty_scores(probs.data_ptr(), noisy_plan.n,
                                                   int(view.effective_switches()[2]), b["score"].data_ptr(),
                                                   None, stream), "dad_certainty_scores")
        b["weights"][nc:].copy_(b["score"])
        pred = out["t_pred"]
        if thresholds is not None:
            thr = torch.as_tensor(thresholds).to(device=noisy_plan.device, dtype=torch.float32)
            if thr.shape != (4,):
                raise ValueError("thresholds must be [4]")
            # calculate_mask (I/utils.py:449-507): confident where score > thresholds[pred]; the rest take no part
            pred = torch.where(b["score"] > thr[pred], pred, torch.full_like(pred, -1))
        b["labels"][nc:].copy_(pred)
    _enqueue_domain_gap(b["emb"], b["labels"], b["domain"], b["weights"], args, b["block_d"], b["ws"])
    return b


def domain_gap_store(model, clean_split, noisy_split, assign="labels", thresholds=None, class_weights=None,
                     precision="fp32", cfg=None):
    """domain_gap of the student's eval-mode embeddings of two FeatureStore splits without their leaving the
    device: one dad_eval_split per split, one dad_domain_gap, one copy of the block.  assign='labels': the noisy
    rows under their true labels with unit weights (the plain domain gap).  assign='teacher': what the loss would
    see split-wide -- each noisy row under the teacher's prediction, weighted by the teacher's certainty score
    (dad_certainty_scores of its softmax); with thresholds [4], rows with score <= thresholds[prediction] take no
    part (calculate_mask's comparison, I/utils.py:449-507).  Every buffer is cached on the noisy split's EvalPlan."""
    model.eval()
    cp, np_ = EvalPlan.of(clean_split), EvalPlan.of(noisy_split)
    b = enqueue_domain_gap_store(model, cp, np_, assign, thresholds, class_weights, precision, cfg)
    b["block_h"].copy_(b["block_d"], non_blocking=True)
    torch.cuda.current_stream(np_.device).synchronize()
    return _domain_gap_result(b["block_h"].numpy().copy())


def alignment_from_gaps(initial, trained):
    """The `initial_weights` / `trained_weights` / `improvement` block (the shape of separation_from_metrics) from
    two domain_gap dicts: the global mmd, the mean per-class mmd and the ECDA loss; a gap that shrank has a
    negative change.  Every value a Python float."""
    pick = lambda r: {"mmd_global": float(r["global"]["mmd"]), "mmd_class_mean": float(r["mmd_class_mean"]),
                      "ecda_loss": float(r["ecda_loss"])}
    a, b = pick(initial), pick(trained)
    return {"initial_weights": a, "trained_weights": b,
            "improvement": {"mmd_global_change": b["mmd_global"] - a["mmd_global"],
                            "mmd_class_mean_change": b["mmd_class_mean"] - a["mmd_class_mean"],
                            "ecda_loss_change": b["ecda_loss"] - a["ecda_loss"],
                            "mmd_global_percentage": ((b["mmd_global"] - a["mmd_global"]) / abs(a["mmd_global"]) * 100
                                                      if a["mmd_global"] != 0 else 0.0)}}


def alignment_report(initial_model, trained_model, clean_split, noisy_split, **gap_args):
    """alignment_from_gaps of domain_gap_store under the initial and the trained weights."""
    return alignment_from_gaps(domain_gap_store(initial_model, clean_split, noisy_split, **gap_args),
                               domain_gap_store(trained_model, clean_split, noisy_split, **gap_args))


# ------------------------------------------------------------------ exact k nearest neighbours of a split
# The neighbour structure of the embeddings (dad_knn, csrc/knn.hip: exact top-k selection inside the Gram walk of the
# other pairwise evaluators) and the three scores on it: the leave-one-out k-NN vote (a non-parametric reading of class
# separation beside silhouette and CH), cross-domain retrieval (the per-utterance counterpart of domain_gap) and
# scikit-learn's trustworthiness of a t-SNE map.  Not in the reference; the yardstick is scikit-learn 1.7.2.

_KNN_MODES = {"all": _lib.KNN_ALL, "same": _lib.KNN_SAME, "other": _lib.KNN_OTHER}
_KV_RESULT = _lib.KV_SLOTS + 1          # the vote's block, then dad_knn's non-finite count


def _knn_workspace(n, k, device):
    need = int(_lib.require("dad_knn_workspace_bytes", "knn")(int(n), int(k)))
    if need == 0:           # (the library's answer for n or k outside its limits)
        raise ValueError("knn takes 1 <= n <= %d rows and 1 <= k <= %d, got n = %d, k = %d"
                         % (_lib.KNN_MAX_N, _lib.KNN_MAX_K, n, k))
    return torch.empty(need, dtype=torch.uint8, device=device)


def _enqueue_knn(emb, group, k, mode, idx, d2, ws, chunks=0):
    """dad_knn on the current stream, enqueue only.  chunks > 0 asks for that many column chunks per row tile
    instead of the planner's (dad_knn_chunked)."""
    fn = _lib.require("dad_knn_chunked", "knn")
    _lib.check(fn(_lib.ptr(emb), _lib.ptr(group), emb.shape[0], int(k), int(mode), _lib.ptr(idx), _lib.ptr(d2),
                  int(chunks), _lib.ptr(ws), torch.cuda.current_stream(emb.device).cuda_stream), "dad_knn")


def _enqueue_knn_vote(idx, labels, group, pred, result, ws):
    """dad_knn_vote on the current stream, enqueue only; result [_KV_RESULT] int64 receives the vote's block and,
    behind it, the non-finite count dad_knn left in ws."""
    fn = _lib.require("dad_knn_vote", "knn")
    _lib.check(fn(_lib.ptr(idx), _lib.ptr(labels), _lib.ptr(group), idx.shape[0], idx.shape[1], _lib.ptr(pred),
                  _lib.ptr(result), torch.cuda.current_stream(idx.device).cuda_stream), "dad_knn_vote")
    w = 4 * _lib.KNN_WS_NONFINITE
    result[_lib.KV_SLOTS:].copy_(ws[w:w + 4].view(torch.int32))


def _knn_group(labels, domain=None):
    """The int32 group of dad_knn from labels [n] (a label outside [0, 4) takes no part) and an optional domain."""
    ok = (labels >= 0) & (labels < 4)
    g = torch.zeros_like(labels, dtype=torch.int32) if domain is None else (domain != 0).to(torch.int32)
    return torch.where(ok, g, torch.full_like(g, -1)).contiguous()


def knn(emb, k=5, group=None, mode="all", _chunks=0):
    """The k nearest rows of every row of emb [n, 256] (float32, device), exactly: device tensors (idx [n, k] int32,
    d2 [n, k] float32), ascending in (squared distance, index), the distances those of cluster_metrics, squared.
    group [n] (int; None: one group): a row with a negative group is neither a query nor a candidate.  mode 'all':
    every other participating row is a candidate; 'same': those of the row's own group; 'other': those of the other
    groups (group = the domain: one call answers noisy -> clean and clean -> noisy).  Entries without a candidate
    are -1 / inf.  Every call and every chunk count gives the same bits.  Raises ValueError for n or k outside
    [1, 65536] / [1, 32], before any launch, and DadError when a participating row has a non-finite component."""
    emb = _check_emb(emb)
    n = emb.shape[0]
    if mode not in _KNN_MODES:
        raise ValueError("mode must be one of %s, got %r" % (", ".join(_KNN_MODES), mode))
    if group is not None:
        group = torch.as_tensor(group).to(device=emb.device, dtype=torch.int32).contiguous()
        if group.shape != (n,):
            raise ValueError("group must be [n]")
    ws = _knn_workspace(n, k, emb.device)
    idx = torch.empty(n, int(k), dtype=torch.int32, device=emb.device)
    d2 = torch.empty(n, int(k), dtype=torch.float32, device=emb.device)
    _enqueue_knn(emb, group, k, _KNN_MODES[mode], idx, d2, ws, _chunks)
    w = 4 * _lib.KNN_WS_NONFINITE
    nbad = int(ws[w:w + 4].view(torch.int32).item())
    if nbad > 0:
        raise _lib.DadError("dad_knn: %d participating row(s) of %d have a non-finite embedding component" % (nbad, n))
    return idx, d2


def _knn_result(result, pred, with_domain):
    """knn_accuracy's dict(s) from the host copy of the result words."""
    nbad = int(result[_lib.KV_SLOTS])
    if nbad > 0:
        raise _lib.DadError("dad_knn: %d participating row(s) have a non-finite embedding component" % nbad)
    out = []
    for g in (0, 1):
        cm = result[_lib.KV_CONFUSION + 16 * g:_lib.KV_CONFUSION + 16 * (g + 1)].reshape(4, 4).copy()
        nq, nv = int(result[_lib.KV_QUERIES + g]), int(result[_lib.KV_NO_VOTE + g])
        if cm.sum() == 0:
            out.append(None)
            continue
        r = metrics_from_confusion(cm)
        r.update({"n_queries": nq, "n_no_vote": nv, "pred": pred, "block": result})
        out.append(r)
    if with_domain:
        return {0: out[0], 1: out[1]}
    if out[0] is None:
        raise ValueError("no row has a voting neighbour")
    return out[0]


def knn_accuracy(emb, labels, k=5, domain=None, mode="all"):
    """The leave-one-out k-NN vote on emb [n, 256] (float32, device) under labels [n]: each row with a label in
    [0, 4) is classified by the uniform vote of its k nearest candidates (knn; rows with another label take no
    part), the smallest class winning a tie (KNeighborsClassifier's rule).  Returns metrics_from_confusion of the
    vote plus 'pred' [n] (int64 device tensor, -1 for a row that takes no part or has no neighbour), 'n_queries'
    and 'n_no_vote' (queries without a candidate: in no cell of the confusion matrix).  With domain [n] (0 / non-zero)
    the rows' group is their domain, mode applies to it ('other': retrieval across the domains) and the result is
    {0: the dict of the queries of domain 0, 1: of the others} (None for a domain without a voting query)."""
    emb = _check_emb(emb)
    n = emb.shape[0]
    if mode not in _KNN_MODES:
        raise ValueError("mode must be one of %s, got %r" % (", ".join(_KNN_MODES), mode))
    labels = torch.as_tensor(labels).to(device=emb.device, dtype=torch.int64).contiguous()
    if labels.shape != (n,):
        raise ValueError("labels must be [n]")
    if domain is not None:
        domain = torch.as_tensor(domain).to(device=emb.device)
        if domain.shape != (n,):
            raise ValueError("domain must be [n]")
    group = _knn_group(labels, domain)
    ws = _knn_workspace(n, k, emb.device)
    idx = torch.empty(n, int(k), dtype=torch.int32, device=emb.device)
    d2 = torch.empty(n, int(k), dtype=torch.float32, device=emb.device)
    pred = torch.empty(n, dtype=torch.int64, device=emb.device)
    result = torch.empty(_KV_RESULT, dtype=torch.int64, device=emb.device)
    _enqueue_knn(emb, group, k, _KNN_MODES[mode], idx, d2, ws)
    _enqueue_knn_vote(idx, labels, group, pred, result, ws)
    return _knn_result(result.cpu().numpy(), pred, domain is not None)


def _knn_buffers(plan, n, k):
    """The buffers of knn_store / cross_domain_knn_store on a split's plan for n rows in all, allocated at the first
    call and reused."""
    cache = plan.__dict__.setdefault("_knn", {})
    b = cache.get((n, int(k)))
    if b is None:
        dev = plan.device
        b = {"ws": _knn_workspace(n, k, dev),
             "idx": torch.empty(n, int(k), dtype=torch.int32, device=dev),
             "d2": torch.empty(n, int(k), dtype=torch.float32, device=dev),
             "pred": torch.empty(n, dtype=torch.int64, device=dev),
             "result_d": torch.zeros(_KV_RESULT, dtype=torch.int64, device=dev),
             "result_h": torch.zeros(_KV_RESULT, dtype=torch.int64).pin_memory()}
        cache[(n, int(k))] = b
    return b


def _read_knn(b, device, with_domain):
    b["result_h"].copy_(b["result_d"], non_blocking=True)
    torch.cuda.current_stream(device).synchronize()
    return _knn_result(b["result_h"].numpy().copy(), b["pred"].clone(), with_domain)


def enqueue_knn_store(model, plan, k=5, use_teacher=False, precision="fp32"):
    """The enqueue part of knn_store (no copy to the host, no synchronisation; graph-capturable): dad_eval_split for
    the embeddings, dad_knn and dad_knn_vote behind it.  Returns the buffers: the result lands in ['result_d']."""
    if plan.labels_d is None:
        raise ValueError("the split has no labels")
    b = _knn_buffers(plan, plan.n, k)
    emb = _enqueue_embeddings(model, plan, use_teacher, precision)
    group = _knn_group(plan.labels_d)
    _enqueue_knn(emb, group, k, _lib.KNN_ALL, b["idx"], b["d2"], b["ws"])
    _enqueue_knn_vote(b["idx"], plan.labels_d, group, b["pred"], b["result_d"], b["ws"])
    return b


def knn_store(model, store_or_loader, k=5, use_teacher=False, precision="fp32"):
    """knn_accuracy of the split's eval-mode embeddings (the teacher's with use_teacher) without their leaving the
    device: one dad_eval_split, one dad_knn, one dad_knn_vote, one copy of the result words."""
    model.eval()
    plan = EvalPlan.of(store_or_loader)
    return _read_knn(enqueue_knn_store(model, plan, k, use_teacher, precision), plan.device, False)


def enqueue_cross_domain_knn_store(model, clean_plan, noisy_plan, k=5, precision="fp32"):
    """The enqueue part of cross_domain_knn_store (no copy to the host, no synchronisation): one dad_eval_split per
    split into one concatenated buffer (the clean rows first), dad_knn with the domain as the group and mode
    'other', dad_knn_vote.  Returns the buffers: the result lands in ['result_d']."""
    if clean_plan.labels_d is None or noisy_plan.labels_d is None:
        raise ValueError("the split has no labels")
    if clean_plan.device != noisy_plan.device:
        raise ValueError("clean split on %s, noisy split on %s" % (clean_plan.device, noisy_plan.device))
    nc, n = clean_plan.n, clean_plan.n + noisy_plan.n
    if n > _lib.KNN_MAX_N:
        raise ValueError("knn takes at most %d rows of both domains together, got %d" % (_lib.KNN_MAX_N, n))
    b = _knn_buffers(noisy_plan, n, k)
    if "emb" not in b:
        dev = noisy_plan.device
        b["emb"] = torch.empty(n, 256, dtype=torch.float32, device=dev)
        b["labels"] = torch.empty(n, dtype=torch.int64, device=dev)
        b["domain"] = torch.cat([torch.zeros(nc, dtype=torch.int32, device=dev),
                                 torch.ones(noisy_plan.n, dtype=torch.int32, device=dev)])
    b["emb"][:nc].copy_(_enqueue_embeddings(model, clean_plan, False, precision))
    b["emb"][nc:].copy_(_enqueue_embeddings(model, noisy_plan, False, precision))
    b["labels"][:nc].copy_(clean_plan.labels_d)
    b["labels"][nc:].copy_(noisy_plan.labels_d)
    group = _knn_group(b["labels"], b["domain"])
    _enqueue_knn(b["emb"], group, k, _lib.KNN_OTHER, b["idx"], b["d2"], b["ws"])
    _enqueue_knn_vote(b["idx"], b["labels"], group, b["pred"], b["result_d"], b["ws"])
    return b


def cross_domain_knn_store(model, clean_split, noisy_split, k=5, precision="fp32"):
    """Retrieval across the domains with the student's eval-mode embeddings of two FeatureStore splits: every noisy
    utterance is classified by its k nearest clean ones and every clean utterance by its k nearest noisy ones, in one
    dad_knn over both.  Returns {'noisy_to_clean': knn_accuracy's dict over the noisy queries, 'clean_to_noisy': over
    the clean ones}; 'pred' covers the concatenated rows, the clean split's first."""
    model.eval()
    cp, np_ = EvalPlan.of(clean_split), EvalPlan.of(noisy_split)
    r = _read_knn(enqueue_cross_domain_knn_store(model, cp, np_, k, precision), np_.device, True)
    return {"noisy_to_clean": r[1], "clean_to_noisy": r[0]}


def _enqueue_trustworthiness(emb, Y, k, out, penalty, ws, chunks=0):
    fn = _lib.require("dad_trustworthiness_chunked", "trustworthiness")
    _lib.check(fn(_lib.ptr(emb), _lib.ptr(Y), emb.shape[0], int(k), _lib.ptr(out), _lib.ptr(penalty), int(chunks),
                  _lib.ptr(ws), torch.cuda.current_stream(emb.device).cuda_stream), "dad_trustworthiness")


def trustworthiness(emb, Y, k=5, samples=False, _chunks=0):
    """sklearn.manifold.trustworthiness(emb, Y, n_neighbors=k) on the device, for emb [n, 256] and its map Y [n, 2]
    (float32, device): how far the k nearest neighbours in the map are also near in the embedding space, 1.0 when
    every one is among the k nearest there.  Returns {'trustworthiness', 'penalty_sum' (int), 'n', 'k', 'block'};
    samples=True adds the device tensor 'penalty' [n] int32, each row's share.  Equal distances are ordered by index
    (scikit-learn leaves them to its sort).  Raises ValueError unless 1 <= k < n / 2 (scikit-learn's rule), k <= 32
    and n <= 65536, before any launch, and DadError when a row of emb or Y has a non-finite component."""
    emb = _check_emb(emb)
    n = emb.shape[0]
    if not torch.is_tensor(Y) or Y.device != emb.device or Y.dtype != torch.float32 or tuple(Y.shape) != (n, 2):
        raise ValueError("Y must be a float32 tensor [n, 2] on emb's device")
    Y = Y.contiguous()
    k = int(k)
    if not 1 <= k <= _lib.KNN_MAX_K or 2 * k >= n or n > _lib.KNN_MAX_N:
        raise ValueError("trustworthiness takes 1 <= k < n / 2, k <= %d and n <= %d, got n = %d, k = %d"
                         % (_lib.KNN_MAX_K, _lib.KNN_MAX_N, n, k))
    ws = _knn_workspace(n, k, emb.device)
    out = torch.empty(_lib.TW_SLOTS, dtype=torch.float64, device=emb.device)
    pen = torch.empty(n, dtype=torch.int32, device=emb.device) if samples else None
    _enqueue_trustworthiness(emb, Y, k, out, pen, ws, _chunks)
    o = out.cpu().numpy()
    if int(o[_lib.TW_NONFINITE]) > 0:
        raise _lib.DadError("dad_trustworthiness: %d row(s) of emb or Y have a non-finite component"
                            % int(o[_lib.TW_NONFINITE]))
    res = {"trustworthiness": float(o[_lib.TW_T]), "penalty_sum": int(o[_lib.TW_PENALTY]), "n": int(o[_lib.TW_N]),
           "k": int(o[_lib.TW_K]), "block": o}
    if samples:
        res["penalty"] = pen
    return res


def neighbourhood_from_scores(initial, trained):
    """The `initial_weights` / `trained_weights` / `improvement` block (the shape of separation_from_metrics) from two
    {'noisy_knn_accuracy', 'noisy_to_clean_accuracy', 'clean_to_noisy_accuracy'} dicts (per cent); every value a
    Python float."""
    keys = ("noisy_knn_accuracy", "noisy_to_clean_accuracy", "clean_to_noisy_accuracy")
    a = {k: float(initial[k]) for k in keys}
    b = {k: float(trained[k]) for k in keys}
    return {"initial_weights": a, "trained_weights": b,
            "improvement": {k + "_change": b[k] - a[k] for k in keys}}


def neighbourhood_report(initial_model, trained_model, clean_split, noisy_split, k=5):
    """neighbourhood_from_scores under the initial and the trained weights: the noisy split's leave-one-out k-NN
    accuracy (knn_store) and both retrieval accuracies across the domains (cross_domain_knn_store)."""
    def scores(model):
        cross = cross_domain_knn_store(model, clean_split, noisy_split, k)
        return {"noisy_knn_accuracy": knn_store(model, noisy_split, k)["accuracy"],
                "noisy_to_clean_accuracy": cross["noisy_to_clean"]["accuracy"],
                "clean_to_noisy_accuracy": cross["clean_to_noisy"]["accuracy"]}
    return neighbourhood_from_scores(scores(initial_model), scores(trained_model))


# ------------------------------------------------------------------ emotion over time: windows of a split
# Every path above answers once per utterance.  dad_eval_windows (csrc/eval_windows.hip) classifies every sliding
# window, or every prefix, of every utterance in one pass over the store: a window's embedding is a partial sum
# of the per-frame rows the split evaluator computes anyway.  A time-resolved prediction otherwise takes one
# evaluate_store per crop of the features.  Definitions: include/dad.h, "windows of a split".

_WIN_MODES = {"sliding": _lib.WIN_SLIDING, "prefix": _lib.WIN_PREFIX}
_WIN_OUTPUTS = {"w_emb": ((256,), torch.float32), "w_logits": ((4,), torch.float32), "w_probs": ((4,), torch.float32),
                "w_score": ((), torch.float32), "w_pred": ((), torch.int64)}
_UTT_OUTPUTS = {"mean_probs": ((4,), torch.float32), "mean_pred": ((), torch.int64), "vote_pred": ((), torch.int64),
                "last_pred": ((), torch.int64), "settle": ((), torch.int32), "switches": ((), torch.int32)}


def _window_geometry(sizes, hop, span, mode):
    sizes = np.asarray(sizes, dtype=np.int64).reshape(-1)
    hop, span = int(hop), int(span)
    if mode not in _WIN_MODES:
        raise ValueError("mode must be 'sliding' or 'prefix', got %r" % (mode,))
    if hop < 1 or hop >= 2 ** 31 or span < 1 or span >= 2 ** 31:
        raise ValueError("hop and span must be in [1, 2^31), got %d and %d" % (hop, span))
    if mode == "prefix" and span != 1:
        raise ValueError("prefix windows take span = 1, got %d" % span)
    if len(sizes) and (sizes.min() < 0 or sizes.max() >= 2 ** 31):
        raise ValueError("sample sizes must be in [0, 2^31)")
    segs = -(-sizes // hop)
    J = segs if mode == "prefix" else np.where(sizes == 0, 0, np.maximum(1, segs - span + 1))
    return sizes, hop, span, J


def windows_host(sizes, hop, span=1, mode="sliding"):
    """The host side of dad_eval_windows' ragged layouts, a pure function of the per-sample sizes:
    (win_off int32 [n + 1], piece_off int32 [n + 1]), the exclusive prefixes of every utterance's window count J
    and piece count ceil(L / 32) + ceil(L / hop) - ceil(L / lcm(32, hop)) (its frames cut at every multiple of 32
    and of hop).  Raises ValueError when either total reaches 2^31."""
    sizes, hop, span, J = _window_geometry(sizes, hop, span, mode)
    lcm = hop * 32 // int(np.gcd(hop, 32))
    pieces = -(-sizes // 32) + -(-sizes // hop) - -(-sizes // lcm)
    win_off = np.concatenate([[0], np.cumsum(J)])
    piece_off = np.concatenate([[0], np.cumsum(pieces)])
    if win_off[-1] >= 2 ** 31 or piece_off[-1] >= 2 ** 31:
        raise ValueError("the split holds %d windows and %d pieces; the evaluator indexes them with 32 bits"
                         % (win_off[-1], piece_off[-1]))
    return win_off.astype(np.int32), piece_off.astype(np.int32)


def window_frames(sizes, hop, span=1, mode="sliding"):
    """(utterance, start, end) int64 of every window in the order of windows_host: window w is frames
    [start[w], end[w]) of utterance[w]."""
    sizes, hop, span, J = _window_geometry(sizes, hop, span, mode)
    utt = np.repeat(np.arange(len(sizes), dtype=np.int64), J)
    first = np.concatenate([[0], np.cumsum(J)])[:-1]
    j = np.arange(len(utt), dtype=np.int64) - first[utt]
    if mode == "prefix":
        return utt, np.zeros(len(utt), np.int64), np.minimum((j + 1) * hop, sizes[utt])
    return utt, j * hop, np.minimum((j + span) * hop, sizes[utt])


def piece_frames(sizes, hop):
    """(utterance, start, end) int64 of every piece in the order of windows_host's piece prefix."""
    sizes = np.asarray(sizes, dtype=np.int64).reshape(-1)
    hop = int(hop)
    utt, start, end = [], [], []
    for i, L in enumerate(sizes):
        cuts = np.union1d(np.arange(0, L, 32), np.arange(0, L, hop))
        utt.append(np.full(len(cuts), i, np.int64))
        start.append(cuts)
        end.append(np.concatenate([cuts[1:], [L]]) if len(cuts) else cuts)
    cat = lambda v: np.concatenate(v).astype(np.int64) if v else np.zeros(0, np.int64)
    return cat(utt), cat(start), cat(end)


def enqueue_eval_windows(model, plan, hop, span=1, mode="sliding", use_teacher=False, use_entropy=True,
                         precision="fp32", outputs=()):
    """dad_eval_windows on the current stream, enqueue only (no copy, no synchronisation; graph-capturable): the
    DAD_EW_* block lands in plan.window_buffers(hop, span, mode)['result_d'].  One network per call, the teacher
    with use_teacher.  Returns the {name: device tensor} of the requested outputs: per window 'w_emb', 'w_logits',
    'w_probs', 'w_score', 'w_pred' (window order of windows_host), per utterance 'mean_probs', 'mean_pred',
    'vote_pred', 'last_pred', 'settle', 'switches'."""
    prec = _PRECISIONS[precision] if isinstance(precision, str) else int(precision)
    dev = plan.device
    if model.student_flat.device != dev:
        raise RuntimeError("model on %s, store on %s" % (model.student_flat.device, dev))
    b = plan.window_buffers(hop, span, mode)
    out = {}
    for name in outputs:
        if name in _WIN_OUTPUTS:
            (shape, dt), rows = _WIN_OUTPUTS[name], b["windows"]
        elif name in _UTT_OUTPUTS:
            (shape, dt), rows = _UTT_OUTPUTS[name], plan.n
        else:
            raise ValueError("unknown output %r (one of %s)" % (name, ", ".join(list(_WIN_OUTPUTS) + list(_UTT_OUTPUTS))))
        out[name] = torch.empty((rows,) + shape, dtype=dt, device=dev)
    fn = _lib.require("dad_eval_windows", "window inference")
    need = int(_lib.require("dad_eval_windows_workspace_bytes", "window inference")(
        plan.n, plan.slabs, b["windows"], b["pieces"], prec))
    if b["ws"] is None or b["ws"].numel() < need:
        b["ws"] = torch.empty(max(need, 1), dtype=torch.uint8, device=dev)
    store = plan.store
    a = _lib.DadWindowArgs()
    a.store = store.feats.data_ptr()
    a.rows, a.lens, a.slab_off = plan.rows_d.data_ptr(), plan.lens_d.data_ptr(), plan.slab_off_d.data_ptr()
    a.labels = None if plan.labels_d is None else plan.labels_d.data_ptr()
    a.params = (model.teacher_flat if use_teacher else model.student_flat).data_ptr()
    a.win_off, a.piece_off = b["win_off_d"].data_ptr(), b["piece_off_d"].data_ptr()
    a.win_off_host = b["win_off"].ctypes.data
    for name, t in out.items():
        setattr(a, name, t.data_ptr() or None)
    a.result = b["result_d"].data_ptr()
    a.n, a.slabs, a.windows, a.pieces = plan.n, plan.slabs, b["windows"], b["pieces"]
    a.hop, a.span, a.mode = int(hop), int(span), _WIN_MODES[mode]
    a.store_dtype = STORE_DTYPES[store.feats.dtype]
    a.use_entropy = int(bool(use_entropy))
    a.precision = prec
    _lib.check(fn(a, _lib.ptr(b["ws"]), torch.cuda.current_stream(dev).cuda_stream), "dad_eval_windows")
    return out


def _window_block(host):
    """The dict of evaluate_windows_store from the host copy of the DAD_EW_* block."""
    conf = lambda s: host[s:s + 16].reshape(4, 4).copy()
    curve = lambda s: host[s:s + _lib.EW_CURVE].copy()
    return {
        "confusion_mean": conf(_lib.EW_CONF_MEAN), "confusion_vote": conf(_lib.EW_CONF_VOTE),
        "confusion_last": conf(_lib.EW_CONF_LAST), "n": int(host[_lib.EW_N]),
        "n_labelled": int(host[_lib.EW_N_LABELLED]), "n_empty": int(host[_lib.EW_N_EMPTY]),
        "n_windows": int(host[_lib.EW_N_WINDOWS]), "n_nonfinite": int(host[_lib.EW_N_NONFINITE]),
        "reached": curve(_lib.EW_REACHED), "correct": curve(_lib.EW_CORRECT), "carried": curve(_lib.EW_CARRIED),
        "settle_sum": int(host[_lib.EW_SETTLE_SUM]), "switches_sum": int(host[_lib.EW_SWITCHES_SUM]),
        "settle_frames_sum": int(host[_lib.EW_SETTLE_FRAMES_SUM]), "block": host,
    }


def evaluate_windows_store(model, plan_or_store, hop, span=1, mode="sliding", use_teacher=False, use_entropy=True,
                           precision="fp32", outputs=()):
    """One dad_eval_windows over the whole split and one device-to-host copy of its result block.  Returns
    {'confusion_mean', 'confusion_vote', 'confusion_last' [4,4] (row = label; labelled utterances with a window),
    'n', 'n_labelled', 'n_empty', 'n_windows', 'n_nonfinite', 'reached', 'correct', 'carried' [64] (the curve over the
    window index), 'settle_sum', 'switches_sum', 'settle_frames_sum', 'block', 'win_off' (host int32 [n + 1])} as
    NumPy values, plus a device tensor per name in `outputs` (enqueue_eval_windows).  Raises DadError when any
    window has a non-finite logit."""
    plan = EvalPlan.of(plan_or_store)
    out = enqueue_eval_windows(model, plan, hop, span, mode, use_teacher, use_entropy, precision, outputs)
    b = plan.window_buffers(hop, span, mode)
    b["result_h"].copy_(b["result_d"], non_blocking=True)
    torch.cuda.current_stream(plan.device).synchronize()
    res = _window_block(b["result_h"].numpy().copy())
    if res["n_nonfinite"] > 0:
        raise _lib.DadError("dad_eval_windows: %d of %d window(s) have a non-finite logit (fp16: an operand beyond "
                            "+-65504; any precision: non-finite features)" % (res["n_nonfinite"], res["n_windows"]))
    res["win_off"] = b["win_off"]
    res.update(out)
    return res


def _curve_from_block(res, hop):
    live = int(np.count_nonzero(res["reached"]))
    k = max(live, 1)
    base = int(res["reached"][0])                 # labelled utterances with a window
    nonempty = res["n"] - res["n_empty"]
    ratio = lambda a, b: np.divide(100.0 * a, b, out=np.zeros(len(a), np.float64), where=b > 0)
    reached = res["reached"][:k]
    return {
        "frames": (np.arange(k, dtype=np.int64) + 1) * int(hop),
        "reached": reached,
        "accuracy": ratio(res["correct"][:k].astype(np.float64), reached),
        "accuracy_carried": ratio(res["carried"][:k].astype(np.float64), np.full(k, base)),
        "correct": res["correct"][:k], "carried": res["carried"][:k],
        "mean_settle_frames": res["settle_frames_sum"] / nonempty if nonempty else 0.0,
        "mean_switches": res["switches_sum"] / nonempty if nonempty else 0.0,
        "final": metrics_from_confusion(res["confusion_last"]),
    }


def early_decision_curve(model, store_or_loader, hop, precision="fp32"):
    """How much audio the model needs: PREFIX windows of `hop` frames over the split, from one dad_eval_windows.
    Returns, over the prefixes j that some labelled utterance reaches (at most the block's 64): 'frames' =
    (j + 1) * hop, 'reached' (labelled utterances with more than j prefixes), 'accuracy' (per cent correct at prefix
    j among them), 'accuracy_carried' (per cent over every labelled non-empty utterance, one that has ended
    counting with its last prefix), 'correct' / 'carried' (the counts), and 'mean_settle_frames' (the audio after
    which the decision no longer changes), 'mean_switches', 'final' = metrics_from_confusion of the whole-utterance
    predictions.  Where the longest utterance has at most 64 prefixes, accuracy_carried ends at final['accuracy']."""
    model.eval()
    res = evaluate_windows_store(model, store_or_loader, hop, 1, "prefix", precision=precision)
    return _curve_from_block(res, hop)


def duration_report(model, clean_split, noisy_split, hop):
    """The accuracy-against-observed-duration comparison of the two domains: {'clean', 'noisy': early_decision_curve,
    'frames_to_final': {'clean', 'noisy'}: the first `frames` at which the domain's accuracy_carried reaches its own
    final accuracy (None if it does not within the curve)}.  Host arithmetic on the two result blocks."""
    rep = {"frames_to_final": {}}
    for name, split in (("clean", clean_split), ("noisy", noisy_split)):
        c = early_decision_curve(model, split, hop)
        rep[name] = c
        right = int(np.trace(c["final"]["confusion_matrix"]))
        hit = np.nonzero(c["carried"] >= right)[0]
        rep["frames_to_final"][name] = int(c["frames"][hit[0]]) if len(hit) else None
    return rep


def windows(model, feats_list, hop, span=1, mode="sliding", use_teacher=False, precision="fp32",
            outputs=("w_probs", "w_pred")):
    """evaluate_windows_store for a list of [T_i, 768] feature tensors or arrays, through a temporary FeatureStore
    on the model's device: the same dict ('win_off' locates utterance i's windows; window_frames gives their
    frames)."""
    from .data import FeatureStore
    model.eval()
    mats = [torch.as_tensor(f).detach().to("cpu", torch.float32).reshape(-1, 768) for f in feats_list]
    if not mats:
        raise ValueError("no utterances")
    sizes = np.array([m.shape[0] for m in mats], dtype=np.int64)
    offsets = np.concatenate([[0], np.cumsum(sizes)[:-1]])
    store = FeatureStore(torch.cat(mats), sizes, offsets, None, device=model.student_flat.device)
    return evaluate_windows_store(model, store, hop, span, mode, use_teacher, True, precision, outputs)


# ------------------------------------------------------------------ noise response: every noise level in one pass
# The train step asks the model to hold its decision under x + std * N.  dad_eval_noise (csrc/eval_noise.hip)
# evaluates a split at K noise levels of one draw in one pass over the store: the encoder is linear before its ReLU,
# so the pass runs one GEMM on the rows and one on the noise, and a level is an epilogue and a head.  The same draw
# serves every level, so the levels of a call differ by sigma only.  Definitions: include/dad.h, "noise response of
# a split".

_NOISE_OUTPUTS = {"emb": ((256,), torch.float32), "logits": ((4,), torch.float32), "probs": ((4,), torch.float32),
                  "score": ((), torch.float32), "pred": ((), torch.int64), "drift": ((), torch.float32),
                  "kl": ((), torch.float32)}
_NOISE_WORDS = _lib.EN_COUNTS + _lib.EN_SUMS


def _noise_sigmas(sigmas):
    s = [float(v) for v in np.asarray(sigmas, dtype=np.float64).reshape(-1)]
    if not 1 <= len(s) <= _lib.EN_MAX_LEVELS:
        raise ValueError("between 1 and %d noise levels, got %d" % (_lib.EN_MAX_LEVELS, len(s)))
    if any(not np.isfinite(v) or v < 0 for v in s):
        raise ValueError("noise levels must be finite and >= 0, got %r" % (s,))
    return s


def _noise_buffers(plan, K):
    """The buffers of dad_eval_noise over this split at K levels, kept on the plan as the window buffers are:
    {'result_d' / 'result_h' the DAD_EN_* block (counts, then sums) and its pinned host copy, 'ws' the workspace}."""
    b = plan._noise.get(K)
    if b is None:
        b = {"result_d": torch.zeros(_NOISE_WORDS, dtype=torch.int64, device=plan.device),
             "result_h": torch.zeros(_NOISE_WORDS, dtype=torch.int64).pin_memory(), "ws": None}
        plan._noise[K] = b
    return b


def _noise_args(plan, seed, draw):
    a = _lib.DadNoiseArgs()
    a.rows, a.lens, a.slab_off = plan.rows_d.data_ptr(), plan.lens_d.data_ptr(), plan.slab_off_d.data_ptr()
    a.n, a.slabs = plan.n, plan.slabs
    a.seed, a.draw = int(seed), int(draw)
    return a


def noise_draws(plan, seed=0, draw=0):
    """The probe (dad_eval_noise_draws): the standard normals that a counter-mode call with (seed, draw) adds to this
    split, as a device tensor [32 * slabs, 768] in the explicit layout: frame t of utterance i is row
    32 * slab_off[i] + t (zeros in the rows past an utterance's length).  Feeding it back as `noise=` repeats the
    counter call bit for bit."""
    plan = EvalPlan.of(plan)
    fn = _lib.require("dad_eval_noise_draws", "the noise response")
    out = torch.empty((32 * plan.slabs, 768), dtype=torch.float32, device=plan.device)
    _lib.check(fn(_noise_args(plan, seed, draw), _lib.ptr(out), torch.cuda.current_stream(plan.device).cuda_stream),
               "dad_eval_noise_draws")
    return out


def enqueue_eval_noise(model, plan, sigmas, seed=0, draw=0, use_teacher=False, use_entropy=True, precision="fp32",
                       outputs=(), noise=None, _block=None):
    """dad_eval_noise on the current stream, enqueue only (no copy, no synchronisation; graph-capturable): level k
    evaluates x + sigmas[k] * n for one draw n of standard normals, the counter RNG's (seed, draw) or the explicit
    device tensor `noise` [32 * slabs, 768] (noise_draws' layout).  One network per call, the teacher with
    use_teacher.  The DAD_EN_* block lands in the plan's buffer of K = len(sigmas) levels (or in _block, an int64
    device tensor of EN_COUNTS + EN_SUMS words).  Returns the {name: device tensor} of the requested outputs:
    'emb', 'logits', 'probs', 'score', 'pred', 'drift', 'kl' ([K, n, ...], level-major) and 'break_level' [n]."""
    prec = _PRECISIONS[precision] if isinstance(precision, str) else int(precision)
    sig = _noise_sigmas(sigmas)
    K = len(sig)
    dev = plan.device
    if model.student_flat.device != dev:
        raise RuntimeError("model on %s, store on %s" % (model.student_flat.device, dev))
    if noise is not None:
        if (noise.dtype != torch.float32 or noise.device != dev or not noise.is_contiguous()
                or tuple(noise.shape) != (32 * plan.slabs, 768)):
            raise ValueError("noise must be a contiguous float32 [%d, 768] tensor on %s" % (32 * plan.slabs, dev))
    out = {}
    for name in outputs:
        if name == "break_level":
            out[name] = torch.empty((plan.n,), dtype=torch.int32, device=dev)
        elif name in _NOISE_OUTPUTS:
            shape, dt = _NOISE_OUTPUTS[name]
            out[name] = torch.empty((K, plan.n) + shape, dtype=dt, device=dev)
        else:
            raise ValueError("unknown output %r (one of %s, break_level)" % (name, ", ".join(_NOISE_OUTPUTS)))
    fn = _lib.require("dad_eval_noise", "the noise response")
    b = _noise_buffers(plan, K)
    need = int(_lib.require("dad_eval_noise_workspace_bytes", "the noise response")(plan.n, plan.slabs, K, prec))
    if b["ws"] is None or b["ws"].numel() < need:
        b["ws"] = torch.empty(max(need, 1), dtype=torch.uint8, device=dev)
    block = b["result_d"] if _block is None else _block
    store = plan.store
    a = _noise_args(plan, seed, draw)
    a.store = store.feats.data_ptr()
    a.labels = None if plan.labels_d is None else plan.labels_d.data_ptr()
    a.params = (model.teacher_flat if use_teacher else model.student_flat).data_ptr()
    a.noise = None if noise is None else noise.data_ptr()
    for name, t in out.items():
        setattr(a, name, t.data_ptr() or None)
    a.counts = block.data_ptr()
    a.sums = block.data_ptr() + 8 * _lib.EN_COUNTS
    a.levels = K
    a.sigma[:K] = sig
    a.store_dtype = STORE_DTYPES[store.feats.dtype]
    a.use_entropy = int(bool(use_entropy))
    a.precision = prec
    _lib.check(fn(a, _lib.ptr(b["ws"]), torch.cuda.current_stream(dev).cuda_stream), "dad_eval_noise")
    return out


def _noise_block(host, sigmas):
    """The dict of evaluate_noise_store from the host copy of the DAD_EN_* block."""
    counts = host[:_lib.EN_COUNTS]
    sums = host[_lib.EN_COUNTS:].view(np.float64)
    K, n = int(counts[_lib.EN_LEVELS]), int(counts[_lib.EN_N])
    res = {"n": n, "n_labelled": int(counts[_lib.EN_N_LABELLED]), "n_skipped": int(counts[_lib.EN_N_SKIPPED]),
           "n_nonfinite": int(counts[_lib.EN_N_NONFINITE]), "n_levels": K, "sigmas": list(sigmas),
           "confusion": counts[_lib.EN_CONF:_lib.EN_CONF + 16 * _lib.EN_MAX_LEVELS].reshape(-1, 4, 4)[:K].copy(),
           "flips": counts[_lib.EN_FLIPS:_lib.EN_FLIPS + K].copy(),
           "survive": counts[_lib.EN_SURVIVE:_lib.EN_SURVIVE + K].copy(),
           "sum_score": sums[_lib.EN_SUM_SCORE:_lib.EN_SUM_SCORE + K].copy(),
           "sum_drift": sums[_lib.EN_SUM_DRIFT:_lib.EN_SUM_DRIFT + K].copy(),
           "sum_kl": sums[_lib.EN_SUM_KL:_lib.EN_SUM_KL + K].copy(), "block": host, "levels": []}
    for k in range(K):
        lv = metrics_from_confusion(res["confusion"][k]) if res["n_labelled"] else {}
        lv.update(sigma=res["sigmas"][k], flip_rate=res["flips"][k] / n, survival=res["survive"][k] / n,
                  mean_score=res["sum_score"][k] / n, mean_drift=res["sum_drift"][k] / n, mean_kl=res["sum_kl"][k] / n)
        res["levels"].append(lv)
    return res


def _check_noise_block(res):
    if res["n_nonfinite"] > 0:
        raise _lib.DadError("dad_eval_noise: %d of %d utterance(s) have a non-finite logit (fp16: an operand beyond "
                            "+-65504; any precision: non-finite features)" % (res["n_nonfinite"], res["n"]))


def evaluate_noise_store(model, plan_or_store, sigmas, seed=0, draw=0, use_teacher=False, use_entropy=True,
                         precision="fp32", outputs=(), noise=None):
    """One dad_eval_noise over the whole split and one device-to-host copy of its result block.  Returns {'levels':
    per level metrics_from_confusion's dict (when the split has labels) plus 'sigma', 'flip_rate' (predictions that
    left level 0's), 'survival' (utterances whose break level lies above this level), 'mean_score', 'mean_drift',
    'mean_kl'; 'confusion' [K,4,4], 'flips', 'survive' [K], 'sum_score', 'sum_drift', 'sum_kl' [K] (float64), 'n',
    'n_labelled', 'n_skipped', 'n_nonfinite', 'n_levels', 'sigmas', 'block'} as NumPy values, plus a device tensor
    per name in `outputs` (enqueue_eval_noise).  Raises DadError when any utterance has a non-finite logit."""
    plan = EvalPlan.of(plan_or_store)
    sig = _noise_sigmas(sigmas)
    out = enqueue_eval_noise(model, plan, sig, seed, draw, use_teacher, use_entropy, precision, outputs, noise)
    b = _noise_buffers(plan, len(sig))
    b["result_h"].copy_(b["result_d"], non_blocking=True)
    torch.cuda.current_stream(plan.device).synchronize()
    res = _noise_block(b["result_h"].numpy().copy(), sig)
    _check_noise_block(res)
    res.update(out)
    return res


def default_noise_levels(cfg=None):
    """(0.0, WEAK_NOISE_STD, STRONG_NOISE_STD) of the config (None: the IEMOCAP defaults), read at call time: the
    perturbations training asks the model to be consistent under."""
    from .config import ConfigView
    view = ConfigView(flavor="iemocap") if cfg is None else cfg
    return (0.0, float(view.WEAK_NOISE_STD), float(view.STRONG_NOISE_STD))


_CURVE_KEYS = (("accuracy", "accuracy"), ("balanced_accuracy", "weighted_accuracy"), ("flip_rate", "flip_rate"),
               ("mean_kl", "mean_kl"))


def noise_response_curve(model, store_or_loader, sigmas=None, draws=8, seed=0, use_teacher=False, precision="fp32",
                         cfg=None):
    """The split's response to additive noise over `draws` independent draws (draw = 0 .. draws - 1 of `seed`):
    `draws` dad_eval_noise calls enqueued into separate result blocks, one synchronisation.  sigmas=None means
    default_noise_levels(cfg).  Returns {'sigmas', 'draws', per level lists 'accuracy', 'balanced_accuracy',
    'flip_rate', 'mean_kl': {'mean', 'std'} (the mean and the population standard deviation across draws; per cent
    for the two accuracies), 'per_draw' (evaluate_noise_store's dict of every draw, without outputs) and 'flip_prob'
    [K, n], a float32 device tensor: the share of draws in which utterance i's prediction at level k left its
    level-0 prediction}."""
    model.eval()
    plan = EvalPlan.of(store_or_loader)
    sig = _noise_sigmas(default_noise_levels(cfg) if sigmas is None else sigmas)
    draws = int(draws)
    if draws < 1:
        raise ValueError("draws must be >= 1")
    if plan.labels_d is None:
        raise ValueError("the split has no labels")
    dev = plan.device
    blocks_d = torch.zeros((draws, _NOISE_WORDS), dtype=torch.int64, device=dev)
    blocks_h = torch.zeros((draws, _NOISE_WORDS), dtype=torch.int64).pin_memory()
    flips = torch.zeros((len(sig), plan.n), dtype=torch.float32, device=dev)
    for d in range(draws):
        pred = enqueue_eval_noise(model, plan, sig, seed, d, use_teacher, True, precision, ("pred",),
                                  _block=blocks_d[d])["pred"]
        flips += (pred != pred[0:1]).to(torch.float32)
    flips /= draws
    blocks_h.copy_(blocks_d, non_blocking=True)
    torch.cuda.current_stream(dev).synchronize()
    per_draw = [_noise_block(blocks_h[d].numpy().copy(), sig) for d in range(draws)]
    for r in per_draw:
        _check_noise_block(r)
    res = {"sigmas": sig, "draws": draws, "per_draw": per_draw, "flip_prob": flips}
    for name, key in _CURVE_KEYS:
        v = np.array([[r["levels"][k][key] for k in range(len(sig))] for r in per_draw], dtype=np.float64)
        res[name] = {"mean": v.mean(0).tolist(), "std": v.std(0).tolist()}
    return res


def robustness_from_curves(initial, trained):
    """The `initial_weights` / `trained_weights` / `improvement` block (the shape of separation_from_metrics) from two
    noise_response_curve dicts: per level the mean accuracy (per cent) and the mean flip rate; every value a Python
    float."""
    pick = lambda c: {"sigmas": [float(s) for s in c["sigmas"]],
                      "accuracy": [float(v) for v in c["accuracy"]["mean"]],
                      "flip_rate": [float(v) for v in c["flip_rate"]["mean"]]}
    a, b = pick(initial), pick(trained)
    return {"initial_weights": a, "trained_weights": b,
            "improvement": {"accuracy_change": [y - x for x, y in zip(a["accuracy"], b["accuracy"])],
                            "flip_rate_change": [y - x for x, y in zip(a["flip_rate"], b["flip_rate"])]}}


def robustness_report(initial_model, trained_model, store_or_loader, sigmas=None, draws=8):
    """robustness_from_curves of noise_response_curve under the initial and the trained weights, on the same draws."""
    return robustness_from_curves(noise_response_curve(initial_model, store_or_loader, sigmas, draws),
                                  noise_response_curve(trained_model, store_or_loader, sigmas, draws))


# ---- the worst-case perturbation: input gradients, FGSM and PGD (dad_input_grad, csrc/input_grad.hip) -------------
_IG_OUTPUTS = ("grad", "delta", "frame_l1")
_ADV_MAX_EPS = _lib.EN_MAX_LEVELS - 1
_TARGETS = ("label", "pred")


def _ig_buffers(plan):
    """The buffers of dad_input_grad over this split, kept on the plan beside the noise buffers: {'counts_d' /
    'counts_h' the DAD_IG_* block and its pinned host copy, 'ws' the workspace, 'row_utt' the utterance of every row
    of the explicit layout}."""
    b = plan._noise.get("input_grad")
    if b is None:
        nslab = (plan.slab_off_d[1:] - plan.slab_off_d[:-1]).to(torch.int64)
        b = {"counts_d": torch.zeros(_lib.IG_COUNTS, dtype=torch.int64, device=plan.device),
             "counts_h": torch.zeros(_lib.IG_COUNTS, dtype=torch.int64).pin_memory(), "ws": None,
             "row_utt": torch.repeat_interleave(torch.arange(plan.n, device=plan.device), 32 * nslab)}
        plan._noise["input_grad"] = b
    return b


def _explicit_tensor(plan, t, what):
    if (t.dtype != torch.float32 or t.device != plan.device or not t.is_contiguous()
            or tuple(t.shape) != (32 * plan.slabs, 768)):
        raise ValueError("%s must be a contiguous float32 [%d, 768] tensor on %s" % (what, 32 * plan.slabs, plan.device))
    return t


def enqueue_input_grad(model, plan, dz, delta=None, alpha=1.0, radius=float("inf"), use_teacher=False,
                       precision="fp32", outputs=("delta",), _delta_out=None, _counts=None):
    """dad_input_grad on the current stream, enqueue only (no copy, no synchronisation; graph-capturable): for the
    logit cotangents dz [n, 4] (float32, on the device) the gradient G of sum_u dz_u . z_u with respect to the
    stored frames, taken at x + delta, and the signed step clamp(delta + alpha * sgn(G), -radius, +radius).  delta
    is None or a float32 [32 * slabs, 768] device tensor in noise_draws' layout (frame t of utterance i in row
    32 * slab_off[i] + t).  outputs: 'grad' and 'delta' [32 * slabs, 768], 'frame_l1' [32 * slabs]; rows past an
    utterance's length are 0.  With a `delta` given, 'delta' is that tensor, updated in place.  The DAD_IG_* counts
    land in the plan's block.  Every tensor of the explicit layout is float32, 3 KB per frame: about 4 GB for a
    split of 5,531 utterances, per tensor.  Returns the {name: device tensor} of the requested outputs."""
    prec = _PRECISIONS[precision] if isinstance(precision, str) else int(precision)
    dev = plan.device
    if model.student_flat.device != dev:
        raise RuntimeError("model on %s, store on %s" % (model.student_flat.device, dev))
    alpha, radius = float(alpha), float(radius)
    if not np.isfinite(alpha):
        raise ValueError("alpha must be finite, got %r" % alpha)
    if not radius >= 0:
        raise ValueError("radius must be >= 0 (inf: no clamp), got %r" % radius)
    if dz.dtype != torch.float32 or dz.device != dev or not dz.is_contiguous() or tuple(dz.shape) != (plan.n, 4):
        raise ValueError("dz must be a contiguous float32 [%d, 4] tensor on %s" % (plan.n, dev))
    if delta is not None:
        _explicit_tensor(plan, delta, "delta")
    out = {}
    for name in outputs:
        if name not in _IG_OUTPUTS:
            raise ValueError("unknown output %r (one of %s)" % (name, ", ".join(_IG_OUTPUTS)))
        if name == "frame_l1":
            out[name] = torch.empty((32 * plan.slabs,), dtype=torch.float32, device=dev)
        elif name == "delta" and _delta_out is not None:
            out[name] = _explicit_tensor(plan, _delta_out, "_delta_out")
        elif name == "delta" and delta is not None:
            out[name] = delta
        else:
            out[name] = torch.empty((32 * plan.slabs, 768), dtype=torch.float32, device=dev)
    fn = _lib.require("dad_input_grad", "the input gradients")
    b = _ig_buffers(plan)
    need = int(_lib.require("dad_input_grad_workspace_bytes", "the input gradients")(plan.n, plan.slabs, prec))
    if b["ws"] is None or b["ws"].numel() < need:
        b["ws"] = torch.empty(max(need, 1), dtype=torch.uint8, device=dev)
    counts = b["counts_d"] if _counts is None else _counts
    store = plan.store
    a = _lib.DadInputGradArgs()
    a.store = store.feats.data_ptr()
    a.rows, a.lens, a.slab_off = plan.rows_d.data_ptr(), plan.lens_d.data_ptr(), plan.slab_off_d.data_ptr()
    a.params = (model.teacher_flat if use_teacher else model.student_flat).data_ptr()
    a.dz = dz.data_ptr()
    a.delta_in = None if delta is None else (delta.data_ptr() or None)
    a.grad = out["grad"].data_ptr() or None if "grad" in out else None
    a.delta_out = out["delta"].data_ptr() or None if "delta" in out else None
    a.frame_l1 = out["frame_l1"].data_ptr() or None if "frame_l1" in out else None
    a.counts = counts.data_ptr()
    a.n, a.slabs = plan.n, plan.slabs
    a.alpha, a.radius = alpha, radius
    a.store_dtype = STORE_DTYPES[store.feats.dtype]
    a.precision = prec
    _lib.check(fn(a, _lib.ptr(b["ws"]), torch.cuda.current_stream(dev).cuda_stream), "dad_input_grad")
    return out


def _adv_target(plan, pred, target):
    """The class each utterance's cross-entropy is taken against: its label where that lies in [0, 4), the network's
    own clean prediction otherwise; 'pred' uses the prediction everywhere."""
    if target == "pred":
        return pred
    lab = plan.labels_d
    return torch.where((lab >= 0) & (lab < 4), lab, pred)


def _adv_check(plan, target):
    if target not in _TARGETS:
        raise ValueError("unknown target %r (one of %s)" % (target, ", ".join(_TARGETS)))
    if target == "label" and plan.labels_d is None:
        raise ValueError("the split has no labels: target='label' needs them (or use target='pred')")


def _ce_cotangent(logits, tgt):
    """softmax(z) - onehot(target): the gradient of plain (not label-smoothed) cross-entropy with respect to z"""
    return (torch.softmax(logits, dim=1) - torch.nn.functional.one_hot(tgt, 4).to(torch.float32)).contiguous()


def _read_ig_counts(plan, counts_d=None):
    b = _ig_buffers(plan)
    b["counts_h"].copy_(b["counts_d"] if counts_d is None else counts_d, non_blocking=True)
    torch.cuda.current_stream(plan.device).synchronize()
    c = b["counts_h"].numpy().copy()
    if c[_lib.IG_NONFINITE] > 0:
        raise _lib.DadError("dad_input_grad: %d gradient element(s) are not finite (fp16: an operand beyond +-65504; any "
                            "precision: non-finite features or cotangents)" % c[_lib.IG_NONFINITE])
    return {"frames": int(c[_lib.IG_FRAMES]), "n_nonfinite_grad": int(c[_lib.IG_NONFINITE]),
            "n_zero_grad": int(c[_lib.IG_ZERO])}


def input_gradients(model, store_or_loader, target="label", use_teacher=False, precision="fp32"):
    """The gradient of each utterance's plain cross-entropy against `target` ('label', or 'pred': the network's own
    prediction) with respect to its stored frames: one dad_eval_split, the cotangent softmax(z) - onehot(target) on
    the device, one dad_input_grad.  Returns {'grad' [32 * slabs, 768] and 'frame_l1' [32 * slabs] (sum_d |G_t[d]|:
    which frames the decision hangs on) in noise_draws' layout, 'utt_l1' [n] (sum |G| of an utterance: the
    first-order loss increase per unit of an L-infinity perturbation), 'target' [n], 'dz' [n, 4], 'frames',
    'n_nonfinite_grad', 'n_zero_grad'}.  'grad' is float32, 3 KB per frame (about 4 GB for 5,531 utterances).
    Raises DadError on a gradient element that is not finite."""
    model.eval()
    plan = EvalPlan.of(store_or_loader)
    _adv_check(plan, target)
    lname, pname = ("t_logits", "t_pred") if use_teacher else ("logits", "pred")
    ev = enqueue_eval_split(model, plan, use_teacher, True, precision, (lname, pname))
    tgt = _adv_target(plan, ev[pname], target)
    dz = _ce_cotangent(ev[lname], tgt)
    out = enqueue_input_grad(model, plan, dz, None, 0.0, float("inf"), use_teacher, precision, ("grad", "frame_l1"))
    utt = torch.zeros(plan.n, dtype=torch.float32, device=plan.device)
    utt.index_add_(0, _ig_buffers(plan)["row_utt"], out["frame_l1"])
    res = _read_ig_counts(plan)
    res.update(grad=out["grad"], frame_l1=out["frame_l1"], utt_l1=utt, target=tgt, dz=dz)
    return res


def _adv_epsilons(epsilons):
    e = [float(v) for v in np.asarray(epsilons, dtype=np.float64).reshape(-1)]
    if not 1 <= len(e) <= _ADV_MAX_EPS:
        raise ValueError("between 1 and %d epsilons, got %d (level 0 is the clean base)" % (_ADV_MAX_EPS, len(e)))
    if any(not np.isfinite(v) or v < 0 for v in e):
        raise ValueError("epsilons must be finite and >= 0, got %r" % (e,))
    return e


def _adv_result(res, eps):
    res.pop("sigmas")
    res["epsilons"] = [0.0] + list(eps)
    for lv in res["levels"]:
        lv["epsilon"] = lv.pop("sigma")
    return res


def evaluate_adversarial_store(model, plan_or_store, epsilons, steps=1, alpha=None, target="label", use_teacher=False,
                               precision="fp32", outputs=()):
    """The split under the worst-case perturbation of L-infinity size epsilon, for up to 7 epsilons.  The loss is the
    plain cross-entropy against `target` (the label where it lies in [0, 4), the clean prediction otherwise; 'pred':
    the prediction everywhere), not the trainer's label-smoothed one.

    steps == 1 with alpha None is FGSM (Goodfellow et al. 2015): one dad_eval_split, one dad_input_grad for the
    direction sgn(dL/dx), then ONE dad_eval_noise(noise=direction, sigmas=(0, eps_1 .. eps_K)): the encoder is linear
    before its ReLU, so a fixed direction at several epsilons costs what one noise draw at several sigmas does.
    Otherwise PGD (Madry et al. 2018), per epsilon: delta_0 = 0; `steps` times the logits at x + delta_j
    (dad_eval_noise(noise=delta_j, sigmas=(1,))), their cotangent, and delta_{j+1} = clamp(delta_j + alpha *
    sgn(G(x + delta_j)), +-eps) in place; then one dad_eval_noise(noise=delta, sigmas=(0, 1)).  alpha defaults to
    2.5 * eps / steps.

    Returns evaluate_noise_store's dict with 'epsilons' (level 0 is the clean base, epsilon 0) in place of 'sigmas'
    and 'epsilon' in place of each level's 'sigma', plus 'n_nonfinite_grad' and 'n_zero_grad', and a device tensor per
    name in `outputs` (enqueue_eval_noise's, level-major over the K + 1 levels, and 'direction': FGSM's sign tensor
    [32 * slabs, 768], or the list of PGD's final delta per epsilon).  The direction is materialised as float32, 3 KB
    per frame: about 4 GB for a split of 5,531 utterances.  Raises DadError on non-finite logits or gradients."""
    model.eval()
    plan = EvalPlan.of(plan_or_store)
    _adv_check(plan, target)
    eps = _adv_epsilons(epsilons)
    steps = int(steps)
    if steps < 1:
        raise ValueError("steps must be >= 1")
    want_dir = "direction" in outputs
    outputs = tuple(o for o in outputs if o != "direction")
    for name in outputs:
        if name != "break_level" and name not in _NOISE_OUTPUTS:
            raise ValueError("unknown output %r (one of %s, break_level, direction)" % (name, ", ".join(_NOISE_OUTPUTS)))
    dev = plan.device
    if model.student_flat.device != dev:
        raise RuntimeError("model on %s, store on %s" % (model.student_flat.device, dev))
    lname, pname = ("t_logits", "t_pred") if use_teacher else ("logits", "pred")
    ev = enqueue_eval_split(model, plan, use_teacher, True, precision, (lname, pname))
    tgt = _adv_target(plan, ev[pname], target)
    if steps == 1 and alpha is None:
        direction = enqueue_input_grad(model, plan, _ce_cotangent(ev[lname], tgt), None, 1.0, float("inf"),
                                       use_teacher, precision, ("delta",))["delta"]
        grad_counts = _read_ig_counts(plan)
        res = evaluate_noise_store(model, plan, [0.0] + eps, 0, 0, use_teacher, True, precision, outputs, direction)
        res = _adv_result(res, eps)
        res.update(grad_counts)
        if want_dir:
            res["direction"] = direction
        return res

    total = torch.zeros(_lib.IG_COUNTS, dtype=torch.int64, device=dev)
    delta = torch.empty((32 * plan.slabs, 768), dtype=torch.float32, device=dev)
    want = tuple(dict.fromkeys(tuple(o for o in outputs if o != "break_level") + ("pred",)))
    runs, finals = [], []
    for e in eps:
        a = 2.5 * e / steps if alpha is None else float(alpha)
        delta.zero_()
        for _ in range(steps):
            z = enqueue_eval_noise(model, plan, (1.0,), 0, 0, use_teacher, True, precision, ("logits",), delta)["logits"]
            enqueue_input_grad(model, plan, _ce_cotangent(z[0], tgt), delta, a, e, use_teacher, precision, ("delta",))
            total += _ig_buffers(plan)["counts_d"]
        runs.append(evaluate_noise_store(model, plan, (0.0, 1.0), 0, 0, use_teacher, True, precision, want, delta))
        if want_dir:
            finals.append(delta.clone())
    grad_counts = _read_ig_counts(plan, total)
    # one block over the K + 1 levels: level 0 of the first run, level 1 of every run
    K = len(eps) + 1
    host = np.zeros(_NOISE_WORDS, dtype=np.int64)
    counts, sums = host[:_lib.EN_COUNTS], host[_lib.EN_COUNTS:].view(np.float64)
    preds = torch.cat([runs[0]["pred"][0:1]] + [r["pred"][1:2] for r in runs])
    moved = preds != preds[0:1]
    brk = torch.where(moved.any(0), moved.to(torch.int32).argmax(0).to(torch.int32),
                      torch.full((plan.n,), K, dtype=torch.int32, device=dev))
    survive = (brk[None, :] > torch.arange(K, device=dev, dtype=torch.int32)[:, None]).sum(1).cpu().numpy()
    for k in range(K):
        r, j = (runs[0], 0) if k == 0 else (runs[k - 1], 1)
        rc, rs = r["block"][:_lib.EN_COUNTS], r["block"][_lib.EN_COUNTS:].view(np.float64)
        counts[_lib.EN_CONF + 16 * k:_lib.EN_CONF + 16 * k + 16] = rc[_lib.EN_CONF + 16 * j:_lib.EN_CONF + 16 * j + 16]
        counts[_lib.EN_FLIPS + k] = rc[_lib.EN_FLIPS + j]
        counts[_lib.EN_SURVIVE + k] = survive[k]
        for slot in (_lib.EN_SUM_SCORE, _lib.EN_SUM_DRIFT, _lib.EN_SUM_KL):
            sums[slot + k] = rs[slot + j]
    rc = runs[0]["block"]
    for slot in (_lib.EN_N, _lib.EN_N_LABELLED, _lib.EN_N_SKIPPED):
        counts[slot] = rc[slot]
    counts[_lib.EN_N_NONFINITE] = max(int(r["n_nonfinite"]) for r in runs)
    counts[_lib.EN_LEVELS] = K
    res = _adv_result(_noise_block(host, [0.0] + eps), eps)
    res.update(grad_counts)
    for name in outputs:
        if name == "break_level":
            res[name] = brk
        else:
            res[name] = torch.cat([runs[0][name][0:1]] + [r[name][1:2] for r in runs])
    if want_dir:
        res["direction"] = finals
    return res


def adversarial_response_curve(model, store_or_loader, epsilons=None, steps=1, alpha=None, target="label",
                               use_teacher=False, precision="fp32", cfg=None):
    """noise_response_curve's shape for the worst-case perturbation: epsilons=None means default_noise_levels(cfg), so
    the curve shares its axis with noise_response_curve (a leading 0 is the clean base level and is not attacked).
    Returns {'sigmas' (the axis: 0 and the epsilons), 'epsilons', 'draws': 1, per level lists 'accuracy',
    'balanced_accuracy', 'flip_rate', 'mean_kl': {'mean', 'std'} (std 0: the direction is deterministic),
    'per_draw': [evaluate_adversarial_store's dict]}.  The direction costs 3 KB per frame (evaluate_adversarial_store)."""
    plan = EvalPlan.of(store_or_loader)
    if plan.labels_d is None:
        raise ValueError("the split has no labels")
    eps = [float(v) for v in (default_noise_levels(cfg) if epsilons is None else epsilons)]
    if eps and eps[0] == 0.0:
        eps = eps[1:]
    r = evaluate_adversarial_store(model, plan, eps, steps, alpha, target, use_teacher, precision)
    res = {"sigmas": list(r["epsilons"]), "epsilons": list(r["epsilons"]), "draws": 1, "per_draw": [r]}
    for name, key in _CURVE_KEYS:
        v = [float(lv[key]) for lv in r["levels"]]
        res[name] = {"mean": v, "std": [0.0] * len(v)}
    return res


def worst_case_report(initial_model, trained_model, store_or_loader, epsilons=None, steps=1, draws=8):
    """The random and the worst-case response on one axis: {'random': robustness_from_curves of noise_response_curve,
    'worst_case': robustness_from_curves of adversarial_response_curve}, each for the initial and the trained weights
    at the same levels (epsilons=None: default_noise_levels)."""
    return {"random": robustness_from_curves(noise_response_curve(initial_model, store_or_loader, epsilons, draws),
                                             noise_response_curve(trained_model, store_or_loader, epsilons, draws)),
            "worst_case": robustness_from_curves(
                adversarial_response_curve(initial_model, store_or_loader, epsilons, steps),
                adversarial_response_curve(trained_model, store_or_loader, epsilons, steps))}


# ---- why a split is classified as it is: exact integrated gradients (dad_attribution, csrc/attribution.hip) -------
_AT_OUTPUTS = ("attr", "frame_attr", "chan_attr", "utt_total")
_AT_TARGETS = ("pred", "label", "margin")


def _at_check_outputs(outputs):
    outputs = tuple(outputs)
    for name in outputs:
        if name not in _AT_OUTPUTS:
            raise ValueError("unknown output %r (one of %s)" % (name, ", ".join(_AT_OUTPUTS)))
    return outputs


def _at_check_target(target):
    if isinstance(target, str):
        if target not in _AT_TARGETS:
            raise ValueError("unknown target %r (one of %s, or a class index)" % (target, ", ".join(_AT_TARGETS)))
        return target
    if isinstance(target, bool) or not isinstance(target, (int, np.integer)) or not 0 <= int(target) < 4:
        raise ValueError("a target class index must be an integer in [0, 4), got %r" % (target,))
    return int(target)


def _at_check_baseline(baseline, allow_mean):
    """None, 'mean' (integrated_gradients only) or a contiguous float32 [768] tensor; the device is checked against
    the plan's by the caller."""
    if baseline is None or (allow_mean and isinstance(baseline, str) and baseline == "mean"):
        return baseline
    if (not isinstance(baseline, torch.Tensor) or baseline.dtype != torch.float32 or tuple(baseline.shape) != (768,)
            or not baseline.is_contiguous()):
        raise ValueError("baseline must be None%s or a contiguous float32 [768] tensor, got %s"
                         % (", 'mean'" if allow_mean else "",
                            "%s %s" % (baseline.dtype, tuple(baseline.shape)) if isinstance(baseline, torch.Tensor)
                            else repr(baseline)))
    return baseline


def _at_buffers(plan):
    b = plan._noise.get("attribution")
    if b is None:
        b = {"counts_d": torch.zeros(_lib.AT_COUNTS, dtype=torch.int64, device=plan.device),
             "counts_h": torch.zeros(_lib.AT_COUNTS, dtype=torch.int64).pin_memory(), "ws": None}
        plan._noise["attribution"] = b
    return b


def _at_args(model, plan, dz, baseline, use_teacher, prec, out, counts):
    store = plan.store
    a = _lib.DadAttributionArgs()
    a.store = store.feats.data_ptr()
    a.rows, a.lens, a.slab_off = plan.rows_d.data_ptr(), plan.lens_d.data_ptr(), plan.slab_off_d.data_ptr()
    a.params = (model.teacher_flat if use_teacher else model.student_flat).data_ptr()
    a.dz = dz.data_ptr()
    a.baseline = None if baseline is None else baseline.data_ptr()
    for name in _AT_OUTPUTS:
        setattr(a, name, (out[name].data_ptr() or None) if name in out else None)
    a.counts = counts.data_ptr()
    a.n, a.slabs = plan.n, plan.slabs
    a.store_dtype = STORE_DTYPES[store.feats.dtype]
    a.precision = prec
    return a


def _at_plan(a):
    slots = (ctypes.c_int64 * _lib.AT_PLAN_SLOTS)()
    _lib.check(_lib.require("dad_attribution_plan", "the attributions")(a, slots), "dad_attribution_plan")
    return {"mode": "full" if slots[_lib.AT_PLAN_MODE] else "frame_only",
            "workspace_bytes": int(slots[_lib.AT_PLAN_BYTES]), "launches": int(slots[_lib.AT_PLAN_LAUNCHES]),
            "kernel": int(slots[_lib.AT_PLAN_KERNEL])}


def enqueue_attribution(model, plan, dz, baseline=None, use_teacher=False, precision="fp32", outputs=("frame_attr",),
                        _counts=None, _plan_only=False, _out=None):
    """dad_attribution on the current stream, enqueue only (no copy, no synchronisation; graph-capturable): exact
    integrated gradients of sum_u dz_u . z_u along the straight path from the baseline row (None: zeros, or a float32
    [768] device tensor) to every stored frame, with the logit cotangents dz [n, 4] (float32, on the device) held
    fixed along the path.  outputs: 'attr' [32 * slabs, 768] and 'frame_attr' [32 * slabs] in noise_draws' layout
    (frame t of utterance i in row 32 * slab_off[i] + t; rows past an utterance's length are 0), 'chan_attr'
    [n, 768], 'utt_total' [n].  Without 'attr' and 'chan_attr' the call runs one GEMM (frame-only mode), else two.
    'attr' is float32, 3 KB per frame (about 4 GB for 5,531 utterances).  The DAD_AT_* counts land in the plan's
    block.  Returns the {name: device tensor} of the requested outputs."""
    prec = _PRECISIONS[precision] if isinstance(precision, str) else int(precision)
    outputs = _at_check_outputs(outputs)
    _at_check_baseline(baseline, False)
    dev = plan.device
    if model.student_flat.device != dev:
        raise RuntimeError("model on %s, store on %s" % (model.student_flat.device, dev))
    if baseline is not None and baseline.device != dev:
        raise ValueError("baseline on %s, store on %s" % (baseline.device, dev))
    if (not isinstance(dz, torch.Tensor) or dz.dtype != torch.float32 or dz.device != dev or not dz.is_contiguous()
            or tuple(dz.shape) != (plan.n, 4)):
        raise ValueError("dz must be a contiguous float32 [%d, 4] tensor on %s" % (plan.n, dev))
    shapes = {"attr": (32 * plan.slabs, 768), "frame_attr": (32 * plan.slabs,), "chan_attr": (plan.n, 768),
              "utt_total": (plan.n,)}
    out = {}
    for name in outputs:
        t = None if _out is None else _out.get(name)
        if t is None and _plan_only:
            out[name] = plan.lens_d          # any non-NULL device pointer: the host plan dereferences none
            continue
        if t is None:
            t = torch.empty(shapes[name], dtype=torch.float32, device=dev)
        elif t.dtype != torch.float32 or t.device != dev or not t.is_contiguous() or tuple(t.shape) != shapes[name]:
            raise ValueError("%s must be a contiguous float32 %s tensor on %s" % (name, list(shapes[name]), dev))
        out[name] = t
    fn = _lib.require("dad_attribution", "the attributions")
    b = _at_buffers(plan)
    a = _at_args(model, plan, dz, baseline, use_teacher, prec, out, b["counts_d"] if _counts is None else _counts)
    p = _at_plan(a)
    if _plan_only:
        return p
    if b["ws"] is None or b["ws"].numel() < p["workspace_bytes"]:
        b["ws"] = torch.empty(max(p["workspace_bytes"], 1), dtype=torch.uint8, device=dev)
    _lib.check(fn(a, _lib.ptr(b["ws"]), torch.cuda.current_stream(dev).cuda_stream), "dad_attribution")
    return out


def attribution_plan(model, plan, dz, baseline=None, use_teacher=False, precision="fp32", outputs=("frame_attr",)):
    """What enqueue_attribution would launch for these arguments, from the library's host plan (nothing is enqueued):
    {'mode': 'frame_only' | 'full', 'workspace_bytes' (the part of the workspace the call touches), 'launches',
    'kernel' (the slab kernel's instance)}."""
    return enqueue_attribution(model, plan, dz, baseline, use_teacher, precision, outputs, _plan_only=True)


def _read_at_counts(plan):
    b = _at_buffers(plan)
    b["counts_h"].copy_(b["counts_d"], non_blocking=True)
    torch.cuda.current_stream(plan.device).synchronize()
    c = b["counts_h"].numpy().copy()
    if c[_lib.AT_NONFINITE] > 0:
        raise _lib.DadError("dad_attribution: %d attribution element(s) are not finite (fp16: an operand beyond "
                            "+-65504; any precision: non-finite features, baseline or cotangents)"
                            % c[_lib.AT_NONFINITE])
    return {"frames": int(c[_lib.AT_FRAMES]), "n_nonfinite": int(c[_lib.AT_NONFINITE]),
            "n_crossing": int(c[_lib.AT_CROSS]), "n_lambda_one": int(c[_lib.AT_ONE])}


def _mean_frame(plan):
    """The split's mean frame [768] float32, on the device (float64 sums over the utterances' rows, in chunks)."""
    store, dev = plan.store, plan.device
    sizes = np.asarray(store.sizes, np.int64)
    offsets = np.asarray(store.offsets, np.int64)
    total = torch.zeros(768, dtype=torch.float64, device=dev)
    if int(sizes.sum()) == int(store.feats.shape[0]):
        for r in range(0, int(store.feats.shape[0]), 1 << 16):
            total += store.feats[r:r + (1 << 16)].sum(0, dtype=torch.float64)
    else:
        for o, L in zip(offsets, sizes):
            if L:
                total += store.feats[int(o):int(o + L)].sum(0, dtype=torch.float64)
    return (total / max(int(sizes.sum()), 1)).to(torch.float32).contiguous()


def _at_cotangent(plan, z, pred, target):
    """(target class [n] int64, dz [n, 4] float32) of `target` (integrated_gradients)."""
    pred = pred.to(torch.int64)
    if target == "label":
        if plan.labels_d is None:
            raise ValueError("the split has no labels: target='label' needs them (or use target='pred')")
        lab = plan.labels_d.to(torch.int64)
        tgt = torch.where((lab >= 0) & (lab < 4), lab, pred)
    elif isinstance(target, int):
        tgt = torch.full_like(pred, target)
    else:
        tgt = pred
    dz = torch.nn.functional.one_hot(tgt, 4).to(torch.float32)
    if target == "margin":
        other = z.masked_fill(dz.bool(), float("-inf")).argmax(1)
        dz = dz - torch.nn.functional.one_hot(other, 4).to(torch.float32)
    return tgt, dz.contiguous()


def integrated_gradients(model, store_or_loader, target="pred", baseline=None, use_teacher=False, precision="fp32",
                         outputs=("frame_attr", "chan_attr")):
    """Exact integrated gradients (Sundararajan et al. 2017) of every utterance of a split: which frames and which
    of the 768 channels carry F = dz . z, against a baseline frame.  target: 'pred' (the predicted class's logit),
    'label' (the label's where it lies in [0, 4), the prediction's otherwise), 'margin' (the predicted logit minus
    the runner-up: dz = e_c - e_c') or a class index; the cotangent is held fixed along the path, so log-probability
    or cross-entropy targets are out of scope.  baseline: None (zeros), 'mean' (the split's mean frame, computed on
    the device) or a float32 [768] device tensor.  One dad_eval_split for the logits, one dad_attribution.

    Returns the requested device tensors (enqueue_attribution's) plus 'utt_total' [n], 'target' [n], 'dz' [n, 4],
    'baseline' (None or the tensor used), 'completeness_gap' [n] float64 = utt_total - dz . (z(x) - z(x')) with
    z(x') = W2 ReLU(W1 x' + b1) + b2 in float64 on the device (0 for an utterance without frames), and the counts
    'frames', 'n_nonfinite', 'n_crossing', 'n_lambda_one'.  Raises DadError on a non-finite attribution element."""
    target = _at_check_target(target)
    outputs = _at_check_outputs(outputs)
    _at_check_baseline(baseline, True)
    model.eval()
    plan = EvalPlan.of(store_or_loader)
    lname, pname = ("t_logits", "t_pred") if use_teacher else ("logits", "pred")
    ev = enqueue_eval_split(model, plan, use_teacher, True, precision, (lname, pname))
    tgt, dz = _at_cotangent(plan, ev[lname], ev[pname], target)
    if isinstance(baseline, str):
        baseline = _mean_frame(plan)
    want = tuple(dict.fromkeys(outputs + ("utt_total",)))
    out = enqueue_attribution(model, plan, dz, baseline, use_teacher, precision, want)
    flat = (model.teacher_flat if use_teacher else model.student_flat).detach().to(torch.float64)
    W1, b1 = flat[:256 * 768].view(256, 768), flat[256 * 768:256 * 769]
    W2, b2 = flat[256 * 769:256 * 773].view(4, 256), flat[256 * 773:256 * 773 + 4]
    p0 = b1 if baseline is None else W1 @ baseline.to(torch.float64) + b1
    z0 = W2 @ torch.relu(p0) + b2
    gap = out["utt_total"].to(torch.float64) - (dz.to(torch.float64) * (ev[lname].to(torch.float64) - z0)).sum(1)
    gap = torch.where(plan.lens_d > 0, gap, torch.zeros_like(gap))
    res = _read_at_counts(plan)
    res.update(out)
    res.update(target=tgt, dz=dz, baseline=baseline, completeness_gap=gap)
    return res


def _saliency_of(model, split, target, baseline):
    """One model on one split (saliency_report): host summaries of integrated_gradients."""
    plan = EvalPlan.of(split)
    r = integrated_gradients(model, plan, target, baseline, outputs=("frame_attr", "chan_attr"))
    chan = r["chan_attr"].cpu().numpy().astype(np.float64)
    tgt = r["target"].cpu().numpy()
    fa = np.abs(r["frame_attr"].cpu().numpy().astype(np.float64))
    _, lens, slab_off = plan_host(plan.store.sizes, plan.store.offsets)
    profile, count = np.zeros((4, 768)), np.zeros(4, np.int64)
    np.add.at(profile, tgt, chan)
    np.add.at(count, tgt, 1)
    profile /= np.maximum(count, 1)[:, None]
    shares = []
    for i, L in enumerate(lens):
        v = np.sort(fa[32 * int(slab_off[i]):32 * int(slab_off[i]) + int(L)])[::-1]
        if L > 0 and v.sum() > 0:
            shares.append((int(np.searchsorted(np.cumsum(v), 0.5 * v.sum())) + 1) / float(L))
    return {"class_profile": profile, "class_count": count.tolist(),
            "temporal_concentration": float(np.mean(shares)) if shares else float("nan"),
            "max_completeness_gap": float(r["completeness_gap"].abs().max().item()),
            "n_crossing": r["n_crossing"], "frames": r["frames"], "_chan": chan, "_lens": np.asarray(lens)}


def _row_cosine(a, b):
    den = np.linalg.norm(a, axis=1) * np.linalg.norm(b, axis=1)
    ok = den > 0
    return float(((a[ok] * b[ok]).sum(1) / den[ok]).mean()) if ok.any() else float("nan")


def saliency_from_attributions(initial, trained):
    """The `initial_weights` / `trained_weights` / `change` block from two per-model dicts of saliency_report:
    the change of the temporal concentration per split, of the clean-noisy cosine, and the cosine between the initial
    and the trained class profile per split and class; every value a Python float or a list of them."""
    pub = lambda m: {k: ({kk: (vv.tolist() if isinstance(vv, np.ndarray) else vv) for kk, vv in v.items()
                          if not kk.startswith("_")} if isinstance(v, dict) else v) for k, v in m.items()}
    change = {}
    for s in ("clean", "noisy"):
        a, b = initial[s], trained[s]
        change[s] = {"temporal_concentration_change": b["temporal_concentration"] - a["temporal_concentration"],
                     "class_profile_cosine": [_row_cosine(a["class_profile"][c:c + 1], b["class_profile"][c:c + 1])
                                              for c in range(4)]}
    if initial["clean_noisy_cosine"] is not None and trained["clean_noisy_cosine"] is not None:
        change["clean_noisy_cosine_change"] = trained["clean_noisy_cosine"] - initial["clean_noisy_cosine"]
    return {"initial_weights": pub(initial), "trained_weights": pub(trained), "change": change}


def saliency_report(initial_model, trained_model, clean_split, noisy_split, target="pred", baseline=None):
    """Which channels and frames carry the decision, for the initial and the trained weights on a clean and a noisy
    split.  Per model and split: 'class_profile' [4][768] (the mean chan_attr per target class) and 'class_count',
    'temporal_concentration' (the smallest share of an utterance's frames that holds half of sum_t |frame_attr_t|,
    averaged over the utterances), 'max_completeness_gap'; per model 'clean_noisy_cosine' (the mean cosine between
    the clean and the noisy chan_attr rows) where the two splits have the same lengths utterance for utterance, None
    otherwise.  Host work on small tensors behind four integrated_gradients.  Returns saliency_from_attributions'
    block."""
    per = []
    for model in (initial_model, trained_model):
        c = _saliency_of(model, clean_split, target, baseline)
        n = _saliency_of(model, noisy_split, target, baseline)
        same = c["_lens"].shape == n["_lens"].shape and bool((c["_lens"] == n["_lens"]).all())
        per.append({"clean": c, "noisy": n, "clean_noisy_cosine": _row_cosine(c["_chan"], n["_chan"]) if same else None})
    return saliency_from_attributions(per[0], per[1])


# ------------------------------------------------------------------ rank a split by certainty
# DACP keeps a pseudo-label when the teacher's certainty score clears a per-class quantile threshold
# (I/utils.py:449-507).  dad_rank_metrics (csrc/rank.hip) puts the rows of a split in a total order by a key
# (descending, ties by row index, -0.0 == +0.0) and counts positives along it: the risk-coverage curve, ROC-AUC,
# average precision, what a threshold accepts, torch.quantile in the step's float32 arithmetic, reliability bins and
# the reference's confidence_stats (I/inference.py:361-369), every integer exact and every double bit-identical from
# call to call.

_RK_COLUMNS = _lib.RK_EVAL_COLUMNS


def _rank_buffers(n, m, Q, B, curves, device):
    """The buffers of one dad_rank_metrics call: 'block_d', one int64 tensor that holds counts [m][8] | values [m][8]
    (float64) | bin_counts [m][B][2] | bin_sum [m][B] (float64) | quant [m][Q] (float32) so that one copy returns all
    of it, its pinned host copy, thr, gammas, the curve tensors (curves) and the workspace."""
    need = int(_lib.require("dad_rank_workspace_bytes", "rank_metrics")(int(n), int(m)))
    if need == 0:
        raise ValueError("rank metrics take 1 <= n <= %d rows and 1 <= m <= %d columns, got n = %d, m = %d"
                         % (_lib.RK_MAX_N, _lib.RK_MAX_M, n, m))
    if not 0 <= Q <= _lib.RK_MAX_Q or not 0 <= B <= _lib.RK_MAX_BINS:
        raise ValueError("rank metrics take up to %d quantiles and %d bins" % (_lib.RK_MAX_Q, _lib.RK_MAX_BINS))
    off = np.cumsum([0, m * _lib.RK_COUNTS, m * _lib.RK_VALUES, m * B * 2, m * B, (m * Q + 1) // 2]).tolist()
    b = {"n": n, "m": m, "Q": Q, "B": B, "off": off,
         "block_d": torch.zeros(max(off[-1], 1), dtype=torch.int64, device=device),
         "block_h": torch.zeros(max(off[-1], 1), dtype=torch.int64).pin_memory(),
         "thr": torch.full((m,), float("nan"), dtype=torch.float32, device=device),
         "gammas": torch.zeros(max(Q, 1), dtype=torch.float32, device=device),
         "ws": torch.empty(need, dtype=torch.uint8, device=device)}
    if curves:
        b["order"] = torch.empty(m, n, dtype=torch.int32, device=device)
        b["cum_pos"] = torch.empty(m, n, dtype=torch.int32, device=device)
        b["tie_end"] = torch.empty(m, n, dtype=torch.uint8, device=device)
    return b


def _enqueue_rank(key, flags, b, bin_range=(0.0, 1.0), chunks=0):
    """dad_rank_metrics on the current stream, enqueue only; chunks > 0: dad_rank_metrics_chunked."""
    a = _lib.DadRankArgs()
    base, off = b["block_d"].data_ptr(), b["off"]
    a.key, a.flags, a.thr = key.data_ptr(), flags.data_ptr(), b["thr"].data_ptr()
    a.gammas = b["gammas"].data_ptr() if b["Q"] else None
    for name in ("order", "cum_pos", "tie_end"):
        setattr(a, name, b[name].data_ptr() if name in b else None)
    a.counts, a.values = base + 8 * off[0], base + 8 * off[1]
    a.bin_counts, a.bin_sum = (base + 8 * off[2], base + 8 * off[3]) if b["B"] else (None, None)
    a.quant = base + 8 * off[4] if b["Q"] else None
    a.n, a.m, a.Q, a.B = b["n"], b["m"], b["Q"], b["B"]
    a.bin_lo, a.bin_hi = float(bin_range[0]), float(bin_range[1])
    stream = torch.cuda.current_stream(key.device).cuda_stream
    if chunks:
        rc = _lib.require("dad_rank_metrics_chunked", "rank_metrics")(a, int(chunks), _lib.ptr(b["ws"]), stream)
    else:
        rc = _lib.require("dad_rank_metrics", "rank_metrics")(a, _lib.ptr(b["ws"]), stream)
    _lib.check(rc, "dad_rank_metrics")


def _rank_blocks(b, host):
    """{'counts' [m][8] int64, 'values' [m][8] float64, 'bin_counts' [m][B][2], 'bin_sum' [m][B], 'quant' [m][Q]
    float32} from the host copy of a call's block."""
    m, Q, B, off = b["m"], b["Q"], b["B"], b["off"]
    return {"counts": host[off[0]:off[1]].reshape(m, _lib.RK_COUNTS).copy(),
            "values": host[off[1]:off[2]].view(np.float64).reshape(m, _lib.RK_VALUES).copy(),
            "bin_counts": host[off[2]:off[3]].reshape(m, B, 2).copy(),
            "bin_sum": host[off[3]:off[4]].view(np.float64).reshape(m, B).copy(),
            "quant": host[off[4]:off[5]].view(np.float32)[:m * Q].reshape(m, Q).copy()}


def _rank_columns(blocks, b=None):
    """One dict per column from _rank_blocks; with the buffers b of a curves call the column's device rows too."""
    cols = []
    for j in range(len(blocks["counts"])):
        c, v = blocks["counts"][j], blocks["values"][j]
        col = {"members": int(c[_lib.RK_MEMBERS]), "positives": int(c[_lib.RK_POSITIVES]),
               "nonfinite": int(c[_lib.RK_NONFINITE]), "runs": int(c[_lib.RK_RUNS]), "u2": int(c[_lib.RK_U2]),
               "accepted": int(c[_lib.RK_ACCEPTED]), "accepted_positives": int(c[_lib.RK_ACCEPTED_POS]),
               "auroc_valid": bool(c[_lib.RK_VALID_AUROC]), "auroc": float(v[_lib.RK_AUROC]),
               "average_precision": float(v[_lib.RK_AP]), "aurc": float(v[_lib.RK_AURC]),
               "key_mean": float(v[_lib.RK_KEY_MEAN]), "key_std": float(v[_lib.RK_KEY_STD]),
               "key_min": float(v[_lib.RK_KEY_MIN]), "key_max": float(v[_lib.RK_KEY_MAX]),
               "quantiles": blocks["quant"][j].copy(), "bin_counts": blocks["bin_counts"][j, :, 0].copy(),
               "bin_positives": blocks["bin_counts"][j, :, 1].copy(), "bin_key_sum": blocks["bin_sum"][j].copy()}
        if b is not None and "order" in b:
            col.update(order=b["order"][j], cum_pos=b["cum_pos"][j], tie_end=b["tie_end"][j])
        cols.append(col)
    return cols


def _read_rank(b, device):
    b["block_h"].copy_(b["block_d"], non_blocking=True)
    torch.cuda.current_stream(device).synchronize()
    return _rank_blocks(b, b["block_h"].numpy().copy())


def rank_metrics(keys, member, positive, thresholds=None, quantiles=(), bins=0, bin_range=(0.0, 1.0), curves=False,
                 _chunks=0):
    """dad_rank_metrics for columns of your own: keys [m, n] (or [n]) float32 on the device, member / positive boolean
    [m, n] (or [n], shared by the columns), thresholds [m] (None: no threshold), quantiles up to 8 gammas, bins up to
    64 over bin_range.  A row takes part in a column when it is a member with a finite key; the order is (key
    descending, row index ascending).  Returns one dict per column: 'members', 'positives', 'nonfinite', 'runs', 'u2'
    (the Mann-Whitney count), 'accepted' / 'accepted_positives' (key >= threshold), 'auroc_valid', 'auroc',
    'average_precision', 'aurc', 'key_mean' / 'key_std' / 'key_min' / 'key_max', 'quantiles' [Q] (torch.quantile in
    float32), 'bin_counts' / 'bin_positives' / 'bin_key_sum' [bins].  curves=True adds the device tensors 'order',
    'cum_pos' and 'tie_end' [n] of the column, which risk_coverage(col) and roc_points(col) read at the tie ends."""
    if not torch.is_tensor(keys) or not keys.is_cuda or keys.dtype != torch.float32 or keys.dim() not in (1, 2):
        raise ValueError("keys must be a float32 device tensor [m, n] or [n]")
    keys = keys.reshape(-1, keys.shape[-1]).contiguous()
    m, n = keys.shape
    dev = keys.device
    flag = lambda t: torch.as_tensor(t).to(device=dev).to(torch.bool).expand(m, n)
    flags = (flag(member).to(torch.uint8) * _lib.RK_MEMBER
             + flag(positive).to(torch.uint8) * _lib.RK_POSITIVE).contiguous()
    quantiles = [float(q) for q in quantiles]
    b = _rank_buffers(n, m, len(quantiles), int(bins), curves, dev)
    if thresholds is not None:
        thr = torch.as_tensor(thresholds, dtype=torch.float32).reshape(-1)
        if thr.shape != (m,):
            raise ValueError("thresholds must be [m]")
        b["thr"].copy_(thr)
    if quantiles:
        b["gammas"].copy_(torch.tensor(quantiles, dtype=torch.float32))
    _enqueue_rank(keys, flags, b, bin_range, _chunks)
    return _rank_columns(_read_rank(b, dev), b)


def risk_coverage(col):
    """(coverage, risk) of a rank_metrics(curves=True) column at its tie ends, as float64 NumPy arrays: accepting the
    k most certain rows covers k / M of the members with (k - positives among them) / k wrong."""
    M = col["members"]
    tie = col["tie_end"][:M].cpu().numpy().astype(bool)
    taken = (np.nonzero(tie)[0] + 1).astype(np.float64)
    return taken / max(M, 1), (taken - col["cum_pos"][:M].cpu().numpy()[tie]) / taken


def roc_points(col):
    """(false-positive rate, true-positive rate) of a rank_metrics(curves=True) column at its tie ends."""
    M, P = col["members"], col["positives"]
    tie = col["tie_end"][:M].cpu().numpy().astype(bool)
    tp = col["cum_pos"][:M].cpu().numpy()[tie].astype(np.float64)
    return (np.nonzero(tie)[0] + 1 - tp) / max(M - P, 1), tp / max(P, 1)


def _ranking_buffers(plan, Q, B):
    cache = plan.__dict__.setdefault("_rank", {})
    b = cache.get((Q, B))
    if b is None:
        b = _rank_buffers(plan.n, _RK_COLUMNS, Q, B, False, plan.device)
        b["key"] = torch.empty(_RK_COLUMNS, plan.n, dtype=torch.float32, device=plan.device)
        b["flags"] = torch.empty(_RK_COLUMNS, plan.n, dtype=torch.uint8, device=plan.device)
        cache[(Q, B)] = b
    return b


def _ranking_quantiles(quantiles, cfg):
    if quantiles is None:
        from .config import ConfigView
        view = ConfigView(flavor="iemocap") if cfg is None else cfg
        return [float(view.DACP_QUANTILE_START), float(view.DACP_QUANTILE_END)]
    return [float(q) for q in quantiles]


def enqueue_certainty_ranking(model, plan, use_teacher=False, thresholds=None, quantiles=None, bins=20,
                              precision="fp32", cfg=None, outputs=()):
    """The enqueue part of certainty_ranking_store (no copy to the host, no synchronisation): one dad_eval_split, with
    use_teacher dad_predict_head on its t_emb for the teacher's probabilities and score, then dad_rank_eval_columns and
    dad_rank_metrics behind it on the current stream.  Returns (buffers, {name: device tensor}) with 'score', 'probs',
    'pred' (the ranked model's) and the further `outputs` of dad_eval_split; the block lands in buffers['block_d']."""
    gam = _ranking_quantiles(quantiles, cfg)
    b = _ranking_buffers(plan, len(gam), int(bins))
    names = set(outputs) | ({"t_emb"} if use_teacher else {"score", "probs", "pred"})
    out = enqueue_eval_split(model, plan, use_teacher=use_teacher, precision=precision, outputs=tuple(sorted(names)))
    stream = torch.cuda.current_stream(plan.device).cuda_stream
    if use_teacher:
        cls = model.teacher_classifier
        w2, b2 = cls.fc_layer.weight.detach().contiguous(), cls.fc_layer.bias.detach().contiguous()
        head = {"probs": torch.empty(plan.n, 4, device=plan.device), "score": torch.empty(plan.n, device=plan.device),
                "pred": torch.empty(plan.n, dtype=torch.int64, device=plan.device)}
        _lib.check(_lib.lib().dad_predict_head(_lib.ptr(out["t_emb"]), plan.n, _lib.ptr(w2), _lib.ptr(b2), 1, None,
                                               _lib.ptr(head["probs"]), _lib.ptr(head["score"]),
                                               _lib.ptr(head["pred"]), stream), "dad_predict_head")
        out.update(head)
    b["thr"].fill_(float("nan"))
    if thresholds is not None:
        thr = torch.as_tensor(thresholds).detach().to(device=plan.device, dtype=torch.float32).reshape(-1)
        if thr.shape != (4,):
            raise ValueError("thresholds must be [4]")
        b["thr"][1:5].copy_(thr)
    if gam:
        b["gammas"].copy_(torch.tensor(gam, dtype=torch.float32), non_blocking=False)
    _lib.check(_lib.require("dad_rank_eval_columns", "certainty ranking")(
        _lib.ptr(out["score"]), _lib.ptr(out["probs"]), _lib.ptr(out["pred"]), _lib.ptr(plan.labels_d), plan.n,
        _lib.ptr(b["key"]), _lib.ptr(b["flags"]), stream), "dad_rank_eval_columns")
    _enqueue_rank(b["key"], b["flags"], b)
    return b, out


def _ratio(a, d):
    return float(a) / float(d) if d else 0.0


def _certainty_result(cols, gam, bins):
    """certainty_ranking_store's dict from the ten columns of dad_rank_eval_columns."""
    sel = lambda c: {"aurc": c["aurc"], "auroc": c["auroc"], "auroc_valid": c["auroc_valid"],
                     "accuracy": _ratio(c["positives"], c["members"]), "n": c["members"]}
    gate = []
    for c in cols[1:5]:
        M, P, A, AP = c["members"], c["positives"], c["accepted"], c["accepted_positives"]
        wrong = M - P
        gate.append({"members": M, "passed": A, "passed_right": AP, "passed_wrong": A - AP, "blocked_right": P - AP,
                     "blocked_wrong": wrong - (A - AP), "purity": _ratio(AP, A), "coverage": _ratio(A, M),
                     "leak": _ratio(A - AP, wrong)})
    ovr = cols[6:10]
    conf = cols[5]
    edges = np.linspace(0.0, 1.0, bins + 1) if bins else np.zeros(0)
    rel = {"edges": edges.tolist(), "count": conf["bin_counts"].tolist(),
           "accuracy": [_ratio(p, k) for p, k in zip(conf["bin_positives"], conf["bin_counts"])],
           "confidence": [_ratio(s, k) for s, k in zip(conf["bin_key_sum"], conf["bin_counts"])]}
    n = max(conf["members"], 1)
    rel["ece"] = float(sum(k / n * abs(a - c) for k, a, c in zip(rel["count"], rel["accuracy"], rel["confidence"])))
    return {
        "selective": {"overall": sel(cols[0]), "per_class": [sel(c) for c in cols[1:5]],
                      "max_probability": sel(cols[5])},
        "ovr": {"auroc_per_class": [c["auroc"] for c in ovr], "ap_per_class": [c["average_precision"] for c in ovr],
                "auroc_macro": float(np.mean([c["auroc"] for c in ovr])),
                "ap_macro": float(np.mean([c["average_precision"] for c in ovr])),
                "valid": all(c["auroc_valid"] for c in ovr)},
        "confidence_stats": {"mean_confidence": conf["key_mean"], "std_confidence": conf["key_std"],
                             "min_confidence": conf["key_min"], "max_confidence": conf["key_max"]},
        "gate": gate,
        "quantiles": list(gam),
        "quantile_thresholds": np.stack([c["quantiles"] for c in cols[1:5]]),
        "reliability": rel,
        "columns": cols,
    }


def certainty_ranking_store(model, store_or_loader, use_teacher=False, thresholds=None, quantiles=None, bins=20,
                            precision="fp32", cfg=None, outputs=()):
    """How good the score that gates training is, over a whole split: one dad_eval_split, dad_rank_eval_columns and
    dad_rank_metrics on the stream, one copy back.  With use_teacher the teacher is ranked (its probabilities and
    score from dad_predict_head on t_emb).  quantiles None: DACP_QUANTILE_START and DACP_QUANTILE_END of the config.
    thresholds [4] (DADStep.ema_thresholds, the calibrated anchors): applied per predicted class, score >= tau
    (I/utils.py:501).  Returns
      'selective'  overall / per predicted class / by max probability: AURC, the AUROC of the score as a detector of
                   correct predictions, the accuracy at full coverage
      'ovr'        per-class one-vs-rest AUROC and AP, their macro means (roc_auc_score(y, probs, multi_class='ovr'))
      'confidence_stats'  the reference's four keys (I/inference.py:361-369), of the max probability
      'gate'       per class: members, passed, passed_right, passed_wrong, blocked_right, blocked_wrong, purity,
                   coverage, leak = wrong passed / wrong
      'quantile_thresholds' [4][Q]  torch.quantile(class scores, gamma) of I/utils.py:477-481 on the whole split
      'reliability'  the bins of the max probability: edges, count, accuracy, confidence, ece
      'columns'    the ten raw columns, plus a device tensor per name in `outputs` and 'score', 'probs', 'pred'.
    An unlabelled split gives the quantiles and the gate's passed counts; what needs labels is 0."""
    model.eval()
    plan = EvalPlan.of(store_or_loader)
    b, out = enqueue_certainty_ranking(model, plan, use_teacher, thresholds, quantiles, bins, precision, cfg, outputs)
    b["block_h"].copy_(b["block_d"], non_blocking=True)
    _read_eval_block(plan, {})        # (synchronises the stream; raises on a non-finite logit)
    cols = _rank_columns(_rank_blocks(b, b["block_h"].numpy().copy()))
    res = _certainty_result(cols, _ranking_quantiles(quantiles, cfg), int(bins))
    res.update(out)
    return res


def _firewall_of(model, split, thresholds):
    r = certainty_ranking_store(model, split, use_teacher=True, thresholds=thresholds)
    g = r["gate"]
    tot = lambda k: sum(c[k] for c in g)
    wrong = tot("passed_wrong") + tot("blocked_wrong")
    return {"passed": float(tot("passed")), "passed_wrong": float(tot("passed_wrong")),
            "coverage": _ratio(tot("passed"), tot("members")), "purity": _ratio(tot("passed_right"), tot("passed")),
            "leak": _ratio(tot("passed_wrong"), wrong), "teacher_aurc": r["selective"]["overall"]["aurc"],
            "teacher_auroc": r["selective"]["overall"]["auroc"],
            "purity_per_class": [c["purity"] for c in g], "coverage_per_class": [c["coverage"] for c in g],
            "leak_per_class": [c["leak"] for c in g], "gate": g}


def _house_report(initial, trained, keys):
    pick = lambda r: {k: r[k] for k in r if k != "gate"}
    return {"initial_weights": pick(initial), "trained_weights": pick(trained),
            "improvement": {k + "_change": float(trained[k] - initial[k]) for k in keys}}


def firewall_report(model, noisy_split, thresholds, initial_model=None):
    """The pseudo-label firewall split-wide: the teacher on the noisy split at the thresholds tau [4] -- how many
    pseudo-labels pass the gate, how pure they are and which share of the wrong ones leaks through (the confirmation
    bias analyze_confirmation_bias.py follows on 50 tracked samples).  `model` is the trained model; initial_model
    (None: the same model, so every change is 0) gives the `initial_weights` block.  Every value a Python float or a
    list of them; 'gate' (the per-class integer counts of the trained model) rides along at the top level."""
    trained = _firewall_of(model, noisy_split, thresholds)
    initial = trained if initial_model is None else _firewall_of(initial_model, noisy_split, thresholds)
    rep = _house_report(initial, trained, ("coverage", "purity", "leak", "teacher_aurc", "teacher_auroc"))
    rep["gate"] = trained["gate"]
    return rep


def _reliability_of(model, clean_split, noisy_split):
    res = {}
    for name, split in (("clean", clean_split), ("noisy", noisy_split)):
        r = certainty_ranking_store(model, split)
        res.update({name + "_aurc": r["selective"]["overall"]["aurc"],
                    name + "_auroc": r["selective"]["overall"]["auroc"],
                    name + "_ece": r["reliability"]["ece"], name + "_auroc_ovr_macro": r["ovr"]["auroc_macro"],
                    name + "_mean_confidence": r["confidence_stats"]["mean_confidence"]})
    return res


def reliability_report(initial_model, trained_model, clean_split, noisy_split):
    """Whether the student's certainty can be trusted, for the initial and the trained weights on a clean and a noisy
    split: AURC, the AUROC of the score as a detector of correct predictions, the expected calibration error of the max
    probability, the macro one-vs-rest AUROC and the mean confidence, in the house format."""
    a = _reliability_of(initial_model, clean_split, noisy_split)
    b = _reliability_of(trained_model, clean_split, noisy_split)
    return _house_report(a, b, tuple(a))


# ------------------------------------------------------------------ several networks on one split
# The reference compares networks on the same split everywhere around its train step (fold checkpoints, ablation
# runners, inference.py, student / teacher).  dad_eval_models (csrc/eval_models.hip) evaluates up to 8 of them in
# one pass over the store and builds what a comparison reads on the device: per-member confusion matrices (the K
# models, their mean ensemble, their vote), pairwise disagreement and McNemar cells, the correct-count histogram
# and the float64 sums behind mean NLL, Brier score and entropy.  Definitions: include/dad.h, "several networks on
# one split".

_MODELS_OUTPUTS = {"emb": ((256,), torch.float32), "logits": ((4,), torch.float32), "probs": ((4,), torch.float32),
                   "score": ((), torch.float32), "pred": ((), torch.int64)}
_MODELS_UTT_OUTPUTS = {"ens_probs": ((4,), torch.float32), "ens_score": ((), torch.float32),
                       "ens_pred": ((), torch.int64), "vote_pred": ((), torch.int64), "votes": ((4,), torch.int32),
                       "n_correct": ((), torch.int32)}
_MODELS_WORDS = _lib.EM_COUNTS + _lib.EM_SUMS


def _models_buffers(plan):
    """The buffers of dad_eval_models over this split, kept on the plan beside the noise buffers: {'result_d' /
    'result_h' the DAD_EM_* block (counts, then sums) and its pinned host copy, 'ws' the workspace, 'scratch' the
    model that checkpoint paths are loaded into, 'flats' the device copies of their weights}."""
    b = plan._noise.get("models")
    if b is None:
        b = {"result_d": torch.zeros(_MODELS_WORDS, dtype=torch.int64, device=plan.device),
             "result_h": torch.zeros(_MODELS_WORDS, dtype=torch.int64).pin_memory(), "ws": None, "scratch": None,
             "flats": {}}
        plan._noise["models"] = b
    return b


def _model_flats(models, plan):
    """The flat [W1|b1|W2|b2] device tensor of every entry of `models`: an SSRLModel (its student), a (model,
    'student' | 'teacher') pair, a flat float32 device tensor, or a checkpoint path (loaded with
    checkpoint.load_checkpoint into a scratch model; its student weights are copied to a tensor kept on the plan)."""
    from .model import SSRLModel
    models = list(models)
    if not 1 <= len(models) <= _lib.EM_MAX_MODELS:
        raise ValueError("between 1 and %d models, got %d" % (_lib.EM_MAX_MODELS, len(models)))
    nparam = int(_lib.lib().dad_param_count())
    flats = []
    for i, m in enumerate(models):
        if isinstance(m, tuple):
            mod, role = m
            if role not in ("student", "teacher"):
                raise ValueError("models[%d]: the role is 'student' or 'teacher', got %r" % (i, role))
            f = mod.teacher_flat if role == "teacher" else mod.student_flat
        elif isinstance(m, torch.Tensor):
            f = m
        elif isinstance(m, (str, bytes)) or hasattr(m, "__fspath__"):
            from . import checkpoint
            b = _models_buffers(plan)
            if b["scratch"] is None:
                b["scratch"] = SSRLModel().to(plan.device)
            checkpoint.load_checkpoint(m, b["scratch"])
            f = b["flats"].setdefault(i, torch.empty(nparam, dtype=torch.float32, device=plan.device))
            f.copy_(b["scratch"].student_flat.detach())
        elif hasattr(m, "student_flat"):
            f = m.student_flat
        else:
            raise TypeError("models[%d]: an SSRLModel, a (model, role) pair, a flat tensor or a checkpoint path, got %s"
                            % (i, type(m).__name__))
        f = f.detach()
        if (f.dtype != torch.float32 or f.device != plan.device or not f.is_contiguous() or f.numel() != nparam):
            raise ValueError("models[%d]: a contiguous float32 tensor of %d parameters on %s is needed"
                             % (i, nparam, plan.device))
        flats.append(f)
    return flats


def _models_weights(weights, K):
    w = [1.0] * K if weights is None else [float(v) for v in np.asarray(weights, dtype=np.float64).reshape(-1)]
    if len(w) != K:
        raise ValueError("%d weights for %d models" % (len(w), K))
    if any(not np.isfinite(v) or v < 0 for v in w) or not sum(w) > 0:
        raise ValueError("ensemble weights must be finite, >= 0 and not all zero, got %r" % (w,))
    return w


def enqueue_eval_models(models, plan, weights=None, use_entropy=True, precision="fp32", outputs=(), _block=None):
    """dad_eval_models on the current stream, enqueue only (no copy, no synchronisation): `models` (1 to 8 entries,
    _model_flats' forms; the same network may appear twice) over the plan's split, `weights` the ensemble weights
    (None: equal).  The DAD_EM_* block lands in the plan's buffer (or in _block, an int64 device tensor of EM_COUNTS
    + EM_SUMS words).  Returns the {name: device tensor} of the requested outputs: 'emb', 'logits', 'probs', 'score',
    'pred' ([K, n, ...], model-major, each model's dad_eval_split outputs bit for bit) and 'ens_probs' [n, 4],
    'ens_score', 'ens_pred', 'vote_pred' [n], 'votes' [n, 4] int32, 'n_correct' [n] int32 (-1 unlabelled)."""
    prec = _PRECISIONS[precision] if isinstance(precision, str) else int(precision)
    dev = plan.device
    flats = _model_flats(models, plan)
    K = len(flats)
    w = _models_weights(weights, K)
    out = {}
    for name in outputs:
        if name in _MODELS_OUTPUTS:
            shape, dt = _MODELS_OUTPUTS[name]
            out[name] = torch.empty((K, plan.n) + shape, dtype=dt, device=dev)
        elif name in _MODELS_UTT_OUTPUTS:
            shape, dt = _MODELS_UTT_OUTPUTS[name]
            out[name] = torch.empty((plan.n,) + shape, dtype=dt, device=dev)
        else:
            raise ValueError("unknown output %r (one of %s)" % (name, ", ".join(list(_MODELS_OUTPUTS)
                                                                              + list(_MODELS_UTT_OUTPUTS))))
    fn = _lib.require("dad_eval_models", "the multi-checkpoint evaluator")
    b = _models_buffers(plan)
    need = int(_lib.require("dad_eval_models_workspace_bytes", "the multi-checkpoint evaluator")(
        plan.n, plan.slabs, K, prec))
    if b["ws"] is None or b["ws"].numel() < need:
        b["ws"] = torch.empty(max(need, 1), dtype=torch.uint8, device=dev)
    block = b["result_d"] if _block is None else _block
    store = plan.store
    a = _lib.DadModelsArgs()
    a.store = store.feats.data_ptr()
    a.rows, a.lens, a.slab_off = plan.rows_d.data_ptr(), plan.lens_d.data_ptr(), plan.slab_off_d.data_ptr()
    a.labels = None if plan.labels_d is None else plan.labels_d.data_ptr()
    a.n, a.slabs = plan.n, plan.slabs
    a.store_dtype = STORE_DTYPES[store.feats.dtype]
    a.use_entropy = int(bool(use_entropy))
    a.precision = prec
    for k, f in enumerate(flats):
        a.models[k] = f.data_ptr()
        a.weight[k] = w[k]
    a.K = K
    for name, t in out.items():
        setattr(a, name, t.data_ptr() or None)
    a.counts = block.data_ptr()
    a.sums = block.data_ptr() + 8 * _lib.EM_COUNTS
    _lib.check(fn(a, _lib.ptr(b["ws"]), torch.cuda.current_stream(dev).cuda_stream), "dad_eval_models")
    b["live"] = flats              # (keeps the weights alive until the next call on this plan)
    return out


def _models_block(host, weights):
    """The dict of evaluate_models_store from the host copy of the DAD_EM_* block."""
    counts = host[:_lib.EM_COUNTS]
    sums = host[_lib.EM_COUNTS:].view(np.float64).reshape(4, _lib.EM_MEMBERS)
    K, M = int(counts[_lib.EM_K]), _lib.EM_MEMBERS
    sq = lambda o: counts[o:o + M * M].reshape(M, M)[:K + 2, :K + 2].copy()
    return {"K": K, "n": int(counts[_lib.EM_N]), "n_labelled": int(counts[_lib.EM_N_LABELLED]),
            "n_skipped": int(counts[_lib.EM_N_SKIPPED]),
            "nonfinite": counts[_lib.EM_NONFINITE:_lib.EM_NONFINITE + K].copy(),
            "confusion": counts[_lib.EM_CONF:_lib.EM_CONF + 16 * M].reshape(M, 4, 4)[:K + 2].copy(),
            "disagree": sq(_lib.EM_DISAGREE), "only": sq(_lib.EM_ONLY),
            "hist": counts[_lib.EM_HIST:_lib.EM_HIST + K + 1].copy(),
            "sum_score": sums[0, :K + 1].copy(), "sum_entropy": sums[1, :K + 1].copy(),
            "sum_nll": sums[2, :K + 1].copy(), "sum_brier": sums[3, :K + 1].copy(),
            "weights": list(weights), "block": host}


def evaluate_models_store(models, plan_or_store, weights=None, use_entropy=True, precision="fp32", outputs=()):
    """One dad_eval_models over the whole split and one device-to-host copy of its result block.  Members are the K
    models, then their mean ensemble (index K), then their vote (index K + 1).  Returns {'K', 'n', 'n_labelled',
    'n_skipped', 'nonfinite' [K], 'confusion' [K + 2, 4, 4] (row = label), 'disagree' [K + 2, K + 2] (pred_a != pred_b
    over all n), 'only' [K + 2, K + 2] (a right and b wrong; the diagonal is a's correct count), 'hist' [K + 1]
    (labelled utterances by how many models are right), 'sum_score', 'sum_entropy', 'sum_nll', 'sum_brier' [K + 1]
    (float64; models, then the ensemble), 'weights', 'block'} as NumPy values, plus a device tensor per name in
    `outputs` (enqueue_eval_models).  Raises DadError when any model has a non-finite logit."""
    plan = EvalPlan.of(plan_or_store)
    models = list(models)
    out = enqueue_eval_models(models, plan, weights, use_entropy, precision, outputs)
    K = len(models)
    b = _models_buffers(plan)
    b["result_h"].copy_(b["result_d"], non_blocking=True)
    torch.cuda.current_stream(plan.device).synchronize()
    res = _models_block(b["result_h"].numpy().copy(), _models_weights(weights, K))
    if res["nonfinite"].any():
        raise _lib.DadError("dad_eval_models: model(s) %s have a non-finite logit on %s of %d utterance(s) (fp16: an "
                            "operand beyond +-65504; any precision: non-finite features)"
                            % (np.nonzero(res["nonfinite"])[0].tolist(),
                               res["nonfinite"][res["nonfinite"] > 0].tolist(), res["n"]))
    res.update(out)
    return res


def mcnemar_exact(b, c):
    """The exact two-sided binomial p-value of McNemar's test for the discordant counts b and c: the probability,
    under Binomial(b + c, 1/2), of a split at least as uneven, min(1, 2 P[X <= min(b, c)]); 1.0 when b + c = 0."""
    b, c = int(b), int(c)
    n, k = b + c, min(b, c)
    if n == 0:
        return 1.0
    tail = sum(math.comb(n, i) for i in range(k + 1))
    return min(1.0, 2 * tail / (1 << n))          # (exact integers; the quotient is rounded once)


def ensemble_from_block(res):
    """ensemble_report's dict from evaluate_models_store's (every value a Python or NumPy host value)."""
    K, n, nl = res["K"], res["n"], res["n_labelled"]
    names = ["model_%d" % k for k in range(K)] + ["ensemble", "vote"]
    w = np.asarray(res["weights"], np.float64)
    wn = (w / w.sum()).astype(np.float32).astype(np.float64)
    members = []
    for m, name in enumerate(names):
        d = {"name": name}
        if nl:
            d.update(metrics_from_confusion(res["confusion"][m]))
        if m <= K:
            d["mean_score"] = res["sum_score"][m] / n
            d["mean_entropy"] = res["sum_entropy"][m] / n
            if nl:
                d["nll"] = res["sum_nll"][m] / nl
                d["brier"] = res["sum_brier"][m] / nl
        members.append(d)
    pairs = []
    for a in range(K + 2):
        for b in range(a + 1, K + 2):
            pb, pc = int(res["only"][a, b]), int(res["only"][b, a])
            pairs.append({"a": names[a], "b": names[b], "disagreement_rate": res["disagree"][a, b] / n,
                          "mcnemar_b": pb, "mcnemar_c": pc, "p_value": mcnemar_exact(pb, pc)})
    rep = {"members": members, "pairs": pairs, "hist": res["hist"].tolist(),
           "diversity": float(res["sum_entropy"][K] / n - np.dot(wn, res["sum_entropy"][:K]) / n),
           "n": n, "n_labelled": nl, "K": K}
    if nl:
        rep["oracle_accuracy"] = float(res["hist"][1:].sum() / nl) * 100
        rep["best_single"] = max(range(K), key=lambda k: members[k]["weighted_accuracy"])
    return rep


def ensemble_report(models, store_or_loader, weights=None, precision="fp32"):
    """K networks compared on one split from one dad_eval_models: {'members': per member ('model_k', 'ensemble',
    'vote') metrics_from_confusion's dict plus 'mean_score', 'mean_entropy', 'nll' (mean -ln p_y) and 'brier' (the
    vote has no probabilities); 'pairs': per pair a < b the 'disagreement_rate', McNemar's 'mcnemar_b' (a right, b
    wrong) and 'mcnemar_c', and the exact two-sided binomial 'p_value'; 'oracle_accuracy' (per cent of labelled
    utterances that at least one model gets right); 'hist' (labelled utterances by how many models are right);
    'diversity' (mean H(ensemble) - sum_k w^_k mean H(p_k) in nats, the generalised Jensen-Shannon divergence of the
    models' predictions); 'best_single' (the model with the highest weighted accuracy)}."""
    return ensemble_from_block(evaluate_models_store(models, store_or_loader, weights, True, precision))
