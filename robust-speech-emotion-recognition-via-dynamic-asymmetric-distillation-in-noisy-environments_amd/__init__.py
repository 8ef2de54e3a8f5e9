"""MI355X-native DAD (Dynamic Asymmetric Distillation) train step.

Drop-in for the hot path of the reference's DAD-train-{IEMOCAP,CASIA,EMODB} trainers:
`SSRLModel` (I/model.py) and the train_epoch loop body (I/train.py:484-492), backed by
hand-written HIP kernels for gfx950 behind the C ABI in include/dad.h (libdad_hip.so).

The package directory name is not a Python identifier; it is importable with
`importlib.import_module(...)` and registers the alias `dad_amd` on import.
"""
import sys as _sys

from . import _build, _lib
from .config import FLAVOR_DEFAULTS, ConfigView, dad_config_for
from .model import EmotionClassifier, Emotion2VecEncoder, SSRLModel
from .step import DADStep
from .dist import DPComm, ProcessGroupComm
from .data import DeviceLoader, FeatureStore
from .utils import DACPManager, DataAugmentation, ECDALoss, SupervisedContrastiveLoss
from .trace import TrainingTrace
from . import checkpoint, evaluate, pretrain
from .evaluate import cluster_metrics, cluster_metrics_store, separation_report
from .evaluate import tsne, tsne_affinities, tsne_gradient, tsne_report, tsne_store
from .evaluate import alignment_report, domain_gap, domain_gap_store, enqueue_domain_gap_store
from .evaluate import (cross_domain_knn_store, knn, knn_accuracy, knn_store, neighbourhood_report,
                       trustworthiness)
from .evaluate import (duration_report, early_decision_curve, enqueue_eval_windows, evaluate_windows_store,
                       window_frames, windows, windows_host)
from .evaluate import (enqueue_eval_noise, evaluate_noise_store, noise_draws, noise_response_curve,
                       robustness_report)
from .evaluate import (adversarial_response_curve, enqueue_input_grad, evaluate_adversarial_store, input_gradients,
                       worst_case_report)
from .evaluate import (attribution_plan, enqueue_attribution, integrated_gradients, saliency_from_attributions,
                       saliency_report)
from .evaluate import (certainty_ranking_store, enqueue_certainty_ranking, firewall_report, rank_metrics,
                       reliability_report, risk_coverage, roc_points)
from .evaluate import enqueue_eval_models, ensemble_report, evaluate_models_store

__all__ = ["SSRLModel", "Emotion2VecEncoder", "EmotionClassifier", "DADStep", "DPComm", "ProcessGroupComm", "ConfigView",
           "dad_config_for", "FLAVOR_DEFAULTS", "FeatureStore", "DeviceLoader", "DataAugmentation", "DACPManager", "ECDALoss", "SupervisedContrastiveLoss", "TrainingTrace",
           "cluster_metrics", "cluster_metrics_store", "separation_report",
           "tsne", "tsne_affinities", "tsne_gradient", "tsne_store", "tsne_report",
           "domain_gap", "domain_gap_store", "enqueue_domain_gap_store", "alignment_report",
           "knn", "knn_accuracy", "knn_store", "cross_domain_knn_store", "trustworthiness", "neighbourhood_report",
           "windows", "windows_host", "window_frames", "enqueue_eval_windows", "evaluate_windows_store",
           "early_decision_curve", "duration_report",
           "noise_draws", "enqueue_eval_noise", "evaluate_noise_store", "noise_response_curve", "robustness_report",
           "enqueue_input_grad", "input_gradients", "evaluate_adversarial_store", "adversarial_response_curve",
           "worst_case_report",
           "enqueue_attribution", "attribution_plan", "integrated_gradients", "saliency_report",
           "saliency_from_attributions",
           "rank_metrics", "risk_coverage", "roc_points", "enqueue_certainty_ranking", "certainty_ranking_store",
           "firewall_report", "reliability_report",
           "enqueue_eval_models", "evaluate_models_store", "ensemble_report",
           "build", "lib"]


def build(verbose=True):
    """Compile libdad_hip.so for gfx950 (in-tree)."""
    return _build.build(verbose=verbose)


def lib():
    return _lib.lib()


_sys.modules.setdefault("dad_amd", _sys.modules[__name__])
for _m in ("_build", "_lib", "config", "model", "step", "dist", "data", "utils", "evaluate", "checkpoint", "pretrain", "trace"):
    _sys.modules.setdefault("dad_amd." + _m, _sys.modules[__name__ + "." + _m])
