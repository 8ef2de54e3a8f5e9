"""Writes tests/golden/eval_rank.npz: what the reference says about seeded probabilities of n = 1,100 rows.

The fixture holds seeds and outputs only; probs_of(seed, n) below rebuilds the inputs (integer draws and one
correctly rounded float32 division each, so every machine rebuilds the same bits).  From the reference checkout (its
IEMOCAP trainer directory):
  score, pred   DACPManager.calculate_certainty_scores(probs)                       (I/utils.py:400-428)
  rank          the stable descending sort of score (torch.sort): rank[k] is the row at position k
  tau_hat [4]   torch.quantile(score[pred == c], gamma_e) per class, gamma_e = DACP_QUANTILE_END  (I/utils.py:477-481)
  stats [4]     confidence_stats of _calculate_metrics (I/inference.py:361-369): mean, std, min, max of the max
                probability, the probabilities handed over as float64 (the widening is exact)

    python tests/golden/gen_rank_golden.py <reference>/IEMOCAP/DAD-train-IEMOCAP
"""
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SEED, N = 20251, 1100


def probs_of(seed, n):
    """[n][4] float32 probabilities: integer weights in [1, 64] over their sum (ties in the scores are frequent)."""
    w = np.random.default_rng(seed).integers(1, 65, size=(n, 4)).astype(np.float32)
    return w / w.sum(axis=1, keepdims=True, dtype=np.float32)


class _Self:
    """What _calculate_metrics reads of its object: the class count; whatever else it copies into its report is None."""
    num_classes = 4

    def __getattr__(self, name):
        return None


def main():
    sys.dont_write_bytecode = True          # never write __pycache__ into the reference checkout
    sys.path.insert(0, os.path.abspath(sys.argv[1]))
    import torch
    import config as cfg
    import utils as ref_utils
    probs = probs_of(SEED, N)
    labels = np.random.default_rng(SEED + 1).integers(0, 4, size=N)
    score, pred = ref_utils.DACPManager.calculate_certainty_scores(torch.from_numpy(probs))
    gamma = float(cfg.DACP_QUANTILE_END)
    tau = torch.stack([torch.quantile(score[pred == c], gamma) for c in range(4)])
    rank = torch.sort(score, descending=True, stable=True).indices
    for _ in range(8):      # (the script's plotting and data-loading imports are not needed: an absent one is stubbed)
        try:
            import inference as ref_inference
            break
        except ModuleNotFoundError as e:
            sys.modules[e.name] = types.ModuleType(e.name)
    metrics = ref_inference.IEMOCAPCrossDomainInference._calculate_metrics(
        _Self(), labels, pred.numpy(), probs.astype(np.float64).tolist())
    cs = metrics["confidence_stats"] if "confidence_stats" in metrics else metrics["overview"]["confidence_stats"]
    stats = np.array([cs["mean_confidence"], cs["std_confidence"], cs["min_confidence"], cs["max_confidence"]])
    np.savez(os.path.join(HERE, "eval_rank.npz"), seed=np.int64(SEED), n=np.int64(N), gamma=np.float64(gamma),
             score=score.numpy().astype(np.float32), pred=pred.numpy().astype(np.int64),
             rank=rank.numpy().astype(np.int32), tau_hat=tau.numpy().astype(np.float32), stats=stats,
             use_entropy=np.int64(bool(cfg.USE_ENTROPY_IN_SCORE)))


if __name__ == "__main__":
    main()
