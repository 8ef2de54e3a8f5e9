"""Writes tests/golden/eval_models.npz: the reference's SSRLModel.predict (I/model.py:225-245) in eval mode for four
networks on one split, the definition of dad_eval_models' per-model outputs and of its mean ensemble.

Seven utterances of 0, 1, 31, 32, 33, 64 and 65 frames, features standard_normal(RandomState(SEED)) float32; the
four networks are oracle/data_oracle.eval_weights(SEED) (student, teacher) and eval_weights(SEED + 1) (student,
teacher), in that order, each loaded into the reference model's student.  Stored: the seed, the sizes and per network
the float32 logits [4][7][4], softmax probabilities [4][7][4] and the int64 argmax [4][7]; the float32 mean of the four
probability rows [7][4] (tests/models_ref.ensemble_chain32 with equal weights) and its argmax.  Features and weights
are regenerated from the seed by the tests.  An utterance without frames has logits = b2 by the kernel's definition;
the reference model is not asked about it.  SEED is chosen so that every utterance's top-two margin exceeds MARGIN, per
network (logits and probabilities) and in the ensemble (asserted here and in the CPU test), so no argmax comparison
needs an exclusion.  Needs the reference checkout (its IEMOCAP trainer directory) on the command line:

    python tests/golden/gen_models_golden.py <reference>/IEMOCAP/DAD-train-IEMOCAP
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

SEED = 21
SIZES = [0, 1, 31, 32, 33, 64, 65]
MARGIN = 1e-3


def inputs(seed=SEED):
    """(feats float32 [frames, 768], sizes, offsets) of the fixture."""
    sizes = np.array(SIZES, np.int64)
    offsets = np.concatenate([[0], np.cumsum(sizes)[:-1]])
    feats = np.random.RandomState(seed).standard_normal((int(sizes.sum()), 768)).astype(np.float32)
    return feats, sizes, offsets


def networks(seed=SEED):
    """The four (W1, b1, W2, b2) of the fixture, in the golden's order."""
    from oracle import data_oracle
    return list(data_oracle.eval_weights(seed)) + list(data_oracle.eval_weights(seed + 1))


def margins(x):
    """Top-two margin of every row of x [..., 4]."""
    s = np.sort(np.asarray(x, np.float64), -1)
    return s[..., -1] - s[..., -2]


def main():
    sys.dont_write_bytecode = True          # never write __pycache__ into the reference checkout
    sys.path.insert(0, os.path.abspath(sys.argv[1]))
    import torch
    import config as cfg
    import model as model_mod
    import models_ref
    feats, sizes, offsets = inputs()
    nets = networks()
    K, n = len(nets), len(sizes)
    logits = np.zeros((K, n, 4), np.float32)
    probs = np.zeros((K, n, 4), np.float32)
    for k, (W1, b1, W2, b2) in enumerate(nets):
        m = model_mod.SSRLModel(cfg)
        with torch.no_grad():
            m.student_encoder.pre_net.weight.copy_(torch.from_numpy(W1))
            m.student_encoder.pre_net.bias.copy_(torch.from_numpy(b1))
            m.student_classifier.fc_layer.weight.copy_(torch.from_numpy(W2))
            m.student_classifier.fc_layer.bias.copy_(torch.from_numpy(b2))
        m.eval()
        logits[k] = np.asarray(b2, np.float32)
        for i, (o, L) in enumerate(zip(offsets, sizes)):
            if L:
                with torch.no_grad():
                    logits[k, i] = m.predict(torch.from_numpy(feats[o:o + L])[None]).numpy()[0]
        probs[k] = torch.softmax(torch.from_numpy(logits[k]), dim=1).numpy()
    ens = models_ref.ensemble_chain32(probs, models_ref.norm_weights(None, K))
    worst = min(margins(logits).min(), margins(probs).min(), margins(ens).min())
    assert worst > MARGIN, "seed %d has a top-two margin of %.3g" % (SEED, worst)
    out = {"seed": np.int64(SEED), "sizes": sizes, "logits": logits, "probs": probs,
           "pred": logits.argmax(-1).astype(np.int64), "ens_probs": ens, "ens_pred": ens.argmax(-1).astype(np.int64),
           "torch_version": np.array(torch.__version__)}
    path = os.path.join(HERE, "eval_models.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, {k: getattr(v, "shape", None) for k, v in out.items()}, "smallest margin %.3g" % worst)


if __name__ == "__main__":
    main()
