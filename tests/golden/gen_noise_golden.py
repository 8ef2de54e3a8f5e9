"""Writes tests/golden/eval_noise.npz: the reference's SSRLModel.get_embeddings / predict (I/model.py:225-265) in
eval mode on x + sigma_k n, the definition of dad_eval_noise's per-level outputs.

Seven utterances of 0, 1, 31, 32, 33, 64 and 65 frames, features standard_normal(RandomState(SEED)) float32, noise
standard_normal(RandomState(SEED + 1)) float32 per frame (frame t of utterance i is row offsets[i] + t of the noise
array: inputs() below; the tests move it into the kernel's slab-aligned layout), four levels, student weights
oracle/data_oracle.eval_weights(SEED)[0].  Stored: the seed, the sizes, the levels and per level the float32
embeddings [K][7][256], logits [K][7][4] and the int64 argmax [K][7] (features, noise and weights are regenerated
from the seed by the tests).  An utterance without frames has a zero embedding and logits = b2 by the kernel's
definition; the reference model is not asked about it.  Needs the reference checkout (its IEMOCAP trainer directory)
on the command line:

    python tests/golden/gen_noise_golden.py <reference>/IEMOCAP/DAD-train-IEMOCAP
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

SEED = 23
SIZES = [0, 1, 31, 32, 33, 64, 65]
SIGMAS = (0.0, 0.01, 0.05, 0.25)


def inputs():
    """(feats float32 [frames, 768], noise float32 [frames, 768], sizes, offsets) of the fixture."""
    sizes = np.array(SIZES, np.int64)
    offsets = np.concatenate([[0], np.cumsum(sizes)[:-1]])
    feats = np.random.RandomState(SEED).standard_normal((int(sizes.sum()), 768)).astype(np.float32)
    noise = np.random.RandomState(SEED + 1).standard_normal((int(sizes.sum()), 768)).astype(np.float32)
    return feats, noise, sizes, offsets


def slab_aligned(noise, sizes, offsets):
    """The per-frame noise rows in dad_eval_noise's explicit layout [32 * slabs, 768] (zeros in the unused rows)."""
    soff = np.concatenate([[0], np.cumsum((sizes + 31) // 32)])
    out = np.zeros((32 * int(soff[-1]), noise.shape[1]), np.float32)
    for i, (o, L) in enumerate(zip(offsets, sizes)):
        out[32 * soff[i]:32 * soff[i] + L] = noise[o:o + L]
    return out


def main():
    sys.dont_write_bytecode = True          # never write __pycache__ into the reference checkout
    sys.path.insert(0, os.path.abspath(sys.argv[1]))
    import torch
    import config as cfg
    import model as model_mod
    from oracle import data_oracle
    W1, b1, W2, b2 = data_oracle.eval_weights(SEED)[0]
    m = model_mod.SSRLModel(cfg)
    with torch.no_grad():
        m.student_encoder.pre_net.weight.copy_(torch.from_numpy(W1))
        m.student_encoder.pre_net.bias.copy_(torch.from_numpy(b1))
        m.student_classifier.fc_layer.weight.copy_(torch.from_numpy(W2))
        m.student_classifier.fc_layer.bias.copy_(torch.from_numpy(b2))
    m.eval()
    feats, noise, sizes, offsets = inputs()
    K, n = len(SIGMAS), len(sizes)
    emb = np.zeros((K, n, 256), np.float32)
    logits = np.tile(np.asarray(b2, np.float32), (K, n, 1))
    for k, s in enumerate(SIGMAS):
        for i, (o, L) in enumerate(zip(offsets, sizes)):
            if L == 0:
                continue
            x = torch.from_numpy(feats[o:o + L] + np.float32(s) * noise[o:o + L])[None]
            with torch.no_grad():
                emb[k, i] = m.get_embeddings(x).numpy()[0]
                logits[k, i] = m.predict(x).numpy()[0]
    out = {"seed": np.int64(SEED), "sizes": sizes, "sigmas": np.array(SIGMAS, np.float64), "emb": emb,
           "logits": logits, "pred": logits.argmax(-1).astype(np.int64), "torch_version": np.array(torch.__version__)}
    path = os.path.join(HERE, "eval_noise.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, {k: getattr(v, "shape", None) for k, v in out.items()})


if __name__ == "__main__":
    main()
