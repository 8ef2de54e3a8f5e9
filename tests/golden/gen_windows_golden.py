"""Writes tests/golden/eval_windows.npz: the reference's SSRLModel.predict (I/model.py:225-245) on the features of
six utterances cropped to every window, the definition of dad_eval_windows' per-window outputs.

Utterances of 1, 31, 33, 64, 70 and 96 frames, features standard_normal(RandomState(SEED)) float32, student weights
oracle/data_oracle.eval_weights(SEED)[0]; SLIDING (hop 8, span 4) and PREFIX (hop 25, span 1), the window
enumeration of tests/windows_ref.windows_brute.  Stored: seed, sizes, and per mode the float32 logits [W][4] and
the int64 argmax [W] in window order (the features and weights are regenerated from the seed by the tests).  Needs
the reference checkout (its IEMOCAP trainer directory) on the command line:

    python tests/golden/gen_windows_golden.py <reference>/IEMOCAP/DAD-train-IEMOCAP
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

SEED = 21
SIZES = [1, 31, 33, 64, 70, 96]
MODES = {"sliding": (8, 4), "prefix": (25, 1)}


def inputs():
    """(feats float32 [frames, 768], sizes, offsets) of the fixture."""
    sizes = np.array(SIZES, np.int64)
    offsets = np.concatenate([[0], np.cumsum(sizes)[:-1]])
    feats = np.random.RandomState(SEED).standard_normal((int(sizes.sum()), 768)).astype(np.float32)
    return feats, sizes, offsets


def main():
    sys.dont_write_bytecode = True          # never write __pycache__ into the reference checkout
    sys.path.insert(0, os.path.abspath(sys.argv[1]))
    import torch
    import config as cfg
    import model as model_mod
    import windows_ref
    from oracle import data_oracle
    W1, b1, W2, b2 = data_oracle.eval_weights(SEED)[0]
    m = model_mod.SSRLModel(cfg)
    with torch.no_grad():
        m.student_encoder.pre_net.weight.copy_(torch.from_numpy(W1))
        m.student_encoder.pre_net.bias.copy_(torch.from_numpy(b1))
        m.student_classifier.fc_layer.weight.copy_(torch.from_numpy(W2))
        m.student_classifier.fc_layer.bias.copy_(torch.from_numpy(b2))
    feats, sizes, offsets = inputs()
    out = {"seed": np.int64(SEED), "sizes": sizes, "torch_version": np.array(torch.__version__)}
    for mode, (hop, span) in MODES.items():
        logits = []
        for i, L in enumerate(sizes):
            for a, b in windows_ref.windows_brute(int(L), hop, span, mode):
                crop = torch.from_numpy(feats[offsets[i] + a:offsets[i] + b])[None]
                logits.append(m.predict(crop).numpy()[0])
        z = np.stack(logits).astype(np.float32)
        out[mode + "_hop_span"] = np.array([hop, span], np.int64)
        out[mode + "_logits"] = z
        out[mode + "_pred"] = z.argmax(1).astype(np.int64)
    path = os.path.join(HERE, "eval_windows.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, {k: getattr(v, "shape", None) for k, v in out.items()})


if __name__ == "__main__":
    main()
