"""Writes tests/golden/eval_attribution.npz: integrated gradients of the reference's eval-mode forward by quadrature,
the definition dad_attribution's closed form is held to.

The fixture of gen_input_grad_golden.py (seven utterances of 0, 1, 31, 32, 33, 64 and 65 frames, features
standard_normal(RandomState(23)) float32, student weights oracle/data_oracle.eval_weights(23)[0]).  Per utterance
and baseline x' (zeros, and the fixture's mean frame in float32): torch autograd, in float64, of the predicted
class's logit of student_classifier(student_encoder(x)) (the body of SSRLModel.predict, I/model.py:225-245, in eval
mode) with respect to its input at the POINTS = 256 midpoints x' + alpha_k (x - x'), alpha_k = (k + 1/2) / 256,
averaged and multiplied by (x - x').  The predicted class is that of the float64 forward at x.  Stored, per baseline
b in ('zero', 'mean'): attr_<b>_<i> float32 for the utterances i of 1 and 33 frames, frame_attr_<b> [frames]
(sum_d attr) and utt_total_<b> [7] float64; the targets, the mean frame, the sizes, the seed, the point count and the
torch version.  The utterance without frames has no attribution (0).  Needs the reference checkout (its IEMOCAP
trainer directory) on the command line:

    python tests/golden/gen_attribution_golden.py <reference>/IEMOCAP/DAD-train-IEMOCAP
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from golden.gen_input_grad_golden import SEED, inputs  # noqa: E402

POINTS = 256
ATTR_OF = (1, 4)               # the utterances (of 1 and 33 frames) whose float32 attributions are stored


def mean_frame(feats):
    """The fixture's mean frame as the float32 row the tests hand to the kernel."""
    return feats.astype(np.float64).mean(0).astype(np.float32)


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
    m = m.double()
    m.eval()
    feats, sizes, offsets, _ = inputs()
    n = len(sizes)
    alphas = (np.arange(POINTS) + 0.5) / POINTS
    target = np.zeros(n, np.int64)
    out = {"seed": np.int64(SEED), "sizes": sizes, "points": np.int64(POINTS), "mean_frame": mean_frame(feats),
           "torch_version": np.array(torch.__version__)}
    for bname, xb in (("zero", np.zeros(768, np.float32)), ("mean", mean_frame(feats))):
        frame = np.zeros(feats.shape[0], np.float64)
        total = np.zeros(n, np.float64)
        base = torch.from_numpy(xb.astype(np.float64))
        for i, (o, L) in enumerate(zip(offsets, sizes)):
            if L == 0:
                continue
            x = torch.from_numpy(feats[o:o + L].astype(np.float64))
            with torch.no_grad():
                z = m.student_classifier(m.student_encoder(x[None], None))
                assert torch.equal(z, m.predict(x[None]))
            c = int(z[0].argmax())
            target[i] = c
            acc = torch.zeros_like(x)
            for a in alphas:
                p = (base[None] + a * (x - base[None]))[None].requires_grad_(True)
                g, = torch.autograd.grad(m.student_classifier(m.student_encoder(p, None))[0, c], p)
                acc += g[0]
            attr = ((x - base[None]) * acc / POINTS).numpy()
            frame[o:o + L] = attr.sum(1)
            total[i] = attr.sum()
            if i in ATTR_OF:
                out["attr_%s_%d" % (bname, i)] = attr.astype(np.float32)
        out["frame_attr_" + bname], out["utt_total_" + bname] = frame, total
    out["target"] = target
    path = os.path.join(HERE, "eval_attribution.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), {k: getattr(v, "shape", None) for k, v in out.items()})


if __name__ == "__main__":
    main()
