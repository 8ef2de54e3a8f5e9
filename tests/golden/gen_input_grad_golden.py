"""Writes tests/golden/eval_input_grad.npz: torch autograd of the reference's SSRLModel.predict (I/model.py:225-245)
in eval mode with respect to its input features, the definition of dad_input_grad's gradient under
dz = softmax(z) - onehot(y).

Seven utterances of 0, 1, 31, 32, 33, 64 and 65 frames, features standard_normal(RandomState(SEED)) float32, student
weights oracle/data_oracle.eval_weights(SEED)[0], labels 0, 1, 2, 3, 0, 1, 2.  Per utterance L = F.cross_entropy(
model.predict(x), y) and dL/dx by autograd (predict runs under no_grad, so the graph is built from the two module
calls of its body, student_classifier(student_encoder(x, None)) in eval mode, checked equal to predict's logits).
Stored: the seed, the sizes, the labels, sgn(dL/dx) as int8 for every frame [frames][768], dL/dx float32 for the utterances of 1 and 33 frames, the clean losses and logits, the losses
[3][7] and logits [3][7][4] at x + eps * sgn(dL/dx) for eps in EPS, and the torch version (features and weights are
regenerated from the seed by the tests).  The utterance without frames has logits = b2 by the kernel's definition and
loss 0 here; the reference model is not asked about it.  Needs the reference checkout (its IEMOCAP trainer directory)
on the command line:

    python tests/golden/gen_input_grad_golden.py <reference>/IEMOCAP/DAD-train-IEMOCAP
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

SEED = 23
SIZES = [0, 1, 31, 32, 33, 64, 65]
LABELS = [0, 1, 2, 3, 0, 1, 2]
EPS = (0.01, 0.05, 0.25)
GRAD_OF = (1, 4)               # the utterances (of 1 and 33 frames) whose float32 gradient is stored


def inputs():
    """(feats float32 [frames, 768], sizes, offsets, labels) of the fixture."""
    sizes = np.array(SIZES, np.int64)
    offsets = np.concatenate([[0], np.cumsum(sizes)[:-1]])
    feats = np.random.RandomState(SEED).standard_normal((int(sizes.sum()), 768)).astype(np.float32)
    return feats, sizes, offsets, np.array(LABELS, np.int64)


def main():
    sys.dont_write_bytecode = True          # never write __pycache__ into the reference checkout
    sys.path.insert(0, os.path.abspath(sys.argv[1]))
    import torch
    import torch.nn.functional as F
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
    feats, sizes, offsets, labels = inputs()
    n = len(sizes)
    sign = np.zeros(feats.shape, np.int8)
    grads = {}
    loss0 = np.zeros(n, np.float32)
    logits0 = np.tile(np.asarray(b2, np.float32), (n, 1))
    loss = np.zeros((len(EPS), n), np.float32)
    logits = np.tile(np.asarray(b2, np.float32), (len(EPS), n, 1))
    for i, (o, L) in enumerate(zip(offsets, sizes)):
        if L == 0:
            continue
        y = torch.tensor([labels[i]])
        x = torch.from_numpy(feats[o:o + L])[None].requires_grad_(True)
        z = m.student_classifier(m.student_encoder(x, None))     # predict's body: predict itself runs under no_grad
        assert torch.equal(z.detach(), m.predict(x.detach()))
        l = F.cross_entropy(z, y)
        g, = torch.autograd.grad(l, x)
        loss0[i], logits0[i] = l.item(), z.detach().numpy()[0]
        sign[o:o + L] = np.sign(g.numpy()[0]).astype(np.int8)
        if i in GRAD_OF:
            grads["grad_%d" % i] = g.numpy()[0].copy()
        for k, e in enumerate(EPS):
            with torch.no_grad():
                zk = m.predict(torch.from_numpy(feats[o:o + L] + np.float32(e) * sign[o:o + L].astype(np.float32))[None])
                loss[k, i], logits[k, i] = F.cross_entropy(zk, y).item(), zk.numpy()[0]
    out = {"seed": np.int64(SEED), "sizes": sizes, "labels": labels, "eps": np.array(EPS, np.float64), "sign": sign,
           "loss0": loss0, "logits0": logits0, "loss": loss, "logits": logits,
           "torch_version": np.array(torch.__version__)}
    out.update(grads)
    path = os.path.join(HERE, "eval_input_grad.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), {k: getattr(v, "shape", None) for k, v in out.items()})


if __name__ == "__main__":
    main()
