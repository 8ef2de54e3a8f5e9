"""The conditions that keep tests/test_gpu_exact_operands.py honest, each checked on the reference alone (no GPU):
the operands of tests/exact_problem.py are exact in fp16 and bf16, the pre-activations are exact in fp32 in any
summation order and never 0, the DACP / ECDA gates are open with the mask decisions far from their thresholds, the
strong branch is visible in the weight gradient, the fp32 references and a simulated 16-bit rounding of the
weight gradient's scales lie inside the derived bound, and wrong weight gradients lie at least 10x outside it."""
import numpy as np
import pytest
import torch

import exact_problem as X
from oracle import dad_oracle
from oracle.torch_cpu import TorchCPUStep

GEOMS = pytest.mark.parametrize("geom", X.GEOMS, ids=X.geom_id)
EPOCH = 60


def _encoder_operands(geom):
    """[(name, x [B,T,D], W1, b1)] of the three encoder passes of a post-warm-up step."""
    inp, st, _ = X.case(geom, EPOCH)
    xw, xs = X.augmented(inp, X.cfg())
    return [("clean", inp["xc"], st["student"][0], st["student"][1]),
            ("weak", xw, st["teacher"][0], st["teacher"][1]),
            ("strong", xs, st["student"][0], st["student"][1])]


@GEOMS
def test_operands_survive_fp16_and_bf16(geom):
    inp = X.case(geom, EPOCH)[0]
    assert np.abs(inp["xc"]).max() < 17 and np.abs(inp["xn"]).max() < 17
    for name, x, W1, _ in _encoder_operands(geom):
        for what, a in ((name + " x", x), (name + " W1", W1)):
            t = torch.from_numpy(np.ascontiguousarray(a))
            assert t.dtype == torch.float32
            assert torch.equal(t.half().float(), t), what + ": fp16"
            assert torch.equal(t.bfloat16().float(), t), what + ": bf16"


@GEOMS
def test_preactivations_are_exact_in_any_order_and_never_zero(geom):
    perm = np.random.RandomState(0).permutation(768)
    for name, x, W1, b1 in _encoder_operands(geom):
        B, T, D = x.shape
        x2 = x.reshape(B * T, D)
        want = X.preact64(x, W1, b1).reshape(B * T, -1)
        got = x2 @ W1.T + b1
        assert got.dtype == np.float32
        assert np.array_equal(got.astype(np.float64), want), name
        got_p = np.ascontiguousarray(x2[:, perm]) @ np.ascontiguousarray(W1[:, perm]).T + b1
        assert np.array_equal(got_p.astype(np.float64), want), name + " (columns permuted)"
        units = want * 2.0 ** 14
        assert np.array_equal(units, np.round(units)) and np.all(np.abs(units) % 2 == 1), name   # odd multiples of 2^-14
        assert np.all(want != 0), name
        mag = np.abs(x2).astype(np.float64) @ np.abs(W1).astype(np.float64).T + np.abs(b1).astype(np.float64)
        assert mag.max() < 1024, (name, mag.max())


@GEOMS
def test_gates_are_open_and_mask_decisions_are_robust(geom):
    r = X.case(geom, EPOCH)[2]["oracle"]
    mask = np.asarray(r["mask"])
    assert mask.sum() >= 2 and r["consistency_loss"] != 0.0, (mask.sum(), r["consistency_loss"])
    if geom["B"] >= 12:
        assert r["ecda_loss"] != 0.0
    if geom["Bn"] >= 16:
        assert mask.min() == 0 and mask.max() == 1, mask
    margin = np.abs(np.asarray(r["score"], np.float64) - np.asarray(r["tau_after"], np.float64)[r["pred"]]).min()
    print("%s: mask %d/%d, smallest |score - threshold| %.3g" % (X.geom_id(geom), mask.sum(), mask.size, margin))
    assert margin >= 1e-3, margin


@GEOMS
def test_strong_branch_is_visible_in_the_weight_gradient(geom):
    ref = X.case(geom, EPOCH)[2]
    share = np.linalg.norm(ref["strong"][1]) / np.linalg.norm(ref["S"][0])
    print("%s: strong share of |S_W1| %.3f" % (X.geom_id(geom), share))
    assert share >= 0.10, share


@GEOMS
def test_tail_term_stays_a_small_part_of_the_bound(geom):
    """The worst-case fp32 error of the classifier backward (exact_problem's tail term) matters where dL/de
    cancels; elsewhere the bound is (eps_op + n_rows u + 1e-4) S_W1 as before: at least half of the elements
    keep the fp16 bound within a factor of 20."""
    ref = X.case(geom, EPOCH)[2]
    S = ref["S"][0]
    rel = ref["tail"][S > 0] / S[S > 0]
    print("%s: tail term / S_W1 median %.3g, 90th percentile %.3g, max %.3g" % (
        X.geom_id(geom), np.median(rel), np.percentile(rel, 90), rel.max()))
    assert np.all(ref["tail"][S == 0] == 0)
    assert np.median(rel) <= 19 * X.bound("dW1", "fp16", ref["n_rows"])


def _torch_step(inp, st, epoch):
    """Plain fp32 autograd: (pre-clip gradients, outputs)."""
    c = dict(X.cfg(), GRADIENT_CLIPPING=False)      # (the step would scale .grad in place)
    t = TorchCPUStep(*st["student"], c)
    t.load_state(st)
    out = t.step(inp, epoch, draws=inp)
    grads = [p.grad.detach().numpy().copy() for p in t.student]
    return grads, {k: v.detach().numpy() for k, v in out.items() if torch.is_tensor(v)}


@pytest.mark.parametrize("epoch", [0, EPOCH])
@GEOMS
def test_fp32_references_lie_inside_the_fp32_bound(geom, epoch):
    inp, st, ref = X.case(geom, epoch)
    r = ref["oracle"]
    tg, tout = _torch_step(inp, st, epoch)
    if epoch >= 30:
        np.testing.assert_array_equal(tout["mask"], r["mask"])
    for who, grads, out in (("oracle", r["grads"], r), ("torch", tg, tout)):
        ratios = X.grad_ratios(grads, ref, "fp32")
        ratios.update(X.forward_ratios(out, {**ref, "e": {k: v for k, v in ref["e"].items() if k in out},
                                             "z": {k: v for k, v in ref["z"].items() if k in out}}))
        print("%s e%d %s: %s" % (X.geom_id(geom), epoch, who, {k: float("%.3g" % v) for k, v in ratios.items()}))
        assert max(ratios.values()) <= 1.0, (who, ratios)


def _scales(ref):
    """Per-(utterance, h) scales dL/de / len of the clean and strong rows, stacked [Bc + Bn, H]."""
    v = [p["g"] / np.maximum(p["vlen"], 1.0)[:, None] for p in (ref["parts"]["clean"], ref["parts"]["strong"])]
    return np.concatenate(v, 0)


def _round16(v, prec):
    """The weight gradient's rounding of the scales (csrc/wgrad_direct.h): bf16 directly; fp16 after the power of
    two that maps hidden unit h's largest |v| into [2^14, 2^15)."""
    if prec == "bf16":
        return torch.from_numpy(v.astype(np.float32)).bfloat16().double().numpy()
    mx = np.abs(v).max(0)
    s = 14 - np.floor(np.log2(np.where(mx > 0, mx, 1.0)))
    return np.float16(v * 2.0 ** s).astype(np.float64) / 2.0 ** s


def _dw1(ref, scale=None, clean=None, strong=None):
    """dW1 in float64 from the reference's parts; `scale`: stacked replacement scales; clean / strong: replacement
    fields of a branch (x, act, vlen)."""
    pc, ps = dict(ref["parts"]["clean"], **(clean or {})), dict(ref["parts"]["strong"], **(strong or {}))
    if scale is None:
        return X.wgrad64(**pc)[0] + X.wgrad64(**ps)[0]
    Bc = pc["x"].shape[0]
    return X.wgrad64_scaled(pc["x"], pc["act"], scale[:Bc])[0] + X.wgrad64_scaled(ps["x"], ps["act"], scale[Bc:])[0]


def _ratio(dw, ref, prec):
    return X.worst(dw - ref["grads"][0], X.grad_limit("dW1", prec, ref))


@GEOMS
def test_simulated_16bit_scale_rounding_lies_inside_the_bound(geom):
    ref = X.case(geom, EPOCH)[2]
    assert _ratio(_dw1(ref), ref, "fp32") < 1e-6                 # the rebuild itself
    for prec in ("fp16", "bf16"):
        r = _ratio(_dw1(ref, scale=_round16(_scales(ref), prec)), ref, prec)
        print("%s: simulated %s scales, worst err / bound %.3f" % (X.geom_id(geom), prec, r))
        assert r <= 1.0, (prec, r)


def _last_slab_off(part, u):
    """The branch's ReLU' pattern without the last 32-row slab of utterance u's frames."""
    n = int(part["vlen"][u])
    act = part["act"].copy()
    act[u, 32 * ((n - 1) // 32):n] = False
    return act


def _mutants(geom):
    inp, st, ref = X.case(geom, EPOCH)
    pc, ps = ref["parts"]["clean"], ref["parts"]["strong"]
    W1, b1 = st["student"][:2]
    us = int(np.nonzero(np.asarray(ref["oracle"]["mask"]) > 0)[0][-1])      # the last strong utterance in the mask
    yield "last slab of the last masked-in strong utterance dropped", _dw1(ref, strong=dict(act=_last_slab_off(ps, us)))
    uc = pc["x"].shape[0] - 1
    yield "last clean slab dropped", _dw1(ref, clean=dict(act=_last_slab_off(pc, uc)))
    lens = pc["vlen"].copy()
    # the clean utterance whose scales g / len move most under len + 1 (by |g| / (len (len + 1)))
    u = int(np.argmax(np.linalg.norm(pc["g"], axis=1) / (lens * (lens + 1))))
    lens[u] += 1
    yield "clean utterance %d divided by len + 1" % u, _dw1(ref, clean=dict(lens=lens))
    h = int(np.argmax(np.linalg.norm(ref["grads"][0], axis=1)))
    dw = ref["grads"][0].copy()
    dw[h] *= 2.0
    yield "hidden unit %d's row scaled by 2" % h, dw
    xw = ref["parts"]["weak_x"]
    act_w = dad_oracle.encoder_forward(xw, inp["mn"], W1, b1)[1]
    yield "weak-augmented input in place of the strong one", _dw1(ref, strong=dict(x=xw, act=act_w))


@GEOMS
def test_wrong_weight_gradients_exceed_the_fp16_bound_tenfold(geom):
    ref = X.case(geom, EPOCH)[2]
    for what, dw in _mutants(geom):
        r = _ratio(dw, ref, "fp16")
        print("%s: %s: %.1f x the fp16 bound" % (X.geom_id(geom), what, r))
        assert r >= 10.0, (what, r)
