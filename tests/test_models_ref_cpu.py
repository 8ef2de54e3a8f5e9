"""dad_eval_models without a GPU: the float64 reference (tests/models_ref.py) on hand examples and against its
wrong-answer controls, the golden fixture's margins, the ctypes mirror of dad_models_args and the DAD_EM_* slots, the
host validation of the entry points, the workspace query, and the host side of ensemble_report."""
import ctypes
import math
import os
import subprocess

import numpy as np
import pytest

import dadpkg
import models_ref as mr
from golden import gen_models_golden as gm

PKG = dadpkg.pkg()
E = PKG.evaluate
L_ = PKG._lib


def _golden():
    return np.load(os.path.join(dadpkg.ROOT, "tests", "golden", "eval_models.npz"))


def test_golden_fixture_margins_and_consistency():
    """Every utterance's top-two margin exceeds 1e-3 per network (logits and probabilities) and in the ensemble, so
    the GPU module compares every argmax without an exclusion; the stored ensemble is the float32 chain of the stored
    probabilities; the stored logits agree with a float64 restatement of the forward at the eval goldens' 1e-4."""
    g = _golden()
    assert int(g["seed"]) == gm.SEED and g["sizes"].tolist() == gm.SIZES == [0, 1, 31, 32, 33, 64, 65]
    assert g["logits"].shape == (4, 7, 4) and g["probs"].shape == (4, 7, 4) and g["ens_probs"].shape == (7, 4)
    for key in ("logits", "probs", "ens_probs"):
        assert g[key].dtype == np.float32
        assert gm.margins(g[key]).min() > 1e-3, key
    np.testing.assert_array_equal(g["pred"], g["probs"].argmax(-1))
    np.testing.assert_array_equal(g["ens_probs"], mr.ensemble_chain32(g["probs"], mr.norm_weights(None, 4)))
    np.testing.assert_array_equal(g["ens_pred"], g["ens_probs"].argmax(-1))
    assert np.abs(g["ens_probs"] - g["probs"].astype(np.float64).mean(0)).max() <= 4 * 2.0 ** -24
    feats, sizes, offsets = gm.inputs()
    for k, (W1, b1, W2, b2) in enumerate(gm.networks()):
        for i, (o, L) in enumerate(zip(offsets, sizes)):
            x = feats[o:o + L].astype(np.float64)
            e = np.maximum(x @ W1.T.astype(np.float64) + b1, 0).sum(0) / max(L, 1) if L else np.zeros(256)
            np.testing.assert_allclose(e @ W2.T.astype(np.float64) + b2, g["logits"][k, i], rtol=1e-5, atol=1e-4)
    # the four networks are not copies of one another
    assert len({g["pred"][k].tobytes() for k in range(4)}) == 4


def test_models_args_match_c_layout(tmp_path):
    """Compile a C probe against include/dad.h and compare sizeof / offsetof of dad_models_args with ctypes, and the
    DAD_EM_* numbers with the binding's."""
    cls = L_.DadModelsArgs
    consts = {"DAD_EM_" + k[3:]: getattr(L_, k) for k in dir(L_) if k.startswith("EM_")}
    assert len(consts) == 17
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "dad.h"', "int main(void){",
             'printf("size %zu\\n", sizeof(dad_models_args));']
    for f in cls._fields_:
        lines.append('printf("%s %%zu\\n", offsetof(dad_models_args, %s));' % (f[0], f[0]))
    for name in consts:
        lines.append('printf("%s %%d\\n", (int)%s);' % (name, name))
    lines.append("return 0;}")
    c = tmp_path / "probe.c"
    c.write_text("\n".join(lines))
    exe = tmp_path / "probe"
    subprocess.check_call(["gcc", "-I", os.path.join(dadpkg.ROOT, "include"), str(c), "-o", str(exe)])
    out = dict(l.split() for l in subprocess.check_output([str(exe)]).decode().splitlines())
    assert int(out["size"]) == ctypes.sizeof(cls)
    for f in cls._fields_:
        assert int(out[f[0]]) == getattr(cls, f[0]).offset, f[0]
    for name, v in consts.items():
        assert int(out[name]) == v, name
    # the slots do not overlap: 10 confusion matrices, two [10][10] matrices, [9], three scalars, [8], K
    M = L_.EM_MEMBERS
    assert M == L_.EM_MAX_MODELS + 2
    assert L_.EM_DISAGREE == L_.EM_CONF + 16 * M and L_.EM_ONLY == L_.EM_DISAGREE + M * M
    assert L_.EM_HIST == L_.EM_ONLY + M * M and L_.EM_N == L_.EM_HIST + L_.EM_MAX_MODELS + 1
    assert (L_.EM_N_LABELLED, L_.EM_N_SKIPPED, L_.EM_NONFINITE) == (L_.EM_N + 1, L_.EM_N + 2, L_.EM_N + 3)
    assert L_.EM_K == L_.EM_NONFINITE + L_.EM_MAX_MODELS and L_.EM_K < L_.EM_COUNTS
    assert (L_.EM_SUM_SCORE, L_.EM_SUM_ENTROPY, L_.EM_SUM_NLL, L_.EM_SUM_BRIER, L_.EM_SUMS) == (0, M, 2 * M, 3 * M, 4 * M)


def test_exports_are_listed():
    for name in ("dad_eval_models_workspace_bytes", "dad_eval_models"):
        assert name in L_.EXPORTS and name in L_.OPTIONAL_EXPORTS
        assert hasattr(L_.lib(), name)
    assert "eval_models.hip" in PKG._build.SOURCES
    for name in ("enqueue_eval_models", "evaluate_models_store", "ensemble_report"):
        assert callable(getattr(PKG, name))


def _host_args(**change):
    """Arguments that pass every pointer check with made-up addresses: only error paths may be called with them."""
    a = L_.DadModelsArgs()
    for name in ("store", "rows", "lens", "slab_off", "counts", "sums"):
        setattr(a, name, 0x1000)
    a.n, a.slabs, a.K = 39, 70, 3
    for k in range(3):
        a.models[k] = 0x1000
        a.weight[k] = 1.0
    a.store_dtype, a.use_entropy, a.precision = L_.STORE_F32, 1, L_.PREC_FP32
    for k, v in change.items():
        if k.startswith("weight"):
            a.weight[int(k[6:])] = v
        elif k.startswith("model"):
            a.models[int(k[5:])] = v
        else:
            setattr(a, k, v)
    return a


def test_host_validation_needs_no_gpu():
    """Every listed error returns its code before anything is launched: these calls run where there is no GPU."""
    fn = L_.lib().dad_eval_models
    ws = ctypes.c_void_p(0x1000)
    call = lambda **change: fn(_host_args(**change), ws, None)
    for name in ("store", "rows", "lens", "slab_off", "counts", "sums"):
        assert call(**{name: None}) == L_.E_ARG, name
    assert fn(_host_args(), None, None) == L_.E_ARG
    assert fn(None, ws, None) == L_.E_ARG
    for K in (0, -1, 9):
        assert call(K=K) == L_.E_ARG
    for k in range(3):
        assert call(**{"model%d" % k: None}) == L_.E_ARG
    for bad in (-0.5, float("nan"), float("inf"), -float("inf")):
        assert call(weight1=bad) == L_.E_ARG
        assert call(weight0=bad) == L_.E_ARG
    assert call(weight0=0.0, weight1=0.0, weight2=0.0) == L_.E_ARG          # sum of the weights is 0
    assert call(store_dtype=3) == L_.E_ARG
    assert call(store_dtype=-1) == L_.E_ARG
    assert call(precision=3) == L_.E_ARG
    assert call(precision=L_.PREC_BF16) == L_.E_UNSUPPORTED
    assert call(n=0) == L_.E_SHAPE
    assert call(slabs=-1) == L_.E_SHAPE
    assert call(n=1, slabs=2 ** 26 + 1) == L_.E_SHAPE
    assert call(n=2 ** 20, slabs=2 ** 21, K=4, model3=0x1000, weight3=1.0) == L_.E_SHAPE      # 2^21 * 4 * 256 = 2^31
    assert call(n=2 ** 20, slabs=2 ** 23, K=1) == L_.E_SHAPE
    # entries beyond K are not read: a NULL model, a NaN weight
    assert call(model5=None, weight5=float("nan"), n=0) == L_.E_SHAPE
    # one zero weight among positive ones is allowed (the call then fails only on the shape given here)
    assert call(weight1=0.0, n=0) == L_.E_SHAPE


def test_workspace_query():
    wsb = L_.lib().dad_eval_models_workspace_bytes
    assert wsb(39, 70, 4, L_.PREC_FP32) >= 70 * 4 * 1024
    # FP16 adds K fp16 copies of W1
    for K in (1, 2, 8):
        assert wsb(39, 70, K, L_.PREC_FP16) == wsb(39, 70, K, L_.PREC_FP32) + K * 2 * 256 * 768
    # monotone in K and in slabs; the partials grow as K x slabs x 1 KB
    for prec in (L_.PREC_FP32, L_.PREC_FP16):
        sizes = [wsb(39, 70, K, prec) for K in range(1, 9)]
        assert all(b > a > 0 for a, b in zip(sizes, sizes[1:]))
        sizes = [wsb(39, s, 3, prec) for s in (0, 1, 2, 70, 71, 1070)]
        assert all(b >= a > 0 for a, b in zip(sizes, sizes[1:])) and sizes[-1] > sizes[0]
    assert wsb(39, 1070, 8, 0) - wsb(39, 70, 8, 0) == 1000 * 8 * 1024
    for n, slabs, K in ((0, 0, 1), (39, -1, 1), (39, 70, 0), (39, 70, 9), (1, 2 ** 26 + 1, 1), (2 ** 20, 2 ** 21, 4),
                        (2 ** 20, 2 ** 20, 8)):
        assert wsb(n, slabs, K, L_.PREC_FP32) == 0, (n, slabs, K)
    assert wsb(2 ** 20, 2 ** 21 - 1, 4, L_.PREC_FP32) > 0


def test_block_on_a_hand_example():
    """Three models, five utterances (one unlabelled), probabilities chosen by hand."""
    pred = np.array([[0, 1, 2, 3, 0], [0, 1, 1, 0, 1], [1, 1, 2, 2, 2]])
    labels = np.array([0, 1, 2, -1, 3])
    probs = np.full((3, 5, 4), 0.1, np.float32)
    for k in range(3):
        probs[k, np.arange(5), pred[k]] = 0.7
    score = np.ones((3, 5), np.float32)
    r = mr.block(L_, probs, pred, score, labels)
    c = r["counts"]
    np.testing.assert_array_equal(r["votes"], [[2, 1, 0, 0], [0, 3, 0, 0], [0, 1, 2, 0], [1, 0, 1, 1], [1, 1, 1, 0]])
    np.testing.assert_array_equal(r["vote_pred"], [0, 1, 2, 0, 0])          # utterances 3 and 4: ties to the lowest
    np.testing.assert_array_equal(r["n_correct"], [2, 3, 2, -1, 0])
    np.testing.assert_array_equal(c[L_.EM_HIST:L_.EM_HIST + 9], [1, 0, 2, 1, 0, 0, 0, 0, 0])
    assert (c[L_.EM_N], c[L_.EM_N_LABELLED], c[L_.EM_N_SKIPPED], c[L_.EM_K]) == (5, 4, 1, 3)
    dis = c[L_.EM_DISAGREE:L_.EM_DISAGREE + 100].reshape(10, 10)
    only = c[L_.EM_ONLY:L_.EM_ONLY + 100].reshape(10, 10)
    assert dis[0, 1] == dis[1, 0] == 3 and dis[0, 2] == 3 and dis[1, 2] == 4 and not np.diag(dis).any()
    assert (only[0, 0], only[1, 1], only[2, 2]) == (3, 2, 2)                 # the diagonal: correct counts
    assert only[0, 1] == 1 and only[1, 0] == 0 and only[0, 2] == 1 and only[2, 0] == 0
    assert only[0, 1] + only[1, 1] - only[1, 0] == only[0, 0]               # McNemar's cells close the table
    cm0 = c[L_.EM_CONF:L_.EM_CONF + 16].reshape(4, 4)
    assert cm0[0, 0] == cm0[1, 1] == cm0[2, 2] == cm0[3, 0] == 1 and cm0.sum() == 4
    # members K (ensemble) and K + 1 (vote) have their rows; members beyond are zero
    assert c[L_.EM_CONF + 16 * 3:L_.EM_CONF + 16 * 5].sum() == 8 and not c[L_.EM_CONF + 16 * 5:L_.EM_DISAGREE].any()
    assert not dis[5:].any() and not dis[:, 5:].any() and not only[5:].any() and not only[:, 5:].any()
    # sums: entropy of (0.7, 0.1, 0.1, 0.1) on every utterance; NLL and Brier on the labelled ones
    p = np.array([0.7, 0.1, 0.1, 0.1], np.float32).astype(np.float64)
    h = -(p * np.log(p)).sum()
    np.testing.assert_allclose(r["sums"][L_.EM_SUM_ENTROPY:L_.EM_SUM_ENTROPY + 3], 5 * h, rtol=1e-14)
    nll0 = -3 * math.log(p[0]) - math.log(p[1])
    np.testing.assert_allclose(r["sums"][L_.EM_SUM_NLL], nll0, rtol=1e-14)
    right, wrong = (1 - p[0]) ** 2 + 3 * p[1] ** 2, (1 - p[1]) ** 2 + p[0] ** 2 + 2 * p[1] ** 2
    np.testing.assert_allclose(r["sums"][L_.EM_SUM_BRIER], 3 * right + wrong, rtol=1e-14)
    assert r["sums"][L_.EM_SUM_SCORE] == 5.0 and not r["sums"][L_.EM_SUM_SCORE + 3:L_.EM_SUM_ENTROPY].any()
    # K = 1 with weight 1: the chain returns the probabilities bit for bit
    one = mr.block(L_, probs[:1], pred[:1], score[:1], labels, weights=[3.0])
    assert one["ens32"].tobytes() == probs[0].tobytes()
    np.testing.assert_array_equal(one["ens_pred"], pred[0])
    np.testing.assert_array_equal(one["vote_pred"], pred[0])


def test_weights_are_normalised_in_double_then_rounded():
    wn = mr.norm_weights([1.0, 2.0, 4.0], 3)
    assert wn.dtype == np.float32
    np.testing.assert_array_equal(wn, np.array([1 / 7, 2 / 7, 4 / 7], np.float64).astype(np.float32))
    assert mr.norm_weights(None, 4).tolist() == [0.25] * 4
    assert mr.norm_weights([5.0], 1).tolist() == [1.0]
    with pytest.raises(ValueError):
        E._models_weights([1.0, -1.0], 2)
    with pytest.raises(ValueError):
        E._models_weights([0.0, 0.0], 2)
    with pytest.raises(ValueError):
        E._models_weights([1.0], 2)
    assert E._models_weights(None, 3) == [1.0, 1.0, 1.0]


@pytest.mark.parametrize("variant", mr.VARIANTS)
@pytest.mark.parametrize("K", [2, 3, 8])
def test_wrong_references_differ(variant, K):
    """Each wrong reference gives another counts block (or vote) on the seeded CPU case, at every K the GPU module
    uses beyond 1: an equality check against the right reference can fail."""
    probs, pred, score, labels = mr.cpu_case(K)
    ref = mr.block(L_, probs, pred, score, labels)
    wrong = mr.block(L_, probs, pred, score, labels, variant=variant)
    if variant == "vote_tie_high":
        assert (wrong["vote_pred"] != ref["vote_pred"]).any()
        if K < 8:
            assert ((ref["votes"] == ref["votes"].max(1, keepdims=True)).sum(1) > 1).any()     # there are ties
    else:
        lo = L_.EM_ONLY if variant == "only_transposed" else L_.EM_DISAGREE
        assert (wrong["counts"][lo:lo + 100] != ref["counts"][lo:lo + 100]).any()
        assert (np.delete(wrong["counts"], np.arange(lo, lo + 100)) == np.delete(ref["counts"], np.arange(lo, lo + 100))).all()
    assert (wrong["counts"] != ref["counts"]).any()


def test_mcnemar_exact_p_value():
    """The exact two-sided binomial p-value against a direct sum of the binomial pmf in rational arithmetic."""
    from fractions import Fraction
    for b, c in ((0, 0), (1, 0), (3, 9), (9, 3), (5, 5), (0, 6), (20, 41), (700, 800)):
        n, k = b + c, min(b, c)
        want = 1.0 if n == 0 else min(1.0, float(2 * sum(Fraction(math.comb(n, i), 2 ** n) for i in range(k + 1))))
        assert E.mcnemar_exact(b, c) == pytest.approx(want, rel=1e-12), (b, c)
    assert E.mcnemar_exact(0, 6) == pytest.approx(2 * 0.5 ** 6)
    assert E.mcnemar_exact(5, 5) == 1.0 and E.mcnemar_exact(3, 9) == E.mcnemar_exact(9, 3)


def test_ensemble_report_from_a_reference_block():
    """ensemble_report's host arithmetic on a block built by the reference: accuracies from the confusion matrices,
    means from the sums, oracle accuracy from the histogram, and the diversity as the weighted Jensen-Shannon
    divergence, which is non-negative and equals the direct per-utterance computation."""
    K = 3
    probs, pred, score, labels = mr.cpu_case(K)
    weights = [1.0, 2.0, 1.0]
    r = mr.block(L_, probs, pred, score, labels, weights=weights)
    r["sums"][L_.EM_SUM_SCORE + K] = r["ens_score64"].sum()
    host = np.concatenate([r["counts"], r["sums"].view(np.int64)])
    res = E._models_block(host, weights)
    assert res["K"] == K and res["n"] == len(labels) and res["confusion"].shape == (K + 2, 4, 4)
    rep = E.ensemble_from_block(res)
    lab = labels >= 0
    nl = int(lab.sum())
    assert [m["name"] for m in rep["members"]] == ["model_0", "model_1", "model_2", "ensemble", "vote"]
    for m in range(K + 2):
        acc = float((r["member_pred"][m][lab] == labels[lab]).mean()) * 100
        assert rep["members"][m]["accuracy"] == pytest.approx(acc, abs=1e-9)
    assert "nll" not in rep["members"][K + 1] and "nll" in rep["members"][K]
    ent, nll, brier = mr.terms(probs[1], labels)
    assert rep["members"][1]["nll"] == pytest.approx(nll.sum() / nl, rel=1e-12)
    assert rep["members"][1]["brier"] == pytest.approx(brier.sum() / nl, rel=1e-12)
    assert rep["members"][1]["mean_entropy"] == pytest.approx(ent.mean(), rel=1e-12)
    any_right = (pred[:, lab] == labels[lab][None]).any(0)
    assert rep["oracle_accuracy"] == pytest.approx(float(any_right.mean()) * 100, abs=1e-9)
    assert sum(rep["hist"]) == nl and len(rep["hist"]) == K + 1
    wn = mr.norm_weights(weights, K).astype(np.float64)
    direct = mr.terms(r["ens32"], labels)[0].mean() - sum(wn[k] * mr.terms(probs[k], labels)[0].mean() for k in range(K))
    assert rep["diversity"] == pytest.approx(direct, rel=1e-9) and rep["diversity"] > 0
    assert len(rep["pairs"]) == (K + 2) * (K + 1) // 2
    p01 = rep["pairs"][0]
    assert (p01["a"], p01["b"]) == ("model_0", "model_1")
    assert p01["disagreement_rate"] == pytest.approx(float((pred[0] != pred[1]).mean()))
    b = int(((pred[0] == labels) & (pred[1] != labels) & lab).sum())
    c = int(((pred[1] == labels) & (pred[0] != labels) & lab).sum())
    assert (p01["mcnemar_b"], p01["mcnemar_c"]) == (b, c) and p01["p_value"] == E.mcnemar_exact(b, c)
    best = rep["best_single"]
    assert all(rep["members"][best]["weighted_accuracy"] >= rep["members"][k]["weighted_accuracy"] for k in range(K))
