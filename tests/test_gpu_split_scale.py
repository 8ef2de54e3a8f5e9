"""The store-fed evaluators on the MI355X at a split of 513 utterances with utterances of up to 33 slabs
(tests/split_scale.py: the case, its float64 references and every bound; tests/test_split_scale_cpu.py: the
conditions and the wrong-answer controls).  What no other module runs: a second trip of the result kernels' stride
loops (n > 256) and full LDS trees, waves 1 .. 8 of dad_models_result's ballot loop and a partly filled last wave, a
second block of dad_window_utt, slab_owner over 572 entries with runs of equal ones, heads that sum 10, 11 and 33 slab
partials, and slab pairs deep inside a long utterance and in a table of odd length past 500.

No bound here is measured on a kernel: split_scale.limits (exact_problem.bound, operators_ref's head bound), the
project's 1e-12 on the float64 moments (test_gpu_eval_split._check_block) and (n + 8) 2^-53 sum |terms| on the float64
sums (test_gpu_models).  The module prints every worst error / bound, and one JSON line of them when it is done."""
import functools
import gc
import json

import numpy as np
import pytest
import torch

import attribution_ref as AR
import dadpkg
import exact_problem as X
import gpu_harness as gh
import input_grad_ref as IR
import noise_ref as nr
import split_scale as S
import test_gpu_attribution as TA
import test_gpu_input_grad as TI
import test_gpu_models as TM
import test_gpu_windows as TW
import windows_ref as wr
from test_gpu_eval_split import ALL_S, ALL_T, DTYPES, _check_block

pytestmark = pytest.mark.gpu
PKG = dadpkg.pkg()
D = PKG.data
E = PKG.evaluate
L_ = PKG._lib
CASES = S.NS + ("perm",)
WORST = {}


def _note(test, key, ratio):
    name = "%s/%s" % (test, key)
    WORST[name] = max(WORST.get(name, 0.0), float(ratio))
    return ratio


@functools.lru_cache(None)
def _base(dt):
    feats, sizes, offsets, labels, _ = S.split()
    return D.FeatureStore(feats, sizes, offsets, labels, dtype=DTYPES[dt])


@functools.lru_cache(None)
def _store(dt, case):
    return _base(dt).subset(S.order(case))


@functools.lru_cache(None)
def _flats():
    return tuple(torch.from_numpy(gh.flat(p)).cuda() for p in S.networks())


@functools.lru_cache(None)
def _model():
    model = PKG.SSRLModel().cuda()
    with torch.no_grad():
        model.student_flat.copy_(_flats()[0])
        model.teacher_flat.copy_(_flats()[1])
    return model


@functools.lru_cache(None)
def _noise():
    return torch.from_numpy(S.split()[4]).cuda()


@functools.lru_cache(None)
def _eval(precision, with_teacher, dt, case):
    """One dad_eval_split call: every per-utterance output on the host and the result block; made once per case."""
    res = E.evaluate_store(_model(), _store(dt, case), use_teacher=with_teacher, precision=precision,
                           outputs=ALL_S + (ALL_T if with_teacher else ()))
    return {k: (v.cpu() if torch.is_tensor(v) else v) for k, v in res.items()}


@pytest.fixture(scope="module", autouse=True)
def _report_and_release():
    yield
    print("\nsplit_scale worst error / bound: " + json.dumps(WORST, sort_keys=True))
    torch.cuda.synchronize()
    for f in (_eval, _store, _base, _flats, _model, _noise, _long_stores):
        f.cache_clear()
    gc.collect()
    torch.cuda.synchronize()


# ---- 1. dad_eval_split against float64 -----------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("dt", ["f32", "f16", "bf16"])
@pytest.mark.parametrize("with_teacher", [False, True])
@pytest.mark.parametrize("precision", ["fp32", "fp16"])
def test_eval_split_matches_float64(precision, with_teacher, dt, case):
    store, idx = _store(dt, case), S.order(case)
    sizes, labels = store.sizes, store.labels
    res = _eval(precision, with_teacher, dt, case)
    empty = np.flatnonzero(sizes == 0)
    assert len(empty) >= 5
    tag = "eval_split-%s" % precision
    for k, pre in ((0, ""),) + (((1, "t_"),) if with_teacher else ()):
        ref = S.rows(S.reference(k), idx)
        lim = S.limits(ref, sizes)
        e, z = res[pre + "emb"].numpy(), res[pre + "logits"].numpy()
        e_ratio = _note(tag, pre + "emb", X.worst(e.astype(np.float64) - ref["emb"], lim["emb"]))
        z_ratio = _note(tag, pre + "logits", X.worst(z.astype(np.float64) - ref["logits"], lim["logits"]))
        print("%s %s %s %s%s: worst error / bound: embeddings %.3f, logits %.3f" % (precision, dt, case, pre, "net", e_ratio, z_ratio))
        assert e_ratio <= 1.0 and z_ratio <= 1.0
        pred = res[pre + "pred"].numpy()
        np.testing.assert_array_equal(pred, z.argmax(1))                   # first maximum of its own logits
        ok = S.decided(ref, sizes)
        np.testing.assert_array_equal(pred[ok], ref["pred"][ok])
        assert not e[empty].any()                                          # an empty utterance: 0 and b2, bit for bit
        b2 = np.asarray(S.networks()[k][3], np.float32)
        assert z[empty].tobytes() == np.tile(b2, (len(empty), 1)).tobytes()
    ref = S.rows(S.reference(0), idx)
    lim = S.limits(ref, sizes)
    p_ratio = _note(tag, "probs", X.worst(res["probs"].numpy().astype(np.float64) - ref["probs"], lim["probs"]))
    s_ratio = _note(tag, "score", X.worst(res["score"].numpy().astype(np.float64) - ref["score_entropy"], lim["score"]))
    print("  probs %.3f, score %.3f" % (p_ratio, s_ratio))
    assert p_ratio <= 1.0 and s_ratio <= 1.0
    # the block: from the device's own predictions, and from the float64 ones (every utterance is decided)
    _check_block(res, labels, with_teacher)
    np.testing.assert_array_equal(res["confusion_student"], S.confusion(labels, ref["pred"]))
    lab = (labels >= 0).sum()
    assert (res["n"], res["n_labelled"], res["n_skipped"]) == (len(idx), lab, len(idx) - lab)
    if with_teacher:
        t_pred = S.reference(1)["pred"][idx]
        np.testing.assert_array_equal(res["confusion_teacher"], S.confusion(labels, t_pred))
        assert res["disagree"] == (ref["pred"] != t_pred).sum() > 0


# ---- 2. an utterance's outputs do not depend on the split around it ---------------------------------------------------
@pytest.mark.parametrize("dt", ["f32", "f16", "bf16"])
@pytest.mark.parametrize("with_teacher", [False, True])
@pytest.mark.parametrize("precision", ["fp32", "fp16"])
def test_rows_do_not_depend_on_n_or_on_the_order(precision, with_teacher, dt):
    whole = _eval(precision, with_teacher, dt, 513)
    names = ALL_S + (ALL_T if with_teacher else ())
    for case in (255, 256, 257, "perm"):
        part, idx = _eval(precision, with_teacher, dt, case), torch.from_numpy(S.order(case))
        for k in names:
            assert torch.equal(whole[k][idx].contiguous().view(torch.uint8), part[k].contiguous().view(torch.uint8)), (case, k)


# ---- 3. dad_eval_models ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [257, 513])
@pytest.mark.parametrize("precision", ["fp32", "fp16"])
@pytest.mark.parametrize("K", [3, 8])
def test_models_equal_eval_split_and_the_reference_block(K, precision, n):
    store = _store("f32", n)
    plan = E.EvalPlan.of(store)
    flats = list(_flats()[:K])
    assert plan.n == n and plan.slabs % 2 == (1 if n == 257 else 0)
    res = E.evaluate_models_store(flats, store, precision=precision, outputs=TM.PER_MODEL + TM.PER_UTT)
    got = TM._host(res, TM.PER_MODEL)
    TM._assert_per_model_identity(got, [TM._split_outputs(f, plan, precision) for f in flats])
    ref = TM._check_against_reference(res, store.labels, K, None)          # counts, pair tables, vote, ensemble, sums
    assert res["disagree"][0, 1] > 0 and (ref["votes"].max(1) < K).any() and res["hist"][1:K].sum() > 0
    for k in range(2):                                                   # and the student's / teacher's float64 matrices
        np.testing.assert_array_equal(res["confusion"][k], S.confusion(store.labels, S.reference(k)["pred"][:n]))
    everything = [s[0] for s in TM._SPECS]
    a, ok_a = TM._raw_call(plan, flats, precision, everything)
    b, ok_b = TM._raw_call(plan, flats, precision, everything, ws_fill=0xFF)
    assert ok_a and ok_b                                                  # guard bytes behind every output intact
    for name in everything:
        assert a[name] == b[name], name
    assert res["block"].tobytes() == a["counts"] + a["sums"]
    for name in TM.PER_MODEL:
        assert a[name] == got[name].tobytes(), name


# ---- 4. dad_eval_noise -------------------------------------------------------------------------------------------------
NOISE_OUT = ("emb", "logits", "probs", "score", "pred", "drift", "kl", "break_level")


@pytest.mark.parametrize("precision", ["fp32", "fp16"])
def test_noise_levels_match_float64_and_the_block(precision):
    store = _store("f32", 513)
    sizes, labels, n = store.sizes, store.labels, 513
    res = E.evaluate_noise_store(_model(), store, S.SIGMAS, precision=precision, outputs=NOISE_OUT, noise=_noise())
    ref = S.noise_reference(0)
    frames = np.broadcast_to(sizes, (len(S.SIGMAS), n))
    lim = S.limits(ref, frames)
    e, z = res["emb"].cpu().numpy(), res["logits"].cpu().numpy()
    for k in range(len(S.SIGMAS)):
        e_ratio = _note("noise-%s" % precision, "emb", X.worst(e[k].astype(np.float64) - ref["emb"][k], lim["emb"][k]))
        z_ratio = _note("noise-%s" % precision, "logits", X.worst(z[k].astype(np.float64) - ref["logits"][k], lim["logits"][k]))
        print("%s sigma %g: worst error / bound: embeddings %.3f, logits %.3f" % (precision, S.SIGMAS[k], e_ratio, z_ratio))
        assert e_ratio <= 1.0 and z_ratio <= 1.0
    assert not np.array_equal(ref["emb"][0], ref["emb"][1]) and not np.array_equal(ref["emb"][1], ref["emb"][2])
    pred = res["pred"].cpu().numpy()
    np.testing.assert_array_equal(pred, z.argmax(-1))
    ok = S.decided(ref, frames)
    np.testing.assert_array_equal(pred[ok], ref["pred"][ok])
    whole = _eval(precision, False, "f32", 513)                            # level 0 is the split evaluator
    for name in ("emb", "logits", "probs", "score", "pred"):
        assert torch.equal(res[name][0].cpu().contiguous().view(torch.uint8), whole[name].contiguous().view(torch.uint8)), name
    vals = [res[name].cpu().numpy() for name in ("score", "drift", "kl")]
    np.testing.assert_array_equal(res["break_level"].cpu().numpy().astype(np.int64), nr.break_level(pred))
    counts, sums = nr.block(L_, pred, vals[0], vals[1], vals[2], labels)
    np.testing.assert_array_equal(res["block"][:L_.EN_COUNTS], counts)
    got = res["block"][L_.EN_COUNTS:].view(np.float64)
    K = len(S.SIGMAS)
    for name, slot, v in zip(("score", "drift", "kl"), (L_.EN_SUM_SCORE, L_.EN_SUM_DRIFT, L_.EN_SUM_KL), vals):
        ratio = _note("noise-%s" % precision, "sum_" + name, X.worst(got[slot:slot + K] - sums[slot:slot + K], S.sum_limit(v, n)))
        print("%s sum of %s: worst error / bound %.3f" % (precision, name, ratio))
        assert ratio <= 1.0 and not got[slot + K:slot + L_.EN_MAX_LEVELS].any()
    assert res["flips"][0] == 0 and res["flips"][2] > 0 and res["survive"][0] == n
    for k in range(K):                                                   # every utterance is decided at every level
        np.testing.assert_array_equal(res["confusion"][k], S.confusion(labels, ref["pred"][k]))


# ---- 5. dad_eval_windows -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [257, 513])
@pytest.mark.parametrize("precision", ["fp32", "fp16"])
@pytest.mark.parametrize("hop,span,mode", S.WINDOW_CASES, ids=["%s-h%d-m%d" % (m, h, s) for h, s, m in S.WINDOW_CASES])
def test_windows_match_float64_and_the_summaries(hop, span, mode, precision, n):
    store = _store("f32", n)
    res = E.evaluate_windows_store(_model(), store, hop, span, mode, precision=precision, outputs=TW.ALL)
    full = S.windows_reference(hop, span, mode)
    off = full["win_off"][:n + 1]
    nw = int(off[-1])
    np.testing.assert_array_equal(res["win_off"], off)
    ref = {k: full[k][:nw] for k in ("emb", "logits", "logit_mag", "probs", "score_entropy", "pred", "gap", "frames")}
    lim = S.limits(ref, ref["frames"])
    e, z = res["w_emb"].cpu().numpy(), res["w_logits"].cpu().numpy()
    assert e.shape == (nw, 256) and (ref["emb"] >= 0).all() and ref["frames"].min() >= 1
    tag = "windows-%s" % precision
    e_ratio = _note(tag, "w_emb", X.worst(e.astype(np.float64) - ref["emb"], lim["emb"]))
    z_ratio = _note(tag, "w_logits", X.worst(z.astype(np.float64) - ref["logits"], lim["logits"]))
    print("%s %s (%d, %d) n = %d: worst error / bound: embeddings %.3f, logits %.3f" % (precision, mode, hop, span, n, e_ratio, z_ratio))
    assert e_ratio <= 1.0 and z_ratio <= 1.0
    pred = res["w_pred"].cpu().numpy()
    np.testing.assert_array_equal(pred, z.argmax(1))
    ok = lim["decided"]
    assert (~ok).mean() <= 0.05                                           # windows_ref.decided's cap
    np.testing.assert_array_equal(pred[ok], ref["pred"][ok])
    s = TW._check_summaries(res, store.sizes, store.labels, hop, span, mode)   # per-utterance outputs and the block
    assert res["n"] == n and res["n_empty"] == (store.sizes == 0).sum() and res["n_windows"] == nw
    if n == 513:
        assert s["J"][259] == len(wr.windows_brute(1025, hop, span, mode)) and (s["J"][259] > L_.EW_CURVE) == (hop == 1)
    if (hop, mode) == (32, "prefix"):                                      # a piece is a slab: the last prefix is dad_eval_split
        whole = _eval(precision, False, "f32", n)
        live = np.flatnonzero(np.diff(off) > 0)
        last = torch.from_numpy(off[1:][live].astype(np.int64) - 1)
        for mine, theirs in (("w_emb", "emb"), ("w_logits", "logits"), ("w_pred", "pred")):
            assert torch.equal(res[mine].cpu()[last].contiguous().view(torch.uint8),
                               whole[theirs][torch.from_numpy(live)].contiguous().view(torch.uint8)), mine
        assert torch.equal(res["last_pred"].cpu()[torch.from_numpy(live)].long(), whole["pred"][torch.from_numpy(live)])


# ---- 6. dad_input_grad and dad_attribution on the long utterances alone ------------------------------------------------
LONG_SIZES = tuple(int(S.FIXED[i]) for i in S.LONG)


@functools.lru_cache(None)
def _long_stores(which):
    """The 331-, 1025- and 300-frame utterances on the reference module's own exact grid (its weights' grid differs
    between the two operators): (problem, model, store)."""
    R, T = (IR, TI) if which == "input_grad" else (AR, TA)
    prob = R.exact_problem(LONG_SIZES)
    feats, sizes, offsets, params = prob[:4]
    return prob, T._model_of(params), D.FeatureStore(feats, sizes, offsets, np.arange(len(sizes)) % 4)


@pytest.mark.parametrize("precision", ["fp32", "fp16"])
def test_input_grad_on_the_long_utterances(precision):
    """test_gpu_input_grad.test_exact_grid's assertions (input_grad_ref.exact_failures: (H + 4) u S, fp16 + 2^-11 S,
    frame_l1 within 768 u) where an utterance has 10, 11 and 33 slabs."""
    (feats, sizes, offsets, params, dz, delta), model, store = _long_stores("input_grad")
    assert tuple(sizes) == (331, 1025, 300)
    for kw in (dict(alpha=0.25), dict(delta=delta, alpha=0.25, radius=0.5)):
        got = TI._run(model, store, dz, precision=precision, **kw)
        ref = IR.reference(feats, sizes, offsets, params, dz, kw.get("delta"), kw["alpha"], kw.get("radius", np.inf))
        fails = IR.exact_failures(got, ref, sizes, fp16=precision == "fp16")
        ratio = _note("input_grad-%s" % precision, "grad", IR.check_grad(got["grad"], ref, sizes, fp16=precision == "fp16")[0])
        print("%s: worst gradient error / bound %.3f" % (precision, ratio))
        assert not fails, fails
        v = IR.valid_rows(sizes)
        np.testing.assert_array_equal(got["counts"], [sizes.sum(), 0, int((got["grad"][v] == 0).sum()), 0])


@pytest.mark.parametrize("precision", ["fp32", "fp16"])
def test_attribution_on_the_long_utterances(precision):
    """test_gpu_attribution.test_exact_grid's assertions (attribution_ref.check) where chan_attr and utt_total sum
    over 10, 11 and 33 slabs."""
    (feats, sizes, offsets, params, dz, xb), model, store = _long_stores("attribution")
    for bname, b in (("zero", None), ("grid", xb)):
        ref = AR.reference(feats, sizes, offsets, params, dz, b)
        got = TA._run(model, store, dz, b, precision, prefill=True)
        ratios, fails = AR.check(got, ref, sizes, fp16=precision == "fp16")
        print("%s baseline %s: worst error / bound %s" % (precision, bname, ratios))
        for k, r in (ratios.items() if isinstance(ratios, dict) else ()):
            _note("attribution-%s" % precision, k, r)
        assert not fails, (bname, fails)
