"""Noise response of a split on the MI355X (evaluate.py *noise* + csrc/eval_noise.hip): every level against the
float64 reference of tests/noise_ref.py in explicit-noise mode (bounds and their sources: its docstring), the
per-utterance comparisons and the DAD_EN_* block against NumPy on the kernel's own outputs, a derived bound on
exactly representable operands, the reference model's golden numbers, the counter RNG (probe equality, independence,
moments), the bit-level identities of the design, the edges and error paths, and the Python surface."""
import functools
import gc
import math
import os

import numpy as np
import pytest
import torch

import dadpkg
import exact_problem as X
import noise_ref as nr
from golden.gen_noise_golden import SIGMAS as GOLDEN_SIGMAS, inputs as golden_inputs, slab_aligned
from oracle import data_oracle as do
from test_gpu_eval_split import _inputs, _model, _store

pytestmark = pytest.mark.gpu
PKG = dadpkg.pkg()
D = PKG.data
E = PKG.evaluate
L_ = PKG._lib

PER_LEVEL = ("emb", "logits", "probs", "score", "pred", "drift", "kl")
ALL = PER_LEVEL + ("break_level",)
SPLIT = ("emb", "logits", "probs", "score", "pred")


def _np(t):
    return t.cpu().numpy()


def _bits(t):
    return t.contiguous().reshape(-1).view(torch.uint8)


@functools.lru_cache(None)
def _main_noise():
    return torch.from_numpy(nr.main_inputs()[5]).cuda()


def _fresh_model(seed):
    """test_gpu_eval_split._model's weights for another seed, not kept in its cache."""
    stu, tea = do.eval_weights(seed)
    flat = lambda ps: torch.from_numpy(np.concatenate([np.asarray(a, np.float32).reshape(-1) for a in ps]))
    model = PKG.SSRLModel().cuda()
    with torch.no_grad():
        model.student_flat.copy_(flat(stu))
        model.teacher_flat.copy_(flat(tea))
    return model


@pytest.fixture(scope="module", autouse=True)
def _release_device_memory():
    """The module keeps nothing on the device once it is done: its own cached tensors, and the noise buffers it
    left on the plans of the stores it shares with the other evaluator modules."""
    yield
    torch.cuda.synchronize()
    _main_noise.cache_clear()
    _exact.cache_clear()
    for which, dt in (("main", "f32"), ("main", "f16"), ("main", "bf16"), ("single", "f32")):
        plan = getattr(_store(which, dt), "_eval_plan", None)
        if plan is not None:
            plan._noise.clear()
    gc.collect()
    torch.cuda.synchronize()


def _check_values(res, ref, use_entropy=True):
    np.testing.assert_allclose(_np(res["emb"]), ref["emb"], rtol=1e-5, atol=1e-4)
    np.testing.assert_allclose(_np(res["logits"]), ref["logits"], rtol=1e-5, atol=1e-4)
    np.testing.assert_allclose(_np(res["probs"]), ref["probs"], rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(_np(res["score"]), ref["score_entropy" if use_entropy else "score_max"],
                               rtol=1e-5, atol=1e-6)
    drift_err = np.abs(_np(res["drift"]).astype(np.float64) - ref["drift"]).max()
    kl_ratio = X.worst(_np(res["kl"]).astype(np.float64) - ref["kl"], ref["kl_lim"])
    print("drift error %.3e of %.3e allowed; kl worst error / bound %.3f" % (drift_err, nr.drift_lim(ref["emb"]), kl_ratio))
    assert drift_err <= nr.drift_lim(ref["emb"])
    assert kl_ratio <= 1.0


def _check_preds(res, ref, min_gap=nr.GAP):
    pred = _np(res["pred"])
    np.testing.assert_array_equal(pred, _np(res["logits"]).argmax(-1))        # first maximum
    ok = nr.decided(ref, min_gap)
    np.testing.assert_array_equal(pred[ok], ref["pred"][ok])


def _check_block(res, labels):
    """break_level and the block against the NumPy restatement from the kernel's own per-utterance outputs."""
    pred = _np(res["pred"])
    vals = [_np(res[k]) for k in ("score", "drift", "kl")]
    K, n = pred.shape
    np.testing.assert_array_equal(_np(res["break_level"]).astype(np.int64), nr.break_level(pred))
    counts, sums = nr.block(L_, pred, vals[0], vals[1], vals[2], labels)
    np.testing.assert_array_equal(res["block"][:L_.EN_COUNTS], counts)
    got = res["block"][L_.EN_COUNTS:].view(np.float64)
    for slot, v in zip((L_.EN_SUM_SCORE, L_.EN_SUM_DRIFT, L_.EN_SUM_KL), vals):
        mag = np.abs(v.astype(np.float64)).sum(1)
        assert (np.abs(got[slot:slot + K] - sums[slot:slot + K]) <= n * 2.0 ** -53 * mag).all(), slot
        assert not got[slot + K:slot + L_.EN_MAX_LEVELS].any()
    assert res["n"] == n and res["n_levels"] == K and res["n_nonfinite"] == 0
    for k, lv in enumerate(res["levels"]):
        assert lv["flip_rate"] == (pred[k] != pred[0]).mean()
        assert lv["survival"] == (nr.break_level(pred) > k).mean()
        assert lv["mean_kl"] == got[L_.EN_SUM_KL + k] / n and lv["mean_drift"] == got[L_.EN_SUM_DRIFT + k] / n
        assert lv["mean_score"] == got[L_.EN_SUM_SCORE + k] / n
        if labels is not None:
            lab = labels >= 0
            assert lv["accuracy"] == pytest.approx(100.0 * (pred[k][lab] == labels[lab]).mean(), abs=1e-9)


# ---- 1. fp32 against float64, explicit noise ------------------------------------------------------------------
@pytest.mark.parametrize("net", ["s", "t"])
@pytest.mark.parametrize("sigmas", [nr.LEVELS4, (0.05,), nr.LEVELS8], ids=["K4", "K1", "K8"])
def test_fp32_matches_float64(sigmas, net):
    store = _store("main", "f32")
    ref = nr.main_reference("f32", net, sigmas)
    res = E.evaluate_noise_store(_model(), store, sigmas, use_teacher=net == "t", outputs=ALL, noise=_main_noise())
    _check_values(res, ref)
    _check_preds(res, ref)
    _check_block(res, store.labels)
    assert res["n"] == 39 and res["n_labelled"] == 37 and res["n_skipped"] == 2
    if len(sigmas) > 1:
        assert res["flips"][-1] > 0 and res["flips"][0] == 0 and res["survive"][0] == 39


# ---- 2. 16-bit stores and fp16 operands -----------------------------------------------------------------------
@pytest.mark.parametrize("use_entropy", [True, False])
@pytest.mark.parametrize("dt", ["f16", "bf16"])
def test_16bit_stores_match_float64_on_the_widened_values(dt, use_entropy):
    store = _store("main", dt)
    ref = nr.main_reference(dt, "s", nr.LEVELS4)
    res = E.evaluate_noise_store(_model(), store, nr.LEVELS4, use_entropy=use_entropy, outputs=ALL, noise=_main_noise())
    _check_values(res, ref, use_entropy)
    _check_preds(res, ref)
    _check_block(res, store.labels)


@pytest.mark.parametrize("dt", ["f32", "f16", "bf16"])
def test_fp16_operands_match_their_float64_simulation(dt):
    """FP16 operand mode against float64 on fp16-rounded rows, noise and W1: only the accumulation differs, so the
    fp32 tolerances hold; predictions on cells whose gap exceeds twice the logit tolerance."""
    store = _store("main", dt)
    for net in "st":
        ref = nr.main_reference(dt, net, nr.LEVELS4, True)
        res = E.evaluate_noise_store(_model(), store, nr.LEVELS4, use_teacher=net == "t", precision="fp16", outputs=ALL,
                                     noise=_main_noise())
        _check_values(res, ref)
        _check_preds(res, ref, 2 * (1e-4 + 1e-5 * float(np.abs(ref["logits"]).max())))
        _check_block(res, store.labels)


# ---- 3. derived bound on exact operands -----------------------------------------------------------------------
EXACT_SIGMAS = (0.0, 0.125, 0.25, 0.5, 1.0)


@functools.lru_cache(None)
def _exact():
    """Features, noise and weights on tests/exact_problem.py's dyadic grid: lengths 1, 33, 65."""
    sizes = np.array([1, 33, 65])
    offsets = np.concatenate([[0], np.cumsum(sizes)[:-1]])
    feats = X.q(np.clip(4.0 * np.random.RandomState(5).standard_normal((int(sizes.sum()), 768)), -16, 16), 2.0 ** -3)
    slabs = int(nr.slab_prefix(sizes)[-1])
    noise = np.random.RandomState(6).randint(-3, 4, (32 * slabs, 768)).astype(np.float32)
    st = X.state()
    model = PKG.SSRLModel().cuda()
    flat = lambda ps: torch.from_numpy(np.concatenate([np.asarray(a, np.float32).reshape(-1) for a in ps]))
    with torch.no_grad():
        model.student_flat.copy_(flat(st["student"]))
        model.teacher_flat.copy_(flat(st["teacher"]))
    refs = {name: nr.forward64(feats, noise, sizes, offsets, np.arange(3), EXACT_SIGMAS, st[name])
            for name in ("student", "teacher")}
    return feats, noise, sizes, offsets, model, refs


@pytest.mark.parametrize("precision", ["fp32", "fp16"])
def test_derived_bound_on_exact_operands(precision):
    """On the dyadic grid every pre-activation x W1 + sigma n W1 + b1 is an exact odd multiple of 2^-14 in both operand
    modes, so |e - e_ref| <= (T + 2) u |e_ref| and the logits (T + H + 8) u times their magnitude sum: no measured
    number."""
    feats, noise, sizes, offsets, model, refs = _exact()
    store = D.FeatureStore(feats, sizes, offsets, np.array([0, 1, 2]))
    T = sizes.astype(np.float64)[:, None]
    for name in ("student", "teacher"):
        ref = refs[name]
        res = E.evaluate_noise_store(model, store, EXACT_SIGMAS, use_teacher=name == "teacher", precision=precision,
                                     outputs=("emb", "logits"), noise=torch.from_numpy(noise).cuda())
        assert (ref["emb"] >= 0).all() and ref["emb"].max() > 0
        assert not np.array_equal(ref["emb"][0], ref["emb"][-1])
        e_ratio = X.worst(_np(res["emb"]).astype(np.float64) - ref["emb"], X.bound("e", None, T) * np.abs(ref["emb"]))
        z_ratio = X.worst(_np(res["logits"]).astype(np.float64) - ref["logits"], X.bound("z", None, T) * ref["logit_mag"])
        print("%s %s: worst error / bound: embeddings %.3f, logits %.3f" % (precision, name, e_ratio, z_ratio))
        assert e_ratio <= 1.0 and z_ratio <= 1.0


# ---- 4. golden ------------------------------------------------------------------------------------------------
def test_golden_levels_of_the_reference_model():
    """SSRLModel.get_embeddings / predict on x + sigma n (tests/golden/eval_noise.npz), at the project's parity bound:
    max |got - ref| <= 1e-4 max |ref|."""
    g = np.load(os.path.join(dadpkg.ROOT, "tests", "golden", "eval_noise.npz"))
    feats, noise, sizes, offsets = golden_inputs()
    store = D.FeatureStore(feats, sizes, offsets, None)
    res = E.evaluate_noise_store(_fresh_model(int(g["seed"])), store, GOLDEN_SIGMAS, outputs=("emb", "logits", "pred"),
                                 noise=torch.from_numpy(slab_aligned(noise, sizes, offsets)).cuda())
    for k in ("emb", "logits"):
        err = np.abs(_np(res[k]).astype(np.float64) - g[k]).max() / np.abs(g[k]).max()
        print("golden %s: max-abs error over max |ref| %.3e" % (k, err))
        assert err <= 1e-4
    top = np.sort(g["logits"].astype(np.float64), -1)
    ok = top[..., -1] - top[..., -2] > nr.GAP
    assert ok.mean() >= 0.95
    np.testing.assert_array_equal(_np(res["pred"])[ok], g["pred"][ok])
    assert res["n_labelled"] == 0 and res["n_skipped"] == len(sizes) and not res["confusion"].any()
    assert "accuracy" not in res["levels"][0]


# ---- 5. counter mode ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["fp32", "fp16"])
@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_counter_call_equals_explicit_call_on_the_probe(dt, precision):
    model, store = _model(), _store("main", dt)
    plan = E.EvalPlan.of(store)
    for seed, draw in ((0, 0), (7, 3)):
        z = E.noise_draws(plan, seed, draw)
        a = E.evaluate_noise_store(model, store, nr.LEVELS4, seed=seed, draw=draw, precision=precision, outputs=ALL)
        b = E.evaluate_noise_store(model, store, nr.LEVELS4, precision=precision, outputs=ALL, noise=z)
        assert a["block"].tobytes() == b["block"].tobytes()
        for k in ALL:
            assert torch.equal(_bits(a[k]), _bits(b[k])), (seed, draw, k)
        assert a["flips"][-1] >= 0 and float(a["sum_drift"][-1]) > 0


def _utt_rows(z, soff, j, L):
    return z[32 * int(soff[j]):32 * int(soff[j]) + int(L)]


def test_counter_draws_depend_on_seed_draw_utterance_only():
    feats, sizes, offsets, labels, order = _inputs("main")
    store = _store("main", "f32")
    plan = E.EvalPlan.of(store)
    sub = sizes[order]
    soff = nr.slab_prefix(sub)
    z = E.noise_draws(plan, 5, 2)
    assert z.shape == (32 * plan.slabs, 768)
    assert torch.equal(z, E.noise_draws(plan, 5, 2))
    assert not torch.equal(z, E.noise_draws(plan, 5, 3)) and not torch.equal(z, E.noise_draws(plan, 6, 2))
    for first, again in ((3, 30), (11, 31)):                      # two utterances on the same store rows
        assert order[first] == order[again] and sub[first] > 0
        assert not torch.equal(_utt_rows(z, soff, first, sub[first]), _utt_rows(z, soff, again, sub[first]))
    valid = torch.zeros(32 * plan.slabs, dtype=torch.bool)
    for j, L in enumerate(sub):
        valid[32 * int(soff[j]):32 * int(soff[j]) + int(L)] = True
    assert not z[~valid.cuda()].any()                              # rows past an utterance's length: zeros
    # utterance i's draws when the other utterances change: the call's first i + 1 utterances alone, and the others
    # in another order (other lengths before it, so another slab assignment and other store rows)
    base = D.FeatureStore(feats, sizes, offsets, labels)
    for i in (4, 17, 38):
        head = base.subset(order[:i + 1])
        zh = E.noise_draws(E.EvalPlan.of(head), 5, 2)
        assert torch.equal(_utt_rows(zh, nr.slab_prefix(sub[:i + 1]), i, sub[i]), _utt_rows(z, soff, i, sub[i]))
        perm = np.random.RandomState(i).permutation(len(order))
        perm = np.concatenate([perm[perm != i][:i], [i], perm[perm != i][i:]])
        assert perm[i] == i and (perm != np.arange(len(order))).any()
        other = base.subset(order[perm])
        zo = E.noise_draws(E.EvalPlan.of(other), 5, 2)
        assert torch.equal(_utt_rows(zo, nr.slab_prefix(sub[perm]), i, sub[i]), _utt_rows(z, soff, i, sub[i]))
    # moments of one probe, at its sample count, as tests/test_gpu_rng.py holds the step's noise streams
    v = _np(z[valid.cuda()]).astype(np.float64).ravel()
    n = v.size
    assert n == int(sub.sum()) * 768
    assert abs(v.mean()) < 5.0 / math.sqrt(n), v.mean()
    assert abs(v.std() - 1.0) < 5.0 * math.sqrt(0.5 / n) + 1e-4, v.std()
    assert np.abs(v).max() < 4.72


# ---- 6. identities --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("net", ["s", "t"])
@pytest.mark.parametrize("dt", ["f32", "f16", "bf16"])
@pytest.mark.parametrize("precision", ["fp32", "fp16"])
def test_zero_levels_are_the_split_evaluator_bit_for_bit(precision, dt, net):
    model, store = _model(), _store("main", dt)
    whole = E.evaluate_store(model, store, use_teacher=True, precision=precision,
                             outputs=("emb", "logits", "probs", "score", "pred", "t_emb", "t_logits", "t_pred"))
    if net == "t":                              # the split evaluator reports the teacher's probs / score as a student
        swapped = PKG.SSRLModel().cuda()
        with torch.no_grad():
            swapped.student_flat.copy_(model.teacher_flat)
            swapped.teacher_flat.copy_(model.student_flat)
        as_student = E.evaluate_store(swapped, store, precision=precision, outputs=SPLIT)
        for k in ("emb", "logits", "pred"):
            assert torch.equal(_bits(as_student[k]), _bits(whole["t_" + k])), k
        whole = as_student
    sig = (0.0, 0.05, 0.0, 0.25)
    for kw in (dict(noise=_main_noise()), dict(seed=3, draw=1)):
        res = E.evaluate_noise_store(model, store, sig, use_teacher=net == "t", precision=precision, outputs=ALL, **kw)
        for level in (0, 2):
            for k in SPLIT:
                assert torch.equal(_bits(res[k][level]), _bits(whole[k])), (level, k)
        assert not res["drift"][2].any() and not res["kl"][2].any() and res["flips"][2] == 0
        assert not torch.equal(res["emb"][1], res["emb"][0])


@pytest.mark.parametrize("precision", ["fp32", "fp16"])
def test_duplicate_levels_and_repeated_calls_write_identical_bits(precision):
    model, store = _model(), _store("main", "f32")
    a = E.evaluate_noise_store(model, store, nr.LEVELS8, precision=precision, outputs=ALL, noise=_main_noise())
    E.evaluate_noise_store(model, store, nr.LEVELS4, precision=precision, seed=1)      # another K between
    b = E.evaluate_noise_store(model, store, nr.LEVELS8, precision=precision, outputs=ALL, noise=_main_noise())
    assert a["block"].tobytes() == b["block"].tobytes()
    for k in ALL:
        assert a[k].data_ptr() != b[k].data_ptr()
        assert torch.equal(_bits(a[k]), _bits(b[k])), k
    for k in PER_LEVEL:
        assert torch.equal(_bits(a[k][3]), _bits(a[k][4])), k      # sigma 0.25 twice
        assert torch.equal(_bits(a[k][0]), _bits(a[k][6])), k      # sigma 0 twice
    assert a["flips"][3] == a["flips"][4] and a["sum_kl"][3] == a["sum_kl"][4]


def test_outputs_do_not_depend_on_the_subset_order():
    """With each utterance's explicit noise moved along with it, its outputs are the same bits wherever it stands
    in the subset; the two samples that the subset repeats, given the same noise, give equal rows."""
    feats, sizes, offsets, labels, order, noise = nr.main_inputs()
    model, a_store = _model(), _store("main", "f32")
    sub = sizes[order]
    soff = nr.slab_prefix(sub)
    noise = noise.copy()
    for first, again in ((3, 30), (11, 31)):
        noise[32 * soff[again]:32 * soff[again] + sub[again]] = noise[32 * soff[first]:32 * soff[first] + sub[first]]
    perm = np.random.RandomState(3).permutation(len(order))
    boff = nr.slab_prefix(sub[perm])
    moved = np.zeros_like(noise)
    for ib, ia in enumerate(perm):
        moved[32 * boff[ib]:32 * boff[ib] + sub[ia]] = noise[32 * soff[ia]:32 * soff[ia] + sub[ia]]
    b_store = D.FeatureStore(feats, sizes, offsets, labels).subset(order[perm])
    a = E.evaluate_noise_store(model, a_store, nr.LEVELS4, outputs=ALL, noise=torch.from_numpy(noise).cuda())
    b = E.evaluate_noise_store(model, b_store, nr.LEVELS4, outputs=ALL, noise=torch.from_numpy(moved).cuda())
    idx = torch.from_numpy(perm).cuda()
    for k in PER_LEVEL:
        assert torch.equal(_bits(a[k][:, idx]), _bits(b[k])), k
    assert torch.equal(a["break_level"][idx], b["break_level"])
    np.testing.assert_array_equal(a["confusion"], b["confusion"])          # (the float64 sums depend on the order)
    np.testing.assert_array_equal(a["flips"], b["flips"])
    for first, again in ((3, 30), (11, 31)):
        for k in PER_LEVEL:
            assert torch.equal(_bits(a[k][:, first]), _bits(a[k][:, again])), k


def test_captured_call_replays_the_eager_result():
    model, store = _model(), _store("main", "f32")
    plan = E.EvalPlan.of(store)
    eager = E.evaluate_noise_store(model, store, nr.LEVELS4, seed=2, draw=5, outputs=("logits", "kl", "break_level"))
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = E.enqueue_eval_noise(model, plan, nr.LEVELS4, seed=2, draw=5, outputs=("logits", "kl", "break_level"))
    b = E._noise_buffers(plan, 4)
    b["result_d"].zero_()
    g.replay()
    torch.cuda.synchronize()
    assert b["result_d"].cpu().numpy().tobytes() == eager["block"].tobytes()
    for k in ("logits", "kl", "break_level"):
        assert torch.equal(_bits(out[k]), _bits(eager[k])), k


# ---- 7. edges -------------------------------------------------------------------------------------------------
def test_single_utterance_and_empty_utterance():
    model = _model()
    single = _store("single", "f32")
    feats, sizes, offsets, _, order = _inputs("single")
    noise = np.random.RandomState(8).standard_normal((32, 768)).astype(np.float32)
    ref = nr.forward64(feats, noise, sizes, offsets, order, nr.LEVELS4, do.eval_weights(11)[0])
    res = E.evaluate_noise_store(model, single, nr.LEVELS4, outputs=ALL, noise=torch.from_numpy(noise).cuda())
    assert res["n"] == 1 and res["emb"].shape == (4, 1, 256)
    _check_values(res, ref)
    _check_block(res, single.labels)
    # the length-0 utterance of the main split
    store = _store("main", "f32")
    i0 = int(np.where(store.sizes == 0)[0][0])
    b2 = np.asarray(do.eval_weights(11)[0][3], np.float32)
    for kw in (dict(noise=_main_noise()), dict(seed=1)):
        r = E.evaluate_noise_store(model, store, nr.LEVELS8, outputs=ALL, **kw)
        assert not r["emb"][:, i0].any() and not r["drift"][:, i0].any() and not r["kl"][:, i0].any()
        np.testing.assert_array_equal(_np(r["logits"][:, i0]), np.tile(b2, (8, 1)))
        assert int(r["break_level"][i0]) == 8


def test_unlabelled_split():
    feats, sizes, offsets, _, order = _inputs("main")
    store = D.FeatureStore(feats, sizes, offsets, None).subset(order)
    res = E.evaluate_noise_store(_model(), store, nr.LEVELS4, outputs=ALL, noise=_main_noise())
    _check_block(res, None)
    assert res["n_labelled"] == 0 and res["n_skipped"] == 39 and not res["confusion"].any()
    with pytest.raises(ValueError, match="no labels"):
        E.noise_response_curve(_model(), store, draws=1)


def test_nonfinite_features_are_counted_and_raise():
    rs = np.random.RandomState(3)
    sizes = np.array([5, 40, 2, 33, 7])
    offsets = np.concatenate([[0], np.cumsum(sizes)[:-1]])
    feats = rs.standard_normal((int(sizes.sum()), 768)).astype(np.float32)
    labels = np.array([0, 1, 2, 3, 0])
    assert E.evaluate_noise_store(_model(), D.FeatureStore(feats, sizes, offsets, labels), nr.LEVELS4)["n_nonfinite"] == 0
    feats[offsets[3] + 32, 100] = np.nan        # a NaN in the data: the last frame of utterance 3
    store = D.FeatureStore(feats, sizes, offsets, labels)
    with pytest.raises(L_.DadError, match="1 of 5 utterance"):
        E.evaluate_noise_store(_model(), store, nr.LEVELS4)
    plan = E.EvalPlan.of(store)
    out = E.enqueue_eval_noise(_model(), plan, nr.LEVELS4, outputs=("logits",))
    torch.cuda.synchronize()
    blk = E._noise_buffers(plan, 4)["result_d"].cpu().numpy()
    assert blk[L_.EN_N_NONFINITE] == 1 and blk[L_.EN_N] == 5
    bad = ~torch.isfinite(out["logits"]).all(-1)
    assert bad[:, 3].all() and not bad[:, [0, 1, 2, 4]].any()


def _raw_args(model, plan, block):
    a = L_.DadNoiseArgs()
    a.store = plan.store.feats.data_ptr()
    a.rows, a.lens, a.slab_off = plan.rows_d.data_ptr(), plan.lens_d.data_ptr(), plan.slab_off_d.data_ptr()
    a.labels = plan.labels_d.data_ptr()
    a.params = model.student_flat.data_ptr()
    a.counts, a.sums = block.data_ptr(), block.data_ptr() + 8 * L_.EN_COUNTS
    a.n, a.slabs, a.levels = plan.n, plan.slabs, 4
    a.sigma[:4] = list(nr.LEVELS4)
    a.store_dtype, a.use_entropy, a.precision = L_.STORE_F32, 1, L_.PREC_FP32
    return a


def test_error_paths_launch_nothing():
    model, store = _model(), _store("main", "f32")
    plan = E.EvalPlan.of(store)
    E.evaluate_noise_store(model, store, nr.LEVELS4)               # (builds the buffers and the workspace)
    b = E._noise_buffers(plan, 4)
    fn = L_.lib().dad_eval_noise
    stream = torch.cuda.current_stream().cuda_stream
    b["result_d"].fill_(-7)

    def call(**change):
        a = _raw_args(model, plan, b["result_d"])
        for k, v in change.items():
            if k == "sigma":
                a.sigma[v[0]] = v[1]
            else:
                setattr(a, k, v)
        return fn(a, L_.ptr(b["ws"]), stream)

    for name in ("store", "rows", "lens", "slab_off", "params", "counts", "sums"):
        assert call(**{name: None}) == L_.E_ARG, name
    assert fn(_raw_args(model, plan, b["result_d"]), None, stream) == L_.E_ARG
    assert call(levels=0) == L_.E_ARG
    assert call(levels=9) == L_.E_ARG
    assert call(sigma=(1, -0.01)) == L_.E_ARG
    assert call(sigma=(3, float("nan"))) == L_.E_ARG
    assert call(sigma=(0, float("inf"))) == L_.E_ARG
    assert call(store_dtype=3) == L_.E_ARG
    assert call(precision=7) == L_.E_ARG
    assert call(precision=L_.PREC_BF16) == L_.E_UNSUPPORTED
    assert call(n=0) == L_.E_SHAPE
    assert call(slabs=-1) == L_.E_SHAPE
    assert call(slabs=2 ** 21) == L_.E_SHAPE                       # 2^21 * 4 * 256 = 2^31
    torch.cuda.synchronize()
    assert (b["result_d"] == -7).all()                            # nothing ran
    with pytest.raises(L_.DadError, match="DAD_E_UNSUPPORTED"):
        E.evaluate_noise_store(model, store, nr.LEVELS4, precision="bf16")
    with pytest.raises(ValueError):
        E.evaluate_noise_store(model, store, ())
    with pytest.raises(ValueError):
        E.evaluate_noise_store(model, store, (0.0, -0.1))
    with pytest.raises(ValueError, match="unknown output"):
        E.evaluate_noise_store(model, store, nr.LEVELS4, outputs=("w_emb",))
    with pytest.raises(ValueError, match="noise must be"):
        E.evaluate_noise_store(model, store, nr.LEVELS4, noise=_main_noise()[:-32])
    assert call() == 0                                            # and the unchanged arguments run
    torch.cuda.synchronize()
    assert int(b["result_d"][L_.EN_N]) == 39 and int(b["result_d"][L_.EN_LEVELS]) == 4


# ---- 8. the Python surface ------------------------------------------------------------------------------------
def test_response_curve_and_report_on_two_small_stores():
    feats, sizes, offsets, labels, order = _inputs("main")
    model, noisy = _model(), _store("main", "f32")
    clean = D.FeatureStore(feats, sizes, offsets, labels)          # 37 utterances, store order
    sig = (0.0, 0.25, 1.0, 4.0)
    for store in (clean, noisy):
        curve = E.noise_response_curve(model, store, sig, draws=3, seed=4)
        singles = [E.evaluate_noise_store(model, store, sig, seed=4, draw=d, outputs=("pred",)) for d in range(3)]
        for name, key in (("accuracy", "accuracy"), ("balanced_accuracy", "weighted_accuracy"),
                          ("flip_rate", "flip_rate"), ("mean_kl", "mean_kl")):
            v = np.array([[r["levels"][k][key] for k in range(4)] for r in singles])
            np.testing.assert_allclose(curve[name]["mean"], v.mean(0), rtol=1e-12, atol=0)
            np.testing.assert_allclose(curve[name]["std"], v.std(0), rtol=1e-12, atol=1e-15)
        for d in range(3):
            assert curve["per_draw"][d]["block"].tobytes() == singles[d]["block"].tobytes()
        preds = np.stack([_np(r["pred"]) for r in singles])           # [3, K, n]
        count = (preds != preds[:, 0:1]).sum(0)
        assert curve["flip_prob"].is_cuda and curve["flip_prob"].shape == (4, len(store.sizes))
        np.testing.assert_allclose(_np(curve["flip_prob"]), count / 3.0, rtol=1e-6, atol=0)
        assert not _np(curve["flip_prob"])[0].any() and count[-1].sum() > 0
        assert curve["sigmas"] == list(sig) and curve["draws"] == 3
    default = E.noise_response_curve(model, noisy, draws=1)
    assert default["sigmas"] == [0.0, PKG.FLAVOR_DEFAULTS["iemocap"]["WEAK_NOISE_STD"],
                                 PKG.FLAVOR_DEFAULTS["iemocap"]["STRONG_NOISE_STD"]] == [0.0, 0.01, 0.05]
    view = PKG.ConfigView(flavor="iemocap", WEAK_NOISE_STD=0.02, STRONG_NOISE_STD=0.1)
    assert E.noise_response_curve(model, noisy, draws=1, cfg=view)["sigmas"] == [0.0, 0.02, 0.1]
    rep = E.robustness_report(_fresh_model(12), model, noisy, sig, draws=2)
    assert sorted(rep) == ["improvement", "initial_weights", "trained_weights"]
    a, b, imp = rep["initial_weights"], rep["trained_weights"], rep["improvement"]
    assert sorted(a) == sorted(b) == ["accuracy", "flip_rate", "sigmas"]
    assert sorted(imp) == ["accuracy_change", "flip_rate_change"]
    for key in ("accuracy", "flip_rate"):
        assert len(a[key]) == len(b[key]) == len(imp[key + "_change"]) == 4
        assert all(type(v) is float for v in a[key] + b[key] + imp[key + "_change"])
        assert imp[key + "_change"] == [y - x for x, y in zip(a[key], b[key])]
    trained = E.noise_response_curve(model, noisy, sig, draws=2)
    assert b["accuracy"] == trained["accuracy"]["mean"] and b["flip_rate"] == trained["flip_rate"]["mean"]
