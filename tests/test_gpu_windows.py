"""Sliding-window and prefix inference over a split on the MI355X (evaluate.py *_windows* + csrc/eval_windows.hip):
per-window outputs against the float64 reference of tests/windows_ref.py (computed once per case on the CPU), the
per-utterance summaries and the DAD_EW_* block against NumPy on the kernel's own predictions, a derived bound on
exactly representable operands, the reference model's golden numbers, the bit-level properties of the design, the
FP16 operand mode, the error paths, and the duration curves."""
import functools
import os

import numpy as np
import pytest
import torch

import dadpkg
import exact_problem as X
import windows_ref as wr
from golden.gen_windows_golden import MODES as GOLDEN_MODES, inputs as golden_inputs
from oracle import data_oracle as do
from test_gpu_eval_split import _model, _store

pytestmark = pytest.mark.gpu
PKG = dadpkg.pkg()
D = PKG.data
E = PKG.evaluate
L_ = PKG._lib

W_OUT = ("w_emb", "w_logits", "w_probs", "w_score", "w_pred")
U_OUT = ("mean_probs", "mean_pred", "vote_pred", "last_pred", "settle", "switches")
ALL = W_OUT + U_OUT
IDS = ["%s-h%d-m%d" % (mode, h, m) for h, m, mode in wr.MODE_CASES]


def _np(t):
    return t.cpu().numpy()


def _check_values(res, ref, use_entropy=True):
    np.testing.assert_array_equal(res["win_off"], ref["win_off"])
    np.testing.assert_allclose(_np(res["w_emb"]), ref["emb"], rtol=1e-5, atol=1e-4)
    np.testing.assert_allclose(_np(res["w_logits"]), ref["logits"], rtol=1e-5, atol=1e-4)
    np.testing.assert_allclose(_np(res["w_probs"]), ref["probs"], rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(_np(res["w_score"]), ref["score_entropy" if use_entropy else "score_max"],
                               rtol=1e-5, atol=1e-6)
    off = ref["win_off"]
    mean = np.array([ref["probs"][a:b].mean(0) if b > a else np.zeros(4) for a, b in zip(off[:-1], off[1:])])
    np.testing.assert_allclose(_np(res["mean_probs"]), mean, rtol=1e-5, atol=1e-6)


def _check_preds(res, ref, min_gap=wr.GAP):
    pred = _np(res["w_pred"])
    np.testing.assert_array_equal(pred, _np(res["w_logits"]).argmax(1))       # first maximum
    ok = wr.decided(ref, min_gap)
    np.testing.assert_array_equal(pred[ok], ref["pred"][ok])


def _check_summaries(res, sizes, labels, hop, span, mode):
    """Per-utterance outputs and the block against the NumPy restatement from the kernel's own w_pred / w_probs."""
    w_pred, w_probs = _np(res["w_pred"]), _np(res["w_probs"])
    s = wr.summaries(w_pred, w_probs, res["win_off"], sizes, hop, span, mode)
    np.testing.assert_allclose(_np(res["mean_probs"]), s["mean_probs"], rtol=0, atol=1e-6)
    for k in ("vote_pred", "last_pred", "settle", "switches"):
        np.testing.assert_array_equal(_np(res[k]).astype(np.int64), s[k], err_msg=k)
    got_mean = _np(res["mean_pred"])
    live = s["J"] > 0
    np.testing.assert_array_equal(got_mean[~live], -1)
    np.testing.assert_array_equal(got_mean[live], _np(res["mean_probs"])[live].argmax(1))
    s["mean_pred"] = got_mean                  # (the argmax of the device's own fp32 mean)
    np.testing.assert_array_equal(res["block"], wr.block(L_, w_pred, s, res["win_off"], labels))
    return s


@pytest.mark.parametrize("net", ["s", "t"])
@pytest.mark.parametrize("hop,span,mode", wr.MODE_CASES, ids=IDS)
def test_fp32_matches_float64(hop, span, mode, net):
    store = _store("main", "f32")
    ref = wr.main_reference("f32", net, hop, span, mode)
    res = E.evaluate_windows_store(_model(), store, hop, span, mode, use_teacher=net == "t", outputs=ALL)
    _check_values(res, ref)
    _check_preds(res, ref)
    s = _check_summaries(res, store.sizes, store.labels, hop, span, mode)
    assert res["n"] == 39 and res["n_empty"] == (store.sizes == 0).sum() == 1 and res["n_nonfinite"] == 0
    assert res["n_labelled"] == (store.labels >= 0).sum() == 37
    assert res["n_windows"] == ref["win_off"][-1] == len(ref["pred"])
    i0 = int(np.where(store.sizes == 0)[0][0])                    # the J = 0 utterance
    assert s["J"][i0] == 0 and not _np(res["mean_probs"])[i0].any()
    top = int(s["J"].max())
    if top < L_.EW_CURVE:                                         # the curve beyond the longest J
        assert not res["reached"][top:].any() and not res["correct"][top:].any()
        assert (res["carried"][top:] == res["carried"][top - 1]).all()


@pytest.mark.parametrize("use_entropy", [True, False])
@pytest.mark.parametrize("dt", ["f16", "bf16"])
@pytest.mark.parametrize("hop,span,mode", [(7, 3, "sliding"), (32, 2, "sliding"), (33, 1, "prefix")])
def test_16bit_stores_match_float64_on_the_widened_values(hop, span, mode, dt, use_entropy):
    store = _store("main", dt)
    ref = wr.main_reference(dt, "s", hop, span, mode)
    res = E.evaluate_windows_store(_model(), store, hop, span, mode, use_entropy=use_entropy, outputs=ALL)
    _check_values(res, ref, use_entropy)
    _check_preds(res, ref)
    _check_summaries(res, store.sizes, store.labels, hop, span, mode)


@pytest.mark.parametrize("dt", ["f32", "f16", "bf16"])
@pytest.mark.parametrize("hop,span,mode", [(1, 1, "sliding"), (8, 4, "sliding"), (25, 2, "sliding"), (32, 1, "prefix")])
def test_fp16_operands_match_their_float64_simulation(hop, span, mode, dt):
    """FP16 operand mode against float64 on fp16-rounded rows and W1: only the accumulation differs, so the fp32
    tolerances hold; predictions on windows whose gap exceeds twice the logit tolerance."""
    store = _store("main", dt)
    for net in "st":
        ref = wr.main_reference(dt, net, hop, span, mode, True)
        res = E.evaluate_windows_store(_model(), store, hop, span, mode, use_teacher=net == "t", precision="fp16",
                                       outputs=ALL)
        _check_values(res, ref)
        _check_preds(res, ref, 2 * (1e-4 + 1e-5 * float(np.abs(ref["logits"]).max())))
        _check_summaries(res, store.sizes, store.labels, hop, span, mode)


@functools.lru_cache(None)
def _exact():
    """Features and weights on tests/exact_problem.py's dyadic grid: lengths 1, 33, 65."""
    sizes = np.array([1, 33, 65])
    offsets = np.concatenate([[0], np.cumsum(sizes)[:-1]])
    feats = X.q(np.clip(4.0 * np.random.RandomState(5).standard_normal((int(sizes.sum()), 768)), -16, 16), 2.0 ** -3)
    st = X.state()
    model = PKG.SSRLModel().cuda()
    flat = lambda ps: torch.from_numpy(np.concatenate([np.asarray(a, np.float32).reshape(-1) for a in ps]))
    with torch.no_grad():
        model.student_flat.copy_(flat(st["student"]))
        model.teacher_flat.copy_(flat(st["teacher"]))
    hid = {k: wr.hidden64(feats, st[n][0], st[n][1]) for k, n in (("s", "student"), ("t", "teacher"))}
    return feats, sizes, offsets, st, model, hid


@pytest.mark.parametrize("precision", ["fp32", "fp16"])
@pytest.mark.parametrize("hop,span,mode", [(7, 3, "sliding"), (32, 1, "sliding"), (32, 1, "prefix")])
def test_derived_bound_on_exact_operands(hop, span, mode, precision):
    """On the dyadic grid the pre-activations are exact in both operand modes, so a window of c frames obeys
    |e - e_ref| <= (c + 2) u |e_ref| and the logits (c + H + 8) u times their magnitude sum: no measured number."""
    feats, sizes, offsets, st, model, hid = _exact()
    store = D.FeatureStore(feats, sizes, offsets, np.array([0, 1, 2]))
    for net, name in (("s", "student"), ("t", "teacher")):
        ref = wr.forward64(hid[net], sizes, offsets, np.arange(3), st[name][2], st[name][3], hop, span, mode)
        res = E.evaluate_windows_store(model, store, hop, span, mode, use_teacher=net == "t", precision=precision,
                                       outputs=("w_emb", "w_logits"))
        c = ref["frames"].astype(np.float64)[:, None]
        assert (ref["emb"] >= 0).all() and ref["emb"].max() > 0
        e_ratio = X.worst(_np(res["w_emb"]).astype(np.float64) - ref["emb"], X.bound("e", None, c) * np.abs(ref["emb"]))
        z_ratio = X.worst(_np(res["w_logits"]).astype(np.float64) - ref["logits"],
                          X.bound("z", None, c) * ref["logit_mag"])
        print("%s %s (%d, %d) %s: worst error / bound: embeddings %.3f, logits %.3f"
              % (precision, mode, hop, span, name, e_ratio, z_ratio))
        assert e_ratio <= 1.0 and z_ratio <= 1.0


def test_golden_windows_of_the_reference_model():
    """SSRLModel.predict on cropped features (tests/golden/eval_windows.npz) at the eval goldens' 1e-4, through
    the list-of-tensors convenience."""
    g = np.load(os.path.join(dadpkg.ROOT, "tests", "golden", "eval_windows.npz"))
    feats, sizes, offsets = golden_inputs()
    model = _model(int(g["seed"]))
    mats = [torch.from_numpy(feats[o:o + s]) for o, s in zip(offsets, sizes)]
    for mode, (hop, span) in GOLDEN_MODES.items():
        res = E.windows(model, mats, hop, span, mode, outputs=("w_logits", "w_pred"))
        np.testing.assert_allclose(_np(res["w_logits"]), g[mode + "_logits"], rtol=1e-5, atol=1e-4)
        top = np.sort(g[mode + "_logits"].astype(np.float64), 1)
        ok = top[:, -1] - top[:, -2] > wr.GAP
        assert ok.mean() >= 0.95
        np.testing.assert_array_equal(_np(res["w_pred"])[ok], g[mode + "_pred"][ok])
        assert res["n_labelled"] == 0 and res["n"] == len(sizes) and not res["reached"].any()


def _bits(t):
    return t.contiguous().reshape(-1).view(torch.uint8)


def test_two_calls_write_identical_bits():
    model, store = _model(), _store("main", "f32")
    for precision in ("fp32", "fp16"):
        for hop, span, mode in ((5, 2, "sliding"), (25, 1, "prefix")):
            a = E.evaluate_windows_store(model, store, hop, span, mode, precision=precision, outputs=ALL)
            E.evaluate_windows_store(model, store, 7, 3, "sliding", precision=precision)      # another plan between
            b = E.evaluate_windows_store(model, store, hop, span, mode, precision=precision, outputs=ALL)
            assert a["block"].tobytes() == b["block"].tobytes()
            for k in ALL:
                assert a[k].data_ptr() != b[k].data_ptr()
                assert torch.equal(_bits(a[k]), _bits(b[k])), (precision, mode, k)


@pytest.mark.parametrize("hop,span,mode", [(5, 2, "sliding"), (8, 1, "prefix")])
def test_outputs_do_not_depend_on_the_subset_order(hop, span, mode):
    """Per-utterance outputs (and an utterance's windows) are the same bits wherever the utterance stands in the
    subset; the two samples that the subset repeats give equal rows."""
    feats, sizes, offsets, labels, order = wr.main_inputs()
    model, a_store = _model(), _store("main", "f32")
    perm = np.random.RandomState(3).permutation(len(order))
    b_store = D.FeatureStore(feats, sizes, offsets, labels).subset(order[perm])
    a = E.evaluate_windows_store(model, a_store, hop, span, mode, outputs=ALL)
    b = E.evaluate_windows_store(model, b_store, hop, span, mode, outputs=ALL)
    for ib, ia in enumerate(perm):
        for k in U_OUT:
            assert torch.equal(_bits(a[k][ia]), _bits(b[k][ib])), k
        wa, wb = a["win_off"][ia:ia + 2], b["win_off"][ib:ib + 2]
        for k in W_OUT:
            assert torch.equal(_bits(a[k][wa[0]:wa[1]]), _bits(b[k][wb[0]:wb[1]])), k
    for first, again in ((3, 30), (11, 31)):                      # the subset's repeats
        assert order[first] == order[again]
        for k in U_OUT:
            assert torch.equal(_bits(a[k][first]), _bits(a[k][again])), k


@pytest.mark.parametrize("precision", ["fp32", "fp16"])
@pytest.mark.parametrize("hop", [32, 128])
def test_last_prefix_is_the_split_evaluator_bit_for_bit(hop, precision):
    """hop % 32 == 0: a piece is a slab, so the last prefix repeats dad_eval_split's arithmetic exactly."""
    model, store = _model(), _store("main", "f32")
    whole = E.evaluate_store(model, store, use_teacher=True, precision=precision,
                             outputs=("emb", "logits", "pred", "t_emb", "t_logits", "t_pred"))
    for teacher, pre in ((False, ""), (True, "t_")):
        res = E.evaluate_windows_store(model, store, hop, 1, "prefix", use_teacher=teacher, precision=precision,
                                       outputs=("w_emb", "w_logits", "w_pred", "last_pred"))
        off = res["win_off"]
        live = np.nonzero(np.diff(off) > 0)[0]
        last = torch.from_numpy(off[1:][live].astype(np.int64) - 1).cuda()
        idx = torch.from_numpy(live).cuda()
        assert len(live) == (store.sizes > 0).sum() == 38
        for mine, theirs in (("w_emb", "emb"), ("w_logits", "logits"), ("w_pred", "pred")):
            assert torch.equal(_bits(res[mine][last]), _bits(whole[pre + theirs][idx])), (pre, mine)
        assert torch.equal(res["last_pred"][idx], whole[pre + "pred"][idx])


@pytest.mark.parametrize("hop", [1, 7, 32, 33])
def test_sliding_and_prefix_agree_on_window_zero(hop):
    model, store = _model(), _store("main", "f32")
    s = E.evaluate_windows_store(model, store, hop, 1, "sliding", outputs=W_OUT)
    p = E.evaluate_windows_store(model, store, hop, 1, "prefix", outputs=W_OUT)
    np.testing.assert_array_equal(s["win_off"], p["win_off"])     # span 1: the same windows
    first = torch.from_numpy(s["win_off"][:-1][np.diff(s["win_off"]) > 0].astype(np.int64)).cuda()
    for k in W_OUT:
        assert torch.equal(_bits(s[k][first]), _bits(p[k][first])), k


@pytest.mark.parametrize("hop", [1, 5, 25, 33])
def test_span_one_windows_add_up_to_the_utterance(hop):
    """With span 1 the windows partition the utterance: sum_j c_j w_emb[j] = L emb to (L + 2) 2^-24 relative."""
    model, store = _model(), _store("main", "f32")
    emb = _np(E.evaluate_store(model, store, outputs=("emb",))["emb"]).astype(np.float64)
    res = E.evaluate_windows_store(model, store, hop, 1, "sliding", outputs=("w_emb",))
    w_emb = _np(res["w_emb"]).astype(np.float64)
    utt, st, en = E.window_frames(store.sizes, hop, 1, "sliding")
    total = np.zeros_like(emb)
    np.add.at(total, utt, (en - st)[:, None] * w_emb)
    Ls = store.sizes.astype(np.float64)[:, None]
    assert X.worst(total - Ls * emb, (Ls + 2) * X.U32 * np.abs(Ls * emb)) <= 1.0


def _raw_args(model, plan, b, hop, span, mode):
    a = L_.DadWindowArgs()
    a.store = plan.store.feats.data_ptr()
    a.rows, a.lens, a.slab_off = plan.rows_d.data_ptr(), plan.lens_d.data_ptr(), plan.slab_off_d.data_ptr()
    a.labels = plan.labels_d.data_ptr()
    a.params = model.student_flat.data_ptr()
    a.win_off, a.piece_off = b["win_off_d"].data_ptr(), b["piece_off_d"].data_ptr()
    a.win_off_host = b["win_off"].ctypes.data
    a.result = b["result_d"].data_ptr()
    a.n, a.slabs, a.windows, a.pieces = plan.n, plan.slabs, b["windows"], b["pieces"]
    a.hop, a.span, a.mode = hop, span, {"sliding": L_.WIN_SLIDING, "prefix": L_.WIN_PREFIX}[mode]
    a.store_dtype, a.use_entropy, a.precision = L_.STORE_F32, 1, L_.PREC_FP32
    return a


def test_error_paths_launch_nothing():
    model, store = _model(), _store("main", "f32")
    plan = E.EvalPlan.of(store)
    E.evaluate_windows_store(model, store, 8, 2, "sliding")       # (builds the buffers and the workspace)
    b = plan.window_buffers(8, 2, "sliding")
    fn = L_.lib().dad_eval_windows
    stream = torch.cuda.current_stream().cuda_stream
    b["result_d"].fill_(-7)

    def call(**change):
        a = _raw_args(model, plan, b, 8, 2, "sliding")
        for k, v in change.items():
            setattr(a, k, v)
        return fn(a, L_.ptr(b["ws"]), stream)

    for name in ("store", "rows", "lens", "slab_off", "params", "win_off", "piece_off", "win_off_host", "result"):
        assert call(**{name: None}) == L_.E_ARG, name
    assert fn(_raw_args(model, plan, b, 8, 2, "sliding"), None, stream) == L_.E_ARG
    assert call(hop=0) == L_.E_ARG
    assert call(span=0) == L_.E_ARG
    assert call(mode=2) == L_.E_ARG
    assert call(mode=L_.WIN_PREFIX) == L_.E_ARG                   # prefix with span 2
    assert call(store_dtype=3) == L_.E_ARG
    assert call(precision=L_.PREC_BF16) == L_.E_UNSUPPORTED
    assert call(windows=b["windows"] + 1) == L_.E_ARG            # disagrees with win_off
    assert call(windows=b["windows"] - 1) == L_.E_ARG
    assert call(n=0) == L_.E_SHAPE
    assert call(pieces=plan.slabs - 1) == L_.E_SHAPE
    assert call(pieces=2 ** 31) == L_.E_SHAPE
    torch.cuda.synchronize()
    assert (b["result_d"] == -7).all()                            # nothing ran
    with pytest.raises(L_.DadError, match="DAD_E_UNSUPPORTED"):
        E.evaluate_windows_store(model, store, 8, 2, "sliding", precision="bf16")
    with pytest.raises(ValueError):
        E.evaluate_windows_store(model, store, 8, 2, "prefix")
    with pytest.raises(ValueError, match="unknown output"):
        E.evaluate_windows_store(model, store, 8, 2, "sliding", outputs=("emb",))
    assert call() == 0                                            # and the unchanged arguments run
    torch.cuda.synchronize()
    assert int(b["result_d"][L_.EW_N]) == 39


def test_nonfinite_features_are_reported():
    rs = np.random.RandomState(3)
    sizes = np.array([5, 40, 2, 33, 7])
    offsets = np.concatenate([[0], np.cumsum(sizes)[:-1]])
    feats = rs.standard_normal((int(sizes.sum()), 768)).astype(np.float32)
    labels = np.array([0, 1, 2, 3, 0])
    assert E.evaluate_windows_store(_model(), D.FeatureStore(feats, sizes, offsets, labels), 8, 2)["n_nonfinite"] == 0
    feats[offsets[3] + 32, 100] = np.inf        # frame 32 of utterance 3: the last of its 4 windows, frames [24, 33)
    with pytest.raises(L_.DadError, match="1 of 11 window"):
        E.evaluate_windows_store(_model(), D.FeatureStore(feats, sizes, offsets, labels), 8, 2)


def test_captured_call_replays_the_eager_result():
    model, store = _model(), _store("main", "f32")
    plan = E.EvalPlan.of(store)
    eager = E.evaluate_windows_store(model, store, 25, 2, "sliding", outputs=("w_logits", "settle"))
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = E.enqueue_eval_windows(model, plan, 25, 2, "sliding", outputs=("w_logits", "settle"))
    b = plan.window_buffers(25, 2, "sliding")
    b["result_d"].zero_()
    g.replay()
    torch.cuda.synchronize()
    assert b["result_d"].cpu().numpy().tobytes() == eager["block"].tobytes()
    for k in ("w_logits", "settle"):
        assert torch.equal(_bits(out[k]), _bits(eager[k])), k


def test_duration_curves_of_two_small_stores():
    feats, sizes, offsets, labels, order = wr.main_inputs()
    model, noisy = _model(), _store("main", "f32")
    clean = D.FeatureStore(feats, sizes, offsets, labels)          # 37 utterances, store order
    hop = 8
    for store in (clean, noisy):
        c = E.early_decision_curve(model, store, hop)
        k = -(-int(store.sizes.max()) // hop)                      # prefixes of the longest utterance
        assert k <= L_.EW_CURVE
        for key in ("frames", "reached", "accuracy", "accuracy_carried"):
            assert c[key].shape == (k,), key
        np.testing.assert_array_equal(c["frames"], (np.arange(k) + 1) * hop)
        lab = (store.labels >= 0) & (store.labels < 4) & (store.sizes > 0)
        assert c["reached"][0] == lab.sum()
        assert (np.diff(c["reached"]) <= 0).all()
        assert c["accuracy_carried"][-1] == pytest.approx(c["final"]["accuracy"], abs=1e-12)
        whole = E.evaluate_store(model, store)["confusion_student"]
        i0 = np.nonzero(store.sizes == 0)[0]                        # the split evaluator also counts the empty one
        for i in i0[(store.labels[i0] >= 0)]:
            whole[store.labels[i], int(np.argmax(do.eval_weights(11)[0][3]))] -= 1
        np.testing.assert_array_equal(c["final"]["confusion_matrix"], whole)
        assert c["mean_switches"] >= 0 and 0 < c["mean_settle_frames"] <= store.sizes.max()
    rep = E.duration_report(model, clean, noisy, hop)
    assert sorted(rep) == ["clean", "frames_to_final", "noisy"]
    for name in ("clean", "noisy"):
        c, f = rep[name], rep["frames_to_final"][name]
        assert f is not None and f % hop == 0
        j = f // hop - 1
        assert c["accuracy_carried"][j] >= c["final"]["accuracy"] - 1e-12
        assert (c["accuracy_carried"][:j] < c["final"]["accuracy"]).all()
