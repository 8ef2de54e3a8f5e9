"""Exact integrated gradients on the MI355X (evaluate.py *attribution* / integrated_gradients / saliency_report +
csrc/attribution.hip) against the float64 closed form of tests/attribution_ref.py (bounds and their sources: its
docstring): the exact grid in both precisions and three store types, the random fixture within the random-operand
bounds with no element left out, the reference model's quadrature golden, completeness against dad_eval_split's
logits, the bit identities dad.h states, the structure of the two modes, and the host errors.  226 frames each.

Printed on the MI355X: the exact grid at 0.022 of its bound in fp32 and 0.18 with fp16 operands; the random fixture in
fp32 at 0.0013 (zero baseline) and 0.0010 (mean frame) of the random-operand bound; fp16 operands at 0.026 and 0.0044
of theirs; the golden at 0.25 and 0.28 of midpoint term plus bound; the completeness gap at most 7.4e-8."""
import ctypes
import functools
import gc
import os

import numpy as np
import pytest
import torch

import attribution_ref as R
import dadpkg
from golden.gen_attribution_golden import ATTR_OF, mean_frame
from golden.gen_input_grad_golden import inputs as golden_inputs
from oracle import data_oracle as do
from test_gpu_eval_split import DTYPES

pytestmark = pytest.mark.gpu
PKG = dadpkg.pkg()
D = PKG.data
E = PKG.evaluate
L_ = PKG._lib
GOLDEN = os.path.join(dadpkg.ROOT, "tests", "golden", "eval_attribution.npz")
EXACT_SIZES = (1, 32, 0, 64, 31, 33, 65)
ALL = ("attr", "frame_attr", "chan_attr", "utt_total")
FRAME_ONLY = ("frame_attr", "utt_total")


def _np(t):
    return t.cpu().numpy()


def _model_of(params):
    model = PKG.SSRLModel().cuda()
    flat = torch.from_numpy(np.concatenate([np.asarray(a, np.float32).reshape(-1) for a in params]))
    with torch.no_grad():
        model.student_flat.copy_(flat)
        model.teacher_flat.copy_(flat)
    return model


@functools.lru_cache(None)
def _exact():
    feats, sizes, offsets, params, dz, xb = R.exact_problem(EXACT_SIZES)
    refs = {b: R.reference(feats, sizes, offsets, params, dz, None if b == "zero" else xb) for b in ("zero", "grid")}
    return feats, sizes, offsets, params, dz, xb, refs, _model_of(params)


@functools.lru_cache(None)
def _exact_store(dt):
    feats, sizes, offsets = _exact()[:3]
    return D.FeatureStore(feats, sizes, offsets, np.arange(len(sizes)) % 4, dtype=DTYPES[dt])


@functools.lru_cache(None)
def _random():
    feats, sizes, offsets, labels = golden_inputs()
    params = do.eval_weights(23)[0]
    target = R.forward64(feats, sizes, offsets, params).argmax(1)
    dz = R.onehot_dz(target)
    xb = mean_frame(feats)
    refs = {b: R.reference(feats, sizes, offsets, params, dz, None if b == "zero" else xb) for b in ("zero", "mean")}
    return (feats, sizes, offsets, labels, params, target, dz, xb, refs, _model_of(params),
            D.FeatureStore(feats, sizes, offsets, labels))


@pytest.fixture(scope="module", autouse=True)
def _release_device_memory():
    yield
    torch.cuda.synchronize()
    for f in (_exact, _exact_store, _random):
        f.cache_clear()
    gc.collect()
    torch.cuda.synchronize()


def _run(model, store, dz, baseline=None, precision="fp32", outputs=ALL, prefill=False):
    """One dad_attribution: the outputs and 'counts' as NumPy arrays."""
    plan = E.EvalPlan.of(store)
    b = None if baseline is None else torch.from_numpy(np.asarray(baseline, np.float32)).cuda()
    pre = None
    if prefill:
        shapes = {"attr": (32 * plan.slabs, 768), "frame_attr": (32 * plan.slabs,), "chan_attr": (plan.n, 768),
                  "utt_total": (plan.n,)}
        pre = {k: torch.full(shapes[k], 0, dtype=torch.int32, device="cuda").fill_(-1).view(torch.float32)
               for k in outputs}
    out = E.enqueue_attribution(model, plan, torch.from_numpy(np.asarray(dz, np.float32)).cuda(), b,
                                precision=precision, outputs=outputs, _out=pre)
    res = {k: _np(v) for k, v in out.items()}
    res["counts"] = _np(plan._noise["attribution"]["counts_d"])
    return res


# ---- 1. the exact grid --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", ["f32", "f16", "bf16"])
@pytest.mark.parametrize("precision", ["fp32", "fp16"])
def test_exact_grid(precision, dt):
    """Lengths 1, 32, 64 and 31, 33, 65, a zero and a non-zero baseline: every output within gamma(H + 10) S (fp16:
    + 2^-11 S + the subnormal term), the crossing and lambda = 1 counts equal to the reference's, rows past each
    length 0 in pre-filled buffers."""
    feats, sizes, offsets, params, dz, xb, refs, model = _exact()
    store = _exact_store(dt)
    for bname, b in (("zero", None), ("grid", xb)):
        got = _run(model, store, dz, b, precision, prefill=True)
        ratios, fails = R.check(got, refs[bname], sizes, fp16=precision == "fp16")
        print("exact grid %s %s baseline %s: worst error / bound %s" % (precision, dt, bname, ratios))
        assert not fails, (bname, fails)
        assert not got["chan_attr"][2].any() and got["utt_total"][2] == 0     # the utterance without frames


# ---- 2. the random fixture ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("bname", ["zero", "mean"])
def test_random_fixture_fp32_within_the_derived_bound(bname):
    feats, sizes, offsets, labels, params, target, dz, xb, refs, model, store = _random()
    ref = refs[bname]
    got = _run(model, store, dz, None if bname == "zero" else xb)
    ratios, fails = R.check(got, ref, sizes, sens=True, counts=False)
    print("fp32 baseline %s: worst error / bound %s, no element left out" % (bname, ratios))
    assert not fails, fails
    assert got["counts"][0] == sizes.sum() and got["counts"][1] == 0
    # a case can only be decided otherwise where |p1| lies within the forward's error
    assert abs(int(got["counts"][2]) - int(ref["counts"][2])) <= ref["n_near"]
    assert abs(int(got["counts"][3]) - int(ref["counts"][3])) <= ref["n_near"]
    # what the closed form buys: sum_d attr = frame_attr to fp32 rounding
    v = R.valid_rows(sizes)
    lim = R.attr_bound(ref, sens=True).sum(1) + R.frame_bound(ref, sens=True) + R.gamma(R.D) * np.abs(ref["attr"]).sum(1)
    assert R.worst((got["attr"].astype(np.float64).sum(1) - got["frame_attr"])[v], lim[v]) <= 1.0


@pytest.mark.parametrize("bname", ["zero", "mean"])
def test_random_fixture_fp16_against_its_restatement(bname):
    feats, sizes, offsets, labels, params, target, dz, xb, refs, model, store = _random()
    b = None if bname == "zero" else xb
    r16 = R.reference(feats, sizes, offsets, params, dz, b, fp16_operands=True)
    got = _run(model, store, dz, b, "fp16")
    ratios, fails = R.check(got, r16, sizes, fp16=True, sens=True, counts=False)
    print("fp16 baseline %s against the fp16-operand restatement: worst error / bound %s" % (bname, ratios))
    assert not fails, fails
    assert got["counts"][0] == sizes.sum() and got["counts"][1] == 0


@pytest.mark.parametrize("bname", ["zero", "mean"])
def test_golden_quadrature_within_the_midpoint_term(bname):
    feats, sizes, offsets, labels, params, target, dz, xb, refs, model, store = _random()
    ref = refs[bname]
    g = np.load(GOLDEN)
    np.testing.assert_array_equal(g["target"][sizes > 0], target[sizes > 0])
    got = _run(model, store, dz, None if bname == "zero" else xb)
    soff = R.slab_prefix(sizes)
    lim = ref["mid"] + R.attr_bound(ref, sens=True) + R.U * np.abs(ref["attr"])
    for i in ATTR_OF:
        r = slice(32 * int(soff[i]), 32 * int(soff[i]) + int(sizes[i]))
        ratio = R.worst(got["attr"][r] - g["attr_%s_%d" % (bname, i)].astype(np.float64), lim[r])
        print("golden attr, utterance %d, baseline %s: worst error / (midpoint term + bound) %.3f" % (i, bname, ratio))
        assert ratio <= 1.0
    fa = R.to_explicit(g["frame_attr_" + bname], sizes, offsets)
    assert R.worst(got["frame_attr"] - fa, ref["mid"].sum(1) + R.frame_bound(ref, sens=True)) <= 1.0
    tot = np.array([ref["mid"][32 * int(soff[i]):32 * int(soff[i + 1])].sum() for i in range(len(sizes))])
    assert R.worst(got["utt_total"] - g["utt_total_" + bname], tot + R.total_bound(ref, sizes, sens=True)) <= 1.0


@pytest.mark.parametrize("bname", ["zero", "mean"])
def test_completeness_against_eval_split_logits(bname):
    feats, sizes, offsets, labels, params, target, dz, xb, refs, model, store = _random()
    ref = refs[bname]
    b = None if bname == "zero" else torch.from_numpy(xb).cuda()
    res = E.integrated_gradients(model, store, target="pred", baseline=b, outputs=FRAME_ONLY)
    np.testing.assert_array_equal(_np(res["target"])[sizes > 0], target[sizes > 0])
    z = _np(E.enqueue_eval_split(model, E.EvalPlan.of(store), outputs=("logits",))["logits"]).astype(np.float64)
    dzg = _np(res["dz"]).astype(np.float64)
    gap = _np(res["utt_total"]).astype(np.float64) - (dzg * (z - ref["z0"])).sum(1)
    lim = R.completeness_bound(ref, feats, sizes, offsets, params, dzg)
    has = sizes > 0
    print("completeness baseline %s: worst |gap| / bound %.3f, largest |gap| %.3g"
          % (bname, R.worst(gap[has], lim[has]), np.abs(gap[has]).max()))
    assert R.worst(gap[has], lim[has]) <= 1.0
    # integrated_gradients' own gap is the same quantity (its z(x') is formed in float64 on the device)
    own = _np(res["completeness_gap"])
    assert own[~has].tolist() == [0.0]
    assert R.worst(own[has], lim[has]) <= 1.0
    assert res["frames"] == sizes.sum() and res["n_nonfinite"] == 0
    assert res["n_crossing"] > 0.3 * sizes.sum() * R.H          # the fixture switches nearly half of its units


# ---- 3. the bit identities ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["fp32", "fp16"])
def test_bit_identities(precision):
    feats, sizes, offsets, labels, params, target, dz, xb, refs, model, store = _random()
    a = _run(model, store, dz, xb, precision, prefill=True)
    b = _run(model, store, dz, xb, precision)
    for k in ALL + ("counts",):                                            # two calls write the same bits
        assert a[k].tobytes() == b[k].tobytes(), k
    none = _run(model, store, dz, None, precision)                         # baseline == NULL equals zeros
    zero = _run(model, store, dz, np.zeros(768, np.float32), precision)
    for k in ALL + ("counts",):
        assert none[k].tobytes() == zero[k].tobytes(), k
    fo = _run(model, store, dz, xb, precision, FRAME_ONLY, prefill=True)   # frame-only mode: the same bits
    for k in FRAME_ONLY:
        assert fo[k].tobytes() == a[k].tobytes(), k
    np.testing.assert_array_equal(fo["counts"][[0, 2, 3]], a["counts"][[0, 2, 3]])
    # pre-filled buffers read 0 past every length; the utterance without frames
    v = R.valid_rows(sizes)
    assert not a["attr"][~v].any() and not a["frame_attr"][~v].any() and not fo["frame_attr"][~v].any()
    assert np.isfinite(a["attr"]).all() and np.isfinite(a["chan_attr"]).all()
    assert not a["chan_attr"][0].any() and a["utt_total"][0] == 0 and fo["utt_total"][0] == 0
    # the same utterances in another order: another slab-to-workgroup assignment
    order = np.array([6, 5, 4, 3, 2, 1, 0])
    p = _run(model, store.subset(order), dz[order], xb, precision)
    so, sp = R.slab_prefix(sizes), R.slab_prefix(sizes[order])
    for k, i in enumerate(order):
        for name in ("attr", "frame_attr"):
            assert p[name][32 * sp[k]:32 * sp[k + 1]].tobytes() == a[name][32 * so[i]:32 * so[i + 1]].tobytes(), (name, i)
        for name in ("chan_attr", "utt_total"):
            assert p[name][k].tobytes() == a[name][i].tobytes(), (name, i)
    np.testing.assert_array_equal(p["counts"], a["counts"])


def test_captured_call_replays_the_eager_result():
    feats, sizes, offsets, labels, params, target, dz, xb, refs, model, store = _random()
    plan = E.EvalPlan.of(store)
    d, b = torch.from_numpy(dz).cuda(), torch.from_numpy(xb).cuda()
    eager = E.enqueue_attribution(model, plan, d, b, outputs=ALL)
    counts = plan._noise["attribution"]["counts_d"]
    want = counts.clone()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = E.enqueue_attribution(model, plan, d, b, outputs=ALL)
    counts.fill_(-1)                                     # the call itself zeroes its counts
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(counts, want)
    for k in ALL:
        assert torch.equal(out[k].view(torch.int32), eager[k].view(torch.int32)), k


# ---- 4. structure -------------------------------------------------------------------------------------------------
def test_frame_only_mode_is_another_kernel_and_a_smaller_workspace():
    feats, sizes, offsets, labels, params, target, dz, xb, refs, model, store = _random()
    plan = E.EvalPlan.of(store)
    d = torch.from_numpy(dz).cuda()
    for precision in ("fp32", "fp16"):
        fo = E.attribution_plan(model, plan, d, precision=precision, outputs=FRAME_ONLY)
        at = E.attribution_plan(model, plan, d, precision=precision, outputs=("attr",))
        full = E.attribution_plan(model, plan, d, precision=precision, outputs=ALL)
        assert fo["mode"] == "frame_only" and at["mode"] == full["mode"] == "full"
        assert fo["kernel"] != full["kernel"] and at["kernel"] == full["kernel"]
        assert fo["kernel"] % 2 == 0 and full["kernel"] % 2 == 1
        assert fo["workspace_bytes"] < at["workspace_bytes"] or precision == "fp32"
        assert at["workspace_bytes"] < full["workspace_bytes"]            # the slab partials of chan_attr
        assert full["workspace_bytes"] - at["workspace_bytes"] >= 4 * 768 * plan.slabs
        total = int(L_.lib().dad_attribution_workspace_bytes(plan.n, plan.slabs, E._PRECISIONS[precision]))
        assert full["workspace_bytes"] == total
        assert E.attribution_plan(model, plan, d, precision=precision, outputs=("frame_attr",))["launches"] \
            == fo["launches"] - 1                                          # no finish launch without utt_total
    # a frame-only call runs in a workspace of its own size
    plan._noise.pop("attribution", None)
    E.enqueue_attribution(model, plan, d, outputs=FRAME_ONLY)
    assert plan._noise["attribution"]["ws"].numel() == E.attribution_plan(model, plan, d, outputs=FRAME_ONLY)["workspace_bytes"]


def test_integrated_gradients_margin_and_saliency_report():
    feats, sizes, offsets, labels, params, target, dz, xb, refs, model, store = _random()
    plan = E.EvalPlan.of(store)
    res = E.integrated_gradients(model, store, target="margin", baseline="mean")
    z = _np(E.enqueue_eval_split(model, plan, outputs=("logits",))["logits"])
    has = sizes > 0
    np.testing.assert_array_equal(_np(res["dz"])[has], R.margin_dz(z, z.argmax(1))[has])
    np.testing.assert_array_equal(_np(res["baseline"]), xb)                # the device's mean frame
    direct = E.enqueue_attribution(model, plan, res["dz"], res["baseline"], outputs=ALL[1:])
    for k in ALL[1:]:
        assert torch.equal(direct[k].view(torch.int32), res[k].view(torch.int32)), k
    for t in ("label", 2):
        r = E.integrated_gradients(model, store, target=t, outputs=())
        want = labels if t == "label" else np.full(len(sizes), 2)
        np.testing.assert_array_equal(_np(r["target"]), want)
        assert set(ALL) & set(r) == {"utt_total"}
    # the report: two 7-utterance splits of equal lengths, two models
    noisy = D.FeatureStore((feats + np.float32(0.25) * np.random.RandomState(5).standard_normal(feats.shape)
                            .astype(np.float32)), sizes, offsets, labels)
    other = _model_of(do.eval_weights(29)[0])
    rep = E.saliency_report(other, model, store, noisy, target="pred", baseline=None)
    assert set(rep) == {"initial_weights", "trained_weights", "change"}
    ig = E.integrated_gradients(model, store, target="pred", baseline=None)
    prof = torch.zeros(4, 768, dtype=torch.float64, device="cuda")
    prof.index_add_(0, ig["target"], ig["chan_attr"].to(torch.float64))
    cnt = torch.bincount(ig["target"], minlength=4).clamp(min=1)
    got = np.asarray(rep["trained_weights"]["clean"]["class_profile"])
    np.testing.assert_allclose(got, _np(prof / cnt[:, None]), rtol=1e-12, atol=1e-15)
    tw = rep["trained_weights"]
    assert 0 < tw["clean"]["temporal_concentration"] <= 1.0
    ca, cb = (_np(E.integrated_gradients(model, s, target="pred")["chan_attr"]).astype(np.float64)[has]
              for s in (store, noisy))
    cos = ((ca * cb).sum(1) / (np.linalg.norm(ca, axis=1) * np.linalg.norm(cb, axis=1))).mean()
    np.testing.assert_allclose(tw["clean_noisy_cosine"], cos, rtol=1e-12)
    assert tw["clean"]["max_completeness_gap"] < 1e-3
    assert "clean_noisy_cosine_change" in rep["change"] and len(rep["change"]["clean"]["class_profile_cosine"]) == 4
    short = D.FeatureStore(feats[:64], np.array([31, 33]), np.array([0, 31]), np.array([0, 1]))
    assert E.saliency_report(model, model, store, short)["trained_weights"]["clean_noisy_cosine"] is None


# ---- 5. host errors -----------------------------------------------------------------------------------------------
def test_host_errors():
    feats, sizes, offsets, labels, params, target, dz, xb, refs, model, store = _random()
    plan = E.EvalPlan.of(store)
    d = torch.from_numpy(dz).cuda()
    fn, ws_bytes = L_.lib().dad_attribution, L_.lib().dad_attribution_workspace_bytes
    ws = torch.empty(int(ws_bytes(plan.n, plan.slabs, 0)), dtype=torch.uint8, device="cuda")
    out = {"utt_total": torch.empty(plan.n, device="cuda")}
    counts = torch.zeros(L_.AT_COUNTS, dtype=torch.int64, device="cuda")
    good = lambda: E._at_args(model, plan, d, None, False, 0, out, counts)
    assert fn(good(), L_.ptr(ws), None) == 0
    for field in ("store", "rows", "lens", "slab_off", "params", "dz", "counts"):      # NULL required pointers
        a = good()
        setattr(a, field, None)
        assert fn(a, L_.ptr(ws), None) == 1001, field
    assert fn(good(), None, None) == 1001 and fn(None, L_.ptr(ws), None) == 1001
    a = good()
    a.n = 0
    assert fn(a, L_.ptr(ws), None) == 1002
    a = good()
    a.store_dtype = 7
    assert fn(a, L_.ptr(ws), None) == 1001
    assert ws_bytes(0, 1, 0) == 0
    slots = (ctypes.c_int64 * L_.AT_PLAN_SLOTS)()
    assert L_.lib().dad_attribution_plan(good(), None) == 1001
    assert L_.lib().dad_attribution_plan(good(), slots) == 0 and slots[L_.AT_PLAN_MODE] == 0
    with pytest.raises(L_.DadError, match="1004"):                                      # bf16 operands
        E.enqueue_attribution(model, plan, d, precision="bf16")
    with pytest.raises(L_.DadError):
        E.integrated_gradients(model, store, precision="bf16")
    with pytest.raises(ValueError, match="baseline"):                                   # shape, then device
        E.enqueue_attribution(model, plan, d, torch.zeros(767, device="cuda"))
    with pytest.raises(ValueError, match="baseline on"):
        E.enqueue_attribution(model, plan, d, torch.zeros(768))
    with pytest.raises(ValueError, match="dz must be"):
        E.enqueue_attribution(model, plan, d[:3])
    with pytest.raises(ValueError, match="dz must be"):
        E.enqueue_attribution(model, plan, d.cpu())
    with pytest.raises(RuntimeError, match="model on"):
        E.enqueue_attribution(PKG.SSRLModel(), plan, d)
    with pytest.raises(ValueError, match="no labels"):
        E.integrated_gradients(model, D.FeatureStore(feats, sizes, offsets), target="label")
    # a non-finite dz: its elements are written 0, counted and reported
    bad = d.clone()
    bad[3, 0] = float("nan")
    got = E.enqueue_attribution(model, plan, bad, outputs=("attr", "chan_attr"))
    rows = slice(32 * int(R.slab_prefix(sizes)[3]), 32 * int(R.slab_prefix(sizes)[4]))
    assert not got["attr"][rows].any() and got["attr"][:rows.start].any() and not got["chan_attr"][3].any()
    assert int(plan._noise["attribution"]["counts_d"][L_.AT_NONFINITE]) == 32 * 768
    with pytest.raises(L_.DadError, match="not finite"):
        E._read_at_counts(plan)
