"""Input gradients, FGSM and PGD on the MI355X (evaluate.py *input_grad* / *adversarial* + csrc/input_grad.hip)
against the float64 closed form of tests/input_grad_ref.py (bounds and their sources: its docstring): bit equality on
exactly representable operands, the derived bound and the sign caps on the random fixture, the design's identities,
FGSM end to end against the reference model's golden numbers, PGD step by step, the error paths.

Printed on the MI355X: the random fixture in fp32 at 0.016 of its bound with 0.82 % of the elements unchecked and no
sign of 173,568 different; fp16 operands 0.078 % of the signs; the FGSM direction equal to the golden signs on 6 of 6
utterances."""
import functools
import gc
import os

import numpy as np
import pytest
import torch

import dadpkg
import input_grad_ref as R
from golden.gen_input_grad_golden import EPS as GOLDEN_EPS, inputs as golden_inputs
from oracle import data_oracle as do
from test_gpu_eval_split import DTYPES

pytestmark = pytest.mark.gpu
PKG = dadpkg.pkg()
D = PKG.data
E = PKG.evaluate
L_ = PKG._lib
GOLDEN = os.path.join(dadpkg.ROOT, "tests", "golden", "eval_input_grad.npz")
EXACT_SIZES = (1, 32, 0, 64, 31, 33, 65)
ALL = ("grad", "delta", "frame_l1")


def _np(t):
    return t.cpu().numpy()


def _bits(t):
    return t.contiguous().reshape(-1).view(torch.uint8)


def _model_of(params):
    model = PKG.SSRLModel().cuda()
    flat = torch.from_numpy(np.concatenate([np.asarray(a, np.float32).reshape(-1) for a in params]))
    with torch.no_grad():
        model.student_flat.copy_(flat)
        model.teacher_flat.copy_(flat)
    return model


@functools.lru_cache(None)
def _exact():
    feats, sizes, offsets, params, dz, delta = R.exact_problem(EXACT_SIZES)
    return feats, sizes, offsets, params, dz, delta, _model_of(params)


@functools.lru_cache(None)
def _exact_store(dt):
    feats, sizes, offsets = _exact()[:3]
    return D.FeatureStore(feats, sizes, offsets, np.arange(len(sizes)) % 4, dtype=DTYPES[dt])


@functools.lru_cache(None)
def _random():
    feats, sizes, offsets, labels = golden_inputs()
    params = do.eval_weights(23)[0]
    dz = R.ce_dz(R.forward64(feats, sizes, offsets, params), labels).astype(np.float32)
    return (feats, sizes, offsets, labels, params, dz, R.reference(feats, sizes, offsets, params, dz),
            _model_of(params), D.FeatureStore(feats, sizes, offsets, labels))


@pytest.fixture(scope="module", autouse=True)
def _release_device_memory():
    yield
    torch.cuda.synchronize()
    for f in (_exact, _exact_store, _random):
        f.cache_clear()
    gc.collect()
    torch.cuda.synchronize()


def _run(model, store, dz, delta=None, alpha=0.0, radius=float("inf"), precision="fp32", alias=False, outputs=ALL):
    """One dad_input_grad: NumPy 'grad', 'step', 'frame_l1', 'counts'."""
    plan = E.EvalPlan.of(store)
    d = None if delta is None else torch.from_numpy(np.asarray(delta, np.float32)).cuda()
    spare = None if d is None or alias else torch.full_like(d, float("nan"))
    out = E.enqueue_input_grad(model, plan, torch.from_numpy(np.asarray(dz, np.float32)).cuda(), d, alpha, radius,
                               precision=precision, outputs=outputs, _delta_out=spare)
    counts = _np(plan._noise["input_grad"]["counts_d"])
    if alias and "delta" in out:
        assert out["delta"].data_ptr() == d.data_ptr()
    res = {("step" if k == "delta" else k): _np(v) for k, v in out.items()}
    res["counts"] = counts
    return res


# ---- 1. the exact grid --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", ["f32", "f16", "bf16"])
@pytest.mark.parametrize("precision", ["fp32", "fp16"])
def test_exact_grid(precision, dt):
    """Lengths 1, 32, 64: grad and the step are the float64 reference's bits, frame_l1 within 768 u.  Lengths 31, 33,
    65: (H + 4) u S (fp16: + 2^-11 S), signs and steps equal wherever |G_ref| exceeds it.  Rows past each length are
    0, the utterance without frames is harmless, the counts are exact."""
    feats, sizes, offsets, params, dz, delta, model = _exact()
    store = _exact_store(dt)
    for kw in (dict(alpha=0.25), dict(delta=delta, alpha=0.25, radius=0.5),
               dict(delta=delta, alpha=0.125, alias=True), dict(delta=delta, alpha=-0.25, radius=0.0)):
        got = _run(model, store, dz, precision=precision, **kw)
        ref = R.reference(feats, sizes, offsets, params, dz, kw.get("delta"), kw["alpha"], kw.get("radius", np.inf))
        fails = R.exact_failures(got, ref, sizes, fp16=precision == "fp16")
        assert not fails, (kw.get("alpha"), fails)
        v = R.valid_rows(sizes)
        zeros = int((got["grad"][v] == 0).sum())
        np.testing.assert_array_equal(got["counts"], [sizes.sum(), 0, zeros, 0])
        odd = ~np.isin(np.repeat(sizes, 32 * ((sizes + 31) // 32)), R.EXACT_POW2)
        assert ((got["grad"][v & ~odd] == 0) == (ref["grad"][v & ~odd] == 0)).all()
        assert (ref["grad"][v & ~odd] == 0).sum() >= 1          # sgn(0) = 0 is exercised


# ---- 2. the random fixture ----------------------------------------------------------------------------------------
def test_random_fixture_fp32_within_the_derived_bound():
    feats, sizes, offsets, labels, params, dz, ref, model, store = _random()
    got = _run(model, store, dz, alpha=1.0)
    ratio, bad, unchecked = R.check_grad(got["grad"], ref, sizes, flips=True)
    dis = R.sign_disagreement(got["grad"], ref, sizes)
    l1 = R.worst(got["frame_l1"] - np.abs(got["grad"].astype(np.float64)).sum(1),
                 R.D * R.U * np.abs(got["grad"].astype(np.float64)).sum(1))
    print("fp32: worst error / bound %.3f, %d sign mismatches among the checked, %.2f %% unchecked, sign disagreement "
          "%.4f %%, frame_l1 worst error / bound %.3f" % (ratio, bad, 100 * unchecked, 100 * dis, l1))
    assert ratio <= 1.0 and bad == 0
    assert unchecked <= 0.015
    assert dis <= 0.0005
    assert l1 <= 1.0
    v = R.valid_rows(sizes)
    assert not got["grad"][~v].any() and not got["step"][~v].any() and not got["frame_l1"][~v].any()
    np.testing.assert_array_equal(got["step"][v], np.sign(got["grad"][v]))
    np.testing.assert_array_equal(got["counts"], [sizes.sum(), 0, int((got["grad"][v] == 0).sum()), 0])


def test_random_fixture_fp16_signs():
    feats, sizes, offsets, labels, params, dz, ref, model, store = _random()
    got = _run(model, store, dz, alpha=1.0, precision="fp16")
    dis = R.sign_disagreement(got["grad"], ref, sizes)
    print("fp16 operands: sign disagreement %.4f %%" % (100 * dis))
    assert dis <= 0.005
    assert got["counts"][0] == sizes.sum() and got["counts"][1] == 0


# ---- 3. identities ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["fp32", "fp16"])
def test_identities(precision):
    feats, sizes, offsets, labels, params, dz, ref, model, store = _random()
    delta = R.to_explicit(R.q(np.random.RandomState(4).uniform(-0.5, 0.5, feats.shape), 2.0 ** -6), sizes, offsets)
    a = _run(model, store, dz, delta, 0.0625, 0.25, precision)
    b = _run(model, store, dz, delta, 0.0625, 0.25, precision)
    for k in ("grad", "step", "frame_l1", "counts"):                      # two calls write the same bits
        assert a[k].tobytes() == b[k].tobytes(), k
    none = _run(model, store, dz, None, 0.0625, 0.25, precision)          # delta == NULL equals delta = 0
    zero = _run(model, store, dz, np.zeros_like(delta), 0.0625, 0.25, precision)
    for k in ("grad", "step", "frame_l1", "counts"):
        assert none[k].tobytes() == zero[k].tobytes(), k
    clamp = _run(model, store, dz, delta, 0.0, 0.25, precision)           # alpha = 0 returns clamp(delta)
    np.testing.assert_array_equal(clamp["step"], np.clip(delta, -0.25, 0.25))
    # the same utterances in another order: another slab-to-workgroup assignment
    order = np.array([5, 0, 6, 2, 4, 1, 3])
    sub = store.subset(order)
    so, sp = R.slab_prefix(sizes), R.slab_prefix(sizes[order])
    delta_p = np.zeros_like(delta)
    for k, i in enumerate(order):
        delta_p[32 * sp[k]:32 * sp[k + 1]] = delta[32 * so[i]:32 * so[i + 1]]
    p = _run(model, sub, dz[order], delta_p, 0.0625, 0.25, precision)
    for k, i in enumerate(order):
        for name in ("grad", "step", "frame_l1"):
            assert p[name][32 * sp[k]:32 * sp[k + 1]].tobytes() == a[name][32 * so[i]:32 * so[i + 1]].tobytes(), (name, i)
    np.testing.assert_array_equal(p["counts"], a["counts"])


def test_captured_call_replays_the_eager_result():
    feats, sizes, offsets, labels, params, dz, ref, model, store = _random()
    plan = E.EvalPlan.of(store)
    d = torch.from_numpy(dz).cuda()
    delta = torch.from_numpy(R.to_explicit(R.q(np.random.RandomState(4).uniform(-0.5, 0.5, feats.shape), 2.0 ** -6),
                                           sizes, offsets)).cuda()
    eager = E.enqueue_input_grad(model, plan, d, delta.clone(), 0.0625, 0.25, outputs=ALL)
    counts = plan._noise["input_grad"]["counts_d"]
    want = counts.clone()
    torch.cuda.synchronize()
    work = delta.clone()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = E.enqueue_input_grad(model, plan, d, work, 0.0625, 0.25, outputs=ALL)
    work.copy_(delta)
    counts.fill_(-1)                                     # the call itself zeroes its counts
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(counts, want)
    for k in ALL:
        assert torch.equal(_bits(out[k]), _bits(eager[k])), k


# ---- 4. FGSM end to end -------------------------------------------------------------------------------------------
def test_fgsm_end_to_end():
    feats, sizes, offsets, labels, params, dz, ref, model, store = _random()
    g = np.load(GOLDEN)
    res = E.evaluate_adversarial_store(model, store, GOLDEN_EPS, outputs=("logits", "pred", "direction"))
    assert res["epsilons"] == [0.0] + list(GOLDEN_EPS) and res["n_levels"] == 4 and res["n_nonfinite_grad"] == 0
    assert [lv["epsilon"] for lv in res["levels"]] == res["epsilons"]
    direction = _np(res["direction"])
    v = R.valid_rows(sizes)
    assert set(np.unique(direction)) <= {-1.0, 0.0, 1.0} and not direction[~v].any()
    # level 0 is dad_eval_split, bit for bit
    clean = E.evaluate_store(model, store, outputs=("logits", "pred"))
    assert torch.equal(_bits(res["logits"][0]), _bits(clean["logits"]))
    assert torch.equal(res["pred"][0], clean["pred"])
    # each level against float64 at x + eps * (the device's direction)
    logits = _np(res["logits"])
    for k, e in enumerate(GOLDEN_EPS):
        zk = R.forward64(feats, sizes, offsets, params, np.float32(e) * direction)
        np.testing.assert_allclose(logits[k + 1], zk, rtol=1e-5, atol=1e-4)
    # the direction against the reference model's signs, and its logits where the two directions are the same
    gold = R.to_explicit(g["sign"].astype(np.float32), sizes, offsets)
    dis = (direction[v] != gold[v]).mean()
    soff = R.slab_prefix(sizes)
    same = [i for i, L in enumerate(sizes)
            if L > 0 and np.array_equal(direction[32 * soff[i]:32 * soff[i + 1]], gold[32 * soff[i]:32 * soff[i + 1]])]
    print("direction against the golden signs: %.4f %% differ; %d of 6 utterances equal" % (100 * dis, len(same)))
    assert dis <= 0.0005
    assert len(same) >= 4
    for k in range(len(GOLDEN_EPS)):
        np.testing.assert_allclose(logits[k + 1][same], g["logits"][k][same], rtol=1e-5, atol=1e-4)
    # an ascent direction, without a tolerance: at eps = 0.01 no random sign pattern raises the loss more
    e = np.float32(GOLDEN_EPS[0])
    mine = R.ce_loss(R.forward64(feats, sizes, offsets, params, e * direction), labels)
    rs = np.random.RandomState(8)
    for _ in range(8):
        r = R.to_explicit(np.sign(rs.standard_normal(feats.shape)).astype(np.float32), sizes, offsets)
        other = R.ce_loss(R.forward64(feats, sizes, offsets, params, e * r), labels)
        assert (mine[sizes > 0] >= other[sizes > 0]).all()
    # the curve shares noise_response_curve's axis
    curve = E.adversarial_response_curve(model, store)
    assert curve["sigmas"] == list(E.default_noise_levels()) and len(curve["accuracy"]["mean"]) == 3
    ig = E.input_gradients(model, store)
    np.testing.assert_array_equal(np.sign(_np(ig["grad"])), direction)
    utt = np.array([_np(ig["frame_l1"])[32 * soff[i]:32 * soff[i + 1]].astype(np.float64).sum() for i in range(len(sizes))])
    np.testing.assert_allclose(_np(ig["utt_l1"]), utt, rtol=1e-5)


# ---- 5. PGD -------------------------------------------------------------------------------------------------------
def test_pgd_step_by_step_on_the_exact_grid():
    feats, sizes, offsets, params, dz0, _, model = _exact()
    store = _exact_store("f32")
    plan = E.EvalPlan.of(store)
    eps, alpha, steps = 0.25, 0.125, 3
    labels = store.labels_d
    delta = torch.zeros((32 * plan.slabs, 768), dtype=torch.float32, device="cuda")
    v = R.valid_rows(sizes)
    for j in range(steps):
        z = E.enqueue_eval_noise(model, plan, (1.0,), outputs=("logits",), noise=delta)["logits"][0]
        dz = E._ce_cotangent(z, labels)                  # from the device's own probabilities
        before = _np(delta).copy()
        E.enqueue_input_grad(model, plan, dz, delta, alpha, eps, outputs=("delta",))
        after = _np(delta)
        ref = R.reference(feats, sizes, offsets, params, _np(dz), before, alpha, eps)
        sure = np.abs(ref["grad"]) > R.grad_bound(ref)
        np.testing.assert_array_equal(after[sure], ref["step"][sure])
        assert sure[v].mean() > 0.99
        assert np.abs(after).max() <= eps and not after[~v].any()
    res = E.evaluate_adversarial_store(model, store, [eps], steps=steps, alpha=alpha, outputs=("direction", "logits"))
    assert torch.equal(_bits(res["direction"][0]), _bits(delta))
    assert res["n_levels"] == 2 and res["epsilons"] == [0.0, eps]
    # one step of size eps is FGSM (eps a power of two: scaling the direction commutes with every rounding)
    one = E.evaluate_adversarial_store(model, store, [eps], steps=1, alpha=eps, outputs=("logits", "pred", "break_level"))
    fgsm = E.evaluate_adversarial_store(model, store, [eps], outputs=("logits", "pred", "break_level"))
    for k in ("logits", "pred", "break_level"):
        assert torch.equal(_bits(one[k]), _bits(fgsm[k])), k
    np.testing.assert_array_equal(one["block"][:L_.EN_COUNTS], fgsm["block"][:L_.EN_COUNTS])
    # the default step size is 2.5 eps / steps
    dflt = E.evaluate_adversarial_store(model, store, [0.24], steps=3, outputs=("direction",))
    assert float(dflt["direction"][0].abs().max()) <= np.float32(0.24)


# ---- 6. error paths and the Python surface ------------------------------------------------------------------------
def test_error_paths():
    feats, sizes, offsets, labels, params, dz, ref, model, store = _random()
    with pytest.raises(ValueError, match="unknown target"):
        E.evaluate_adversarial_store(model, store, [0.1], target="loss")
    with pytest.raises(ValueError, match="between 1 and 7"):
        E.evaluate_adversarial_store(model, store, [0.1] * 8)
    bare = D.FeatureStore(feats, sizes, offsets)
    with pytest.raises(ValueError, match="no labels"):
        E.evaluate_adversarial_store(model, bare, [0.1])
    with pytest.raises(ValueError, match="no labels"):
        E.input_gradients(model, bare)
    res = E.evaluate_adversarial_store(model, bare, [0.1], target="pred")       # against its own predictions
    assert res["n_labelled"] == 0 and res["flips"][0] == 0
    with pytest.raises(RuntimeError, match="model on"):
        E.evaluate_adversarial_store(PKG.SSRLModel(), store, [0.1])
    with pytest.raises(L_.DadError):
        E.evaluate_adversarial_store(model, store, [0.1], precision="bf16")
    plan = E.EvalPlan.of(store)
    d = torch.from_numpy(dz).cuda()
    with pytest.raises(L_.DadError, match="1004"):
        E.enqueue_input_grad(model, plan, d, precision="bf16")
    with pytest.raises(ValueError, match="unknown output"):
        E.enqueue_input_grad(model, plan, d, outputs=("logits",))
    with pytest.raises(ValueError, match="dz must be"):
        E.enqueue_input_grad(model, plan, d[:3])
    with pytest.raises(ValueError, match="delta must be"):
        E.enqueue_input_grad(model, plan, d, delta=torch.zeros(3, 768, device="cuda"))
    with pytest.raises(ValueError, match="alpha"):
        E.enqueue_input_grad(model, plan, d, alpha=float("inf"))
    with pytest.raises(ValueError, match="radius"):
        E.enqueue_input_grad(model, plan, d, radius=-1.0)
    # non-finite cotangents are counted and reported
    bad = d.clone()
    bad[3, 0] = float("nan")
    step = E.enqueue_input_grad(model, plan, bad, alpha=1.0, outputs=("delta",))["delta"]
    rows = slice(32 * int(R.slab_prefix(sizes)[3]), 32 * int(R.slab_prefix(sizes)[4]))
    assert not step[rows].any() and step[:rows.start].any()            # a non-finite element takes step 0
    assert int(plan._noise["input_grad"]["counts_d"][L_.IG_NONFINITE]) > 0
    with pytest.raises(L_.DadError, match="not finite"):
        E._read_ig_counts(plan)
    rep = E.worst_case_report(model, model, store, draws=2)
    assert set(rep) == {"random", "worst_case"}
    assert rep["random"]["trained_weights"]["sigmas"] == rep["worst_case"]["trained_weights"]["sigmas"]
