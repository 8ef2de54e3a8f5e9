"""The fused step, in all three precisions, on inputs every encoder operand of which is exact in fp16 and bf16
(tests/exact_problem.py), against a float64 reference with a bound derived from the reference alone.

On these problems the ReLU' pattern and the DACP mask cannot differ between the modes, the gates are open
(the strong slabs carry 19 - 50 % of the weight gradient's magnitude sum) and the only rounding a 16-bit step adds
is the weight gradient's per-(utterance, h) scale, so every gradient element is held to
    |g - g_ref| <= (eps_op + n_rows 2^-24 + 1e-4) S_g          (eps_op: 0 fp32, 2^-11 fp16, 2^-8 bf16; dW1 only)
(dW1: plus the tail term, the worst-case fp32 error of the classifier backward where dL/de cancels.  It was added
after the fp32 mode measured 1.26 x the bound without it at B1T1/Bn2Tn3, epoch 60, in an element whose dL/de
cancels 2300-fold; every case also prints dW1 against the bound without the term, which is not asserted)
and the embeddings / logits to a few fp32 roundings in EVERY precision; tests/test_exact_problem_cpu.py shows that
the references sit inside these bounds and that a dropped slab, a wrong 1 / len, a mis-scaled hidden unit or the
wrong augmented input sits at least 10x outside.  Derivations: exact_problem's docstring.

  matrix      {fp32, fp16, bf16} x the five edge geometries of test_gpu_parity x epoch {0 (warm-up, clean slabs
              only), 60}
  split-K     B5T33/Bn7Tn31 and B12T45/Bn20Tn70 with DADStep(splits = auto, 3, 5), fp32 and fp16: split boundaries
              inside utterances, splits holding clean and strong slabs together; the split count the plan uses is
              printed (the 16-bit path raises small values)
  store-fed   B5T33/Bn7Tn31 read in place from feature stores of f32, fp16 and bf16 rows (the same values here),
              dense and ragged, fp16 and bf16: DADStep.step takes explicit draws together with store batches, so
              dad_prep_s16 / _rg, dad_encode_wp*_rg and dad_wgrad_direct*_rg meet the float64 reference directly
Every case prints its worst err / bound per tensor; with DAD_EXACT_JSON set the ratios are also written there
(profiles/exact_operands.json is that file from an MI355X run)."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

import dadpkg
import exact_problem as X
import gpu_harness as gh
from test_gpu_parity import EDGE, TOL

pytestmark = pytest.mark.gpu
assert X.GEOMS == EDGE
PRECS = ["fp32", "fp16", "bf16"]
LOSSES = ("total_loss", "supervised_ce_loss", "consistency_loss", "ecda_loss")
_MEASURED = {}


@pytest.fixture(scope="module", autouse=True)
def _dump_measured():
    yield
    path = os.environ.get("DAD_EXACT_JSON")
    if path and _MEASURED:
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "w") as f:
            json.dump(_MEASURED, f, indent=1, sort_keys=True)


def _check(o, step, ref, prec, epoch, what):
    """Every assertion of one case; the figures are printed and recorded before anything is asserted.  A reference
    with the supervised-contrastive term (ref["scl"], tests/test_gpu_exact_scl.py) also holds the step's scl_loss
    to 1e-4 of the float64 loss (gpu_harness.close's measure, as tests/test_gpu_scl.py does) and the total to the
    oracle's plus the weighted term."""
    r = ref["oracle"]
    scl = ref.get("scl")
    want = {k: (ref["total_loss"] if scl and k == "total_loss" else r[k]) for k in LOSSES}
    ratios = dict(X.forward_ratios(o, ref))
    ratios.update(X.grad_ratios(o["grads"], ref, prec))
    loss_err = {k: abs(o[k] - want[k]) / max(1.0, abs(want[k])) for k in LOSSES}
    if scl:
        loss_err["scl_loss"] = abs(o["scl_loss"] - scl["loss"]) / max(1e-6, abs(scl["loss"]))
    # for the record only: dW1 against the bound without exact_problem's tail term
    plain = X.worst(o["grads"][0] - ref["grads"][0], X.bound("dW1", prec, ref["n_rows"]) * ref["S"][0])
    print("%s: %s | dW1 without the tail term %.3g | loss rel %s" % (
        what, {k: float("%.3g" % v) for k, v in ratios.items()}, plain, {k: float("%.2g" % v) for k, v in loss_err.items()}))
    _MEASURED[what] = {k: float("%.4g" % v) for k, v in ratios.items()}
    if epoch >= 30:
        np.testing.assert_array_equal(o["mask"], r["mask"], err_msg=what)
    for k in LOSSES:
        assert loss_err[k] <= TOL, (what, k, o[k], want[k])
    if scl:
        assert loss_err["scl_loss"] < TOL, (what, o["scl_loss"], scl["loss"])
    else:
        assert o.get("scl_loss", 0.0) == 0.0, what
    bad = {k: v for k, v in ratios.items() if not v <= 1.0}
    assert not bad, "%s: err / bound above 1: %s" % (what, bad)
    assert int(step.range_flag()) == 0, what


def _step(prec, st, splits=0):
    step = gh.make_step(X.cfg(), precision=prec, splits=splits)
    gh.load_state(step, st)
    return step


@pytest.mark.parametrize("epoch", [0, 60])
@pytest.mark.parametrize("geom", EDGE, ids=X.geom_id)
@pytest.mark.parametrize("prec", PRECS)
def test_step_on_exact_operands(prec, geom, epoch):
    inp, st, ref = X.case(geom, epoch)
    step = _step(prec, st)
    o = gh.run_step(step, inp, epoch)
    _check(o, step, ref, prec, epoch, "%s %s e%d" % (prec, X.geom_id(geom), epoch))


def _splits_used(step, inp, epoch):
    lib = dadpkg.pkg()._lib
    (Bc, Tc), (Bn, Tn) = inp["mc"].shape, inp["mn"].shape
    info = lib.DadStepPlanInfo()
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    assert lib.lib().dad_step_plan(step.make_config(Bc, Tc, Bn, Tn, epoch), None, None, 0, cus, ctypes.byref(info)) == 0
    return int(info.splits)


@pytest.mark.parametrize("splits", [0, 3, 5], ids=["auto", "3", "5"])
@pytest.mark.parametrize("geom", [EDGE[1], EDGE[3]], ids=X.geom_id)
@pytest.mark.parametrize("prec", ["fp32", "fp16"])
def test_split_k_on_exact_operands(prec, geom, splits):
    inp, st, ref = X.case(geom, 60)
    step = _step(prec, st, splits=splits)
    used = _splits_used(step, inp, 60)
    o = gh.run_step(step, inp, 60)
    what = "%s %s splits %s" % (prec, X.geom_id(geom), splits or "auto")
    print("%s: the plan uses %d splits" % (what, used))
    _check(o, step, ref, prec, 60, what)
    _MEASURED[what]["splits_used"] = used


def _store(x, pad, labels, dtype):
    """A feature store holding the batch's utterances back to back (their frames only), and its store batch."""
    D = dadpkg.pkg().data
    lens = (~pad).sum(1)
    rows = np.concatenate([x[b, :lens[b]] for b in range(len(lens))], 0)
    offsets = np.concatenate([[0], np.cumsum(lens)[:-1]])
    store = D.FeatureStore(rows, lens, offsets, labels, dtype=dtype)
    return store.batch_index(np.arange(len(lens)), with_labels=labels is not None)


@pytest.mark.parametrize("ragged", [False, True], ids=["dense", "ragged"])
@pytest.mark.parametrize("store_dtype", [torch.float32, torch.float16, torch.bfloat16], ids=["f32", "fp16", "bf16"])
@pytest.mark.parametrize("prec", ["fp16", "bf16"])
def test_store_fed_step_on_exact_operands(prec, store_dtype, ragged, monkeypatch):
    geom = EDGE[1]
    inp, st, ref = X.case(geom, 60)

    def refuse(self):
        raise AssertionError("StoreFeats.materialize(): the step made a padded copy of a store batch")
    monkeypatch.setattr(dadpkg.pkg().data.StoreFeats, "materialize", refuse)
    step = _step(prec, st)
    step.ragged = ragged
    clean = _store(inp["xc"], inp["mc"], inp["yc"], store_dtype)
    noisy = _store(inp["xn"], inp["mn"], None, store_dtype)
    assert clean["net_input"]["padding_mask"].shape == inp["mc"].shape          # (one utterance has every frame)
    assert noisy["net_input"]["padding_mask"].shape == inp["mn"].shape
    draws = gh.batches(inp)[2]
    cfg = step._batch_structs(clean, noisy, 60, None, draws)[0]
    assert cfg.ragged == int(ragged)
    losses = step.step(clean, noisy, 60, draws=draws)
    torch.cuda.synchronize()
    Bc, Bn = inp["xc"].shape[0], inp["xn"].shape[0]
    o = {k: (v.detach().cpu().numpy() if torch.is_tensor(v) else v) for k, v in step.outputs(Bc, Bn).items()}
    o.update({k: float(v) for k, v in losses.items()})
    o["grads"] = gh.unflat(o["grad"])
    what = "%s %s store %s %s" % (prec, X.geom_id(geom), str(store_dtype).split(".")[-1], "ragged" if ragged else "dense")
    _check(o, step, ref, prec, 60, what)
