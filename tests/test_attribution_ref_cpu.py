"""The float64 closed form of tests/attribution_ref.py on the CPU: the identities dad.h states, every listed wrong
variant outside the bounds, the reference model's quadrature golden within the midpoint term, the fp32 and the
fp16-operand restatements within their bounds, and the argument checks of the Python layer that need no library."""
import functools
import os

import numpy as np
import pytest
import torch

import attribution_ref as R
import dadpkg
from golden.gen_attribution_golden import ATTR_OF, POINTS, mean_frame
from golden.gen_input_grad_golden import inputs as golden_inputs
from oracle import data_oracle as do

GOLDEN = os.path.join(dadpkg.ROOT, "tests", "golden", "eval_attribution.npz")
BASELINES = ("zero", "mean")


@functools.lru_cache(None)
def _fixture(bname):
    feats, sizes, offsets, _ = golden_inputs()
    params = do.eval_weights(23)[0]
    z = R.forward64(feats, sizes, offsets, params)
    target = z.argmax(1)
    dz = R.onehot_dz(target)
    xb = None if bname == "zero" else mean_frame(feats)
    return feats, sizes, offsets, params, target, dz, xb, R.reference(feats, sizes, offsets, params, dz, xb)


@pytest.mark.parametrize("bname", BASELINES)
def test_identities_in_float64(bname):
    feats, sizes, offsets, params, target, dz, xb, ref = _fixture(bname)
    v = R.valid_rows(sizes)
    # sum_d attr_t[d] = frame_attr_t, and completeness: utt_total = dz . (z(x) - z(x'))
    scale = np.abs(ref["attr"]).sum(1)
    assert (np.abs(ref["attr"].sum(1) - ref["frame_attr"])[v] <= 1e-13 * scale[v]).all()
    has = sizes > 0
    want = (dz * (ref["z1"] - ref["z0"])).sum(1)
    assert np.abs(ref["utt_total"] - want)[has].max() <= 1e-13 * np.abs(ref["frame_attr"]).sum()
    assert ref["utt_total"][~has].tolist() == [0.0] and not ref["chan_attr"][~has].any()
    np.testing.assert_allclose(ref["chan_attr"].sum(1), ref["utt_total"], rtol=0, atol=1e-13)
    # the fixture makes the point of the method: close to half of the hidden units switch along the path
    assert 0.40 <= ref["switch_share"] <= 0.55
    assert ref["counts"][0] == sizes.sum() and ref["counts"][1] == 0
    assert ref["counts"][2] + ref["counts"][3] <= sizes.sum() * R.H


def test_lambda_is_the_active_length_of_the_path():
    rs = np.random.RandomState(3)
    p0, p1 = rs.standard_normal(4000), rs.standard_normal(4000)
    p0[:10], p1[10:20] = 0.0, 0.0
    lam = R.lam_of(p0, p1)
    alpha = (np.arange(20000) + 0.5) / 20000
    frac = ((p0[:, None] + alpha[None, :] * (p1 - p0)[:, None]) > 0).mean(1)
    assert np.abs(lam - frac).max() <= 1.0 / 20000
    np.testing.assert_allclose(lam * (p1 - p0), np.maximum(p1, 0) - np.maximum(p0, 0), rtol=0, atol=1e-15)
    assert ((lam >= 0) & (lam <= 1)).all()


@pytest.mark.parametrize("variant", R.VARIANTS)
def test_wrong_answers_land_outside_the_bounds(variant):
    """With the mean baseline (a zero baseline cannot tell x from x - x') every variant fails the comparison the GPU
    test makes, random-operand sensitivity term included."""
    feats, sizes, offsets, params, target, dz, xb, ref = _fixture("mean")
    wrong = R.reference(feats, sizes, offsets, params, dz, xb, variant=variant)
    ratios, fails = R.check(wrong, ref, sizes, sens=True, counts=False)
    assert fails, (variant, ratios)
    assert max(ratios.values()) > 10.0 or any("rows past" in f for f in fails), (variant, ratios)


@pytest.mark.parametrize("bname", BASELINES)
def test_restatements_in_the_kernels_formats(bname):
    feats, sizes, offsets, params, target, dz, xb, ref = _fixture(bname)
    r32 = R.reference(feats, sizes, offsets, params, dz, xb, dtype=np.float32)
    ratios, fails = R.check(r32, ref, sizes, sens=True, counts=False)
    print("fp32 restatement, worst error / bound:", ratios)
    assert not fails, fails
    # fp16 operands: its own float32 restatement against the float64 one, the forward term from the rounded operands
    r16 = R.reference(feats, sizes, offsets, params, dz, xb, fp16_operands=True)
    r16_32 = R.reference(feats, sizes, offsets, params, dz, xb, dtype=np.float32, fp16_operands=True)
    ratios, fails = R.check(r16_32, r16, sizes, fp16=True, sens=True, counts=False)
    print("fp16-operand restatement, worst error / bound:", ratios)
    assert not fails, fails


@pytest.mark.parametrize("bname", BASELINES)
def test_golden_quadrature_within_the_midpoint_term(bname):
    """The reference model's autograd at 256 midpoints against the closed form: the midpoint term of the crossing
    units plus the closed form's own fp32-storage allowance (the golden stores attr as float32: 2^-24 relative)."""
    feats, sizes, offsets, params, target, dz, xb, ref = _fixture(bname)
    g = np.load(GOLDEN)
    assert int(g["points"]) == POINTS == R.GOLDEN_POINTS
    np.testing.assert_array_equal(g["target"][sizes > 0], target[sizes > 0])
    if bname == "mean":
        np.testing.assert_array_equal(g["mean_frame"], xb)
    soff = R.slab_prefix(sizes)
    worst_share = 0.0
    for i in ATTR_OF:
        r = slice(32 * int(soff[i]), 32 * int(soff[i]) + int(sizes[i]))
        got = g["attr_%s_%d" % (bname, i)].astype(np.float64)
        lim = ref["mid"][r] + R.U * np.abs(ref["attr"][r])
        ratio = R.worst(got - ref["attr"][r], lim)
        worst_share = max(worst_share, ratio)
        assert ratio <= 1.0, (i, ratio)
    fa = R.to_explicit(g["frame_attr_" + bname], sizes, offsets)
    assert R.worst(fa - ref["frame_attr"], ref["mid"].sum(1) + 1e-13 * np.abs(ref["attr"]).sum(1)) <= 1.0
    tot_lim = np.array([ref["mid"][32 * int(soff[i]):32 * int(soff[i + 1])].sum() for i in range(len(sizes))])
    assert R.worst(g["utt_total_" + bname] - ref["utt_total"], tot_lim + 1e-13) <= 1.0
    print("golden attr, worst error / midpoint term: %.3f" % worst_share)
    assert worst_share > 0.01           # the term is not vacuous: the quadrature does err at the crossings


def test_exact_problem_is_exact_in_both_formats():
    feats, sizes, offsets, params, dz, xb = R.exact_problem((1, 32, 0, 64, 31, 33, 65))
    W1, b1 = params[0], params[1]
    for a in (feats, W1, xb):
        np.testing.assert_array_equal(a.astype(np.float16).astype(np.float32), a)
    r64 = R.reference(feats, sizes, offsets, params, dz, xb)
    r32 = R.reference(feats, sizes, offsets, params, dz, xb, dtype=np.float32)
    r16 = R.reference(feats, sizes, offsets, params, dz, xb, fp16_operands=True)
    # the same case decisions and counts in every format, and no pre-activation at 0
    for r in (r32, r16):
        np.testing.assert_array_equal(r["counts"], r64["counts"])
    assert r64["counts"][2] > 0 and r64["counts"][3] > 0
    ratios, fails = R.check(r32, r64, sizes, counts=True)
    assert not fails, fails
    ratios, fails = R.check(r16, r64, sizes, fp16=True)
    assert not fails, fails


# ---- the argument checks of the Python layer that need no library -------------------------------------------------
def test_python_argument_checks():
    E = dadpkg.pkg().evaluate
    with pytest.raises(ValueError, match="unknown target"):
        E.integrated_gradients(None, None, target="logprob")
    for bad in (4, -1, 1.5, True):
        with pytest.raises(ValueError, match="class index"):
            E.integrated_gradients(None, None, target=bad)
    with pytest.raises(ValueError, match="unknown output"):
        E.integrated_gradients(None, None, outputs=("grad",))
    with pytest.raises(ValueError, match="baseline"):
        E.integrated_gradients(None, None, baseline=torch.zeros(767))
    with pytest.raises(ValueError, match="baseline"):
        E.integrated_gradients(None, None, baseline=torch.zeros(768, dtype=torch.float64))
    with pytest.raises(ValueError, match="baseline"):
        E.integrated_gradients(None, None, baseline="median")
    with pytest.raises(ValueError, match="baseline"):
        E.enqueue_attribution(None, None, None, baseline="mean")      # 'mean' is integrated_gradients' alone
    with pytest.raises(ValueError, match="unknown output"):
        E.enqueue_attribution(None, None, None, outputs=("frame_l1",))
    assert E._at_check_target(3) == 3 and E._at_check_target("margin") == "margin"


def test_margin_cotangent():
    z = np.array([[1.0, 3.0, 2.0, 0.0], [5.0, 1.0, 5.0, 0.0]])
    np.testing.assert_array_equal(R.margin_dz(z, [1, 0]), [[0, 1, -1, 0], [1, 0, -1, 0]])
    E = dadpkg.pkg().evaluate

    class P:
        labels_d = None
    tgt, dz = E._at_cotangent(P, torch.tensor(z, dtype=torch.float32), torch.tensor([1, 0]), "margin")
    np.testing.assert_array_equal(dz.numpy(), [[0, 1, -1, 0], [1, 0, -1, 0]])
    tgt, dz = E._at_cotangent(P, torch.tensor(z, dtype=torch.float32), torch.tensor([1, 0]), 2)
    np.testing.assert_array_equal(dz.numpy(), [[0, 0, 1, 0], [0, 0, 1, 0]])
    with pytest.raises(ValueError, match="no labels"):
        E._at_cotangent(P, torch.tensor(z, dtype=torch.float32), torch.tensor([1, 0]), "label")


def test_binding_matches_the_header():
    L = dadpkg.pkg()._lib
    text = open(os.path.join(dadpkg.ROOT, "include", "dad.h")).read()
    for name, val in (("DAD_AT_FRAMES", L.AT_FRAMES), ("DAD_AT_NONFINITE", L.AT_NONFINITE), ("DAD_AT_CROSS", L.AT_CROSS),
                      ("DAD_AT_ONE", L.AT_ONE), ("DAD_AT_COUNTS", L.AT_COUNTS), ("DAD_AT_PLAN_SLOTS", L.AT_PLAN_SLOTS)):
        assert ("#define %s %d " % (name, val) in text) or ("#define %s %d\n" % (name, val) in text), name
    fields = [f for f, _ in L.DadAttributionArgs._fields_]
    body = text[text.index("typedef struct dad_attribution_args {"):text.index("} dad_attribution_args;")]
    order = [ln.split(";")[0].split()[-1].lstrip("*") for ln in body.splitlines()[1:] if ";" in ln]
    assert fields == order
    for name in ("dad_attribution", "dad_attribution_workspace_bytes", "dad_attribution_plan"):
        assert name in L.EXPORTS and name in L.OPTIONAL_EXPORTS
