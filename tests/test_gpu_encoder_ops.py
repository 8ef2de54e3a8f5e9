"""The modular encoder operators (csrc/encoder_ops.hip: dad_encoder_forward / dad_encoder_backward) and the prediction
head (csrc/eval.hip: dad_predict_head) against float64 references on exactly representable operands, with bounds
derived from the references alone (tests/operators_ref.py; its conditions and wrong-answer controls:
tests/test_operators_ref_cpu.py).

  forward    fp32, fp16 and bf16, through the entry point and through SSRLModel.set_precision: T = 1, T on the 32-frame
             slab and one past it, B = 1, a fully padded utterance (exactly 0), padding that ends inside a slab, padded
             frames that hold values, 1024 utterances, B = 1025 (DAD_E_SHAPE), a workspace of NaNs
  backward   the entry point and autograd through student_encoder: the recomputed ReLU' bits at the same geometries,
             dW1 / db1 elements no active frame feeds exactly 0, a workspace of NaNs
  head       B = 1, B not a multiple of the 4 waves of a block, exact logit ties (first maximum), logits spanning +-80
             (probabilities underflow under the entropy's + 1e-8), every combination of null outputs
Each test prints the worst measured error relative to its bound."""
import itertools

import numpy as np
import pytest
import torch

import dadpkg
import operators_ref as R

pytestmark = pytest.mark.gpu
PKG = dadpkg.pkg()
L = PKG._lib
PRECISIONS = {"fp32": L.PREC_FP32, "fp16": L.PREC_FP16, "bf16": L.PREC_BF16}
GEOMS = pytest.mark.parametrize("geom", R.ENC_GEOMS, ids=R.enc_id)


def _cuda(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return t.to("cuda", dtype) if dtype is not None else t.cuda()


def _p(t):
    return None if t is None else t.data_ptr()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int32) if a.dtype == np.float32 else a


def _operands(k):
    return _cuda(k["x"]), _cuda(k["pad"].astype(np.uint8)), _cuda(k["W1"]), _cuda(k["b1"])


def _workspace(B, T, fill):
    n = int(L.lib().dad_encoder_workspace_bytes(B, T))
    assert n > 0
    return torch.full((n,), fill, dtype=torch.uint8, device="cuda")


def _forward(k, precision, ws_fill=0, B=None):
    """dad_encoder_forward -> (rc, e numpy); the output starts as NaN; ws_fill 0xff: a workspace of NaNs."""
    x, pad, w1, b1 = _operands(k)
    e = torch.full((k["B"], R.H), float("nan"), device="cuda")
    ws = _workspace(k["B"], k["T"], ws_fill)
    rc = L.lib().dad_encoder_forward(x.data_ptr(), pad.data_ptr(), k["B"] if B is None else B, k["T"], w1.data_ptr(),
                                     b1.data_ptr(), e.data_ptr(), precision, ws.data_ptr(), _stream())
    torch.cuda.synchronize()
    return rc, e.cpu().numpy()


def _backward(k, ws_fill=0, B=None):
    x, pad, w1, b1 = _operands(k)
    de = _cuda(k["de"])
    dw1 = torch.full((R.H, R.D), float("nan"), device="cuda")
    db1 = torch.full((R.H,), float("nan"), device="cuda")
    ws = _workspace(k["B"], k["T"], ws_fill)
    rc = L.lib().dad_encoder_backward(x.data_ptr(), pad.data_ptr(), k["B"] if B is None else B, k["T"], w1.data_ptr(),
                                      b1.data_ptr(), de.data_ptr(), dw1.data_ptr(), db1.data_ptr(), ws.data_ptr(),
                                      _stream())
    torch.cuda.synchronize()
    return rc, dw1.cpu().numpy(), db1.cpu().numpy()


@pytest.fixture(scope="module")
def model():
    return PKG.SSRLModel().cuda()


def _load(model, k):
    with torch.no_grad():
        model.student_encoder.pre_net.weight.copy_(_cuda(k["W1"]))
        model.student_encoder.pre_net.bias.copy_(_cuda(k["b1"]))


def _check_forward(what, e, k, ref):
    assert np.all(np.isfinite(e)), what
    r = R.enc_forward_ratio(e, ref, k["T"])
    assert r <= 1.0, (what, r)
    for b in np.nonzero(k["lens"] == 0)[0]:
        assert not e[b].any(), (what, "fully padded row", b)
    return r


@pytest.mark.parametrize("prec", sorted(PRECISIONS))
@GEOMS
def test_encoder_forward_meets_the_embedding_bound(geom, prec, model):
    k = R.encoder_case(geom)
    ref = R.encoder_reference(k)
    rc, e = _forward(k, PRECISIONS[prec])
    assert rc == 0
    ratios = [_check_forward("entry point", e, k, ref)]
    rc, e_nan = _forward(k, PRECISIONS[prec], ws_fill=0xff)
    assert rc == 0
    np.testing.assert_array_equal(_bits(e_nan), _bits(e), err_msg="a workspace of NaNs changed the embeddings")
    _load(model, k)
    model.set_precision(PRECISIONS[prec])
    try:
        with torch.no_grad():
            e_mod = model.student_encoder(_cuda(k["x"]), _cuda(k["pad"])).cpu().numpy()
    finally:
        model.set_precision(L.PREC_FP32)
    ratios.append(_check_forward("set_precision", e_mod, k, ref))
    print("%s %s: worst |e - e_ref| / bound: entry point %.3g, module %.3g" % (R.enc_id(geom), prec, *ratios))


@GEOMS
def test_encoder_backward_meets_the_derived_bound(geom, model):
    k = R.encoder_case(geom)
    B, T = k["B"], k["T"]
    ref = R.encoder_reference(k)
    rc, dw1, db1 = _backward(k)
    assert rc == 0 and np.all(np.isfinite(dw1)) and np.all(np.isfinite(db1))
    rW, rb = R.enc_backward_ratios(dw1, db1, ref, B, T)        # (an element with S_g = 0 must be exactly 0)
    assert not dw1[ref["S_W1"].max(1) == 0].any()
    rc, dw1_nan, db1_nan = _backward(k, ws_fill=0xff)
    assert rc == 0
    np.testing.assert_array_equal(_bits(dw1_nan), _bits(dw1), err_msg="a workspace of NaNs changed dW1")
    np.testing.assert_array_equal(_bits(db1_nan), _bits(db1), err_msg="a workspace of NaNs changed db1")
    # autograd through student_encoder: d/dW1, d/db1 of sum(e * de)
    _load(model, k)
    enc = model.student_encoder
    enc.pre_net.weight.grad = enc.pre_net.bias.grad = None
    e = enc(_cuda(k["x"]), _cuda(k["pad"]))
    (e * _cuda(k["de"])).sum().backward()
    torch.cuda.synchronize()
    aW, ab = R.enc_backward_ratios(enc.pre_net.weight.grad.cpu().numpy(), enc.pre_net.bias.grad.cpu().numpy(), ref, B, T)
    enc.pre_net.weight.grad = enc.pre_net.bias.grad = None
    print("%s: worst err / (c u S), c = %d: entry point dW1 %.3g db1 %.3g, autograd dW1 %.3g db1 %.3g" % (
        R.enc_id(geom), R.enc_c(B, T), rW, rb, aW, ab))
    assert max(rW, rb, aW, ab) <= 1.0, (rW, rb, aW, ab)


def test_encoder_ops_at_the_batch_limit():
    geom = R.limit_geom()
    k = R.encoder_case(geom)
    B, T = k["B"], k["T"]
    assert B == L.DAD_MAX_BATCH
    ref = R.encoder_reference(k)
    ratios = {}
    for prec, code in sorted(PRECISIONS.items()):
        rc, e = _forward(k, code)
        assert rc == 0
        ratios[prec] = _check_forward(prec, e, k, ref)
    rc, dw1, db1 = _backward(k)
    assert rc == 0
    ratios["dW1"], ratios["db1"] = R.enc_backward_ratios(dw1, db1, ref, B, T)
    print("B1024T1: worst err / bound %s" % {n: float("%.3g" % v) for n, v in ratios.items()})
    assert max(ratios.values()) <= 1.0, ratios
    # one utterance more: refused before anything is launched
    big = dict(k, B=B + 1, x=np.concatenate([k["x"], k["x"][:1]]), pad=np.concatenate([k["pad"], k["pad"][:1]]),
               de=np.concatenate([k["de"], k["de"][:1]]))
    assert _forward(big, L.PREC_FP32)[0] == L.E_SHAPE
    assert _backward(big)[0] == L.E_SHAPE
    assert _forward(k, L.PREC_FP32, B=0)[0] == L.E_SHAPE and _forward(k, 7)[0] == L.E_ARG


# ------------------------------------------------------------------------------------- dad_predict_head
NAMES = ("logits", "probs", "score", "pred")


def _head(e, W2, b2, use_entropy, want=NAMES):
    """dad_predict_head -> {name: numpy} of the outputs asked for (the others are passed as null)."""
    B = e.shape[0]
    ed, wd, bd = _cuda(e), _cuda(W2), _cuda(b2)
    out = {"logits": torch.full((B, R.C), float("nan"), device="cuda"),
           "probs": torch.full((B, R.C), float("nan"), device="cuda"),
           "score": torch.full((B,), float("nan"), device="cuda"),
           "pred": torch.full((B,), -7, dtype=torch.int64, device="cuda")}
    rc = L.lib().dad_predict_head(ed.data_ptr(), B, wd.data_ptr(), bd.data_ptr(), int(use_entropy),
                                  *[_p(out[n]) if n in want else None for n in NAMES], _stream())
    torch.cuda.synchronize()
    assert rc == 0
    return {n: out[n].cpu().numpy() for n in want}


def _head_ratios(o, ref, use_entropy, probs=True):
    r = {"logits": R.worst(o["logits"] - ref["z"], ref["z_lim"]),
         "score": R.worst(o["score"] - ref["score"][use_entropy], R.score_lim(ref["score"][use_entropy]))}
    if probs:
        r["probs"] = R.worst(o["probs"] - ref["p"], ref["p_lim"])
    return r


@pytest.mark.parametrize("use_entropy", [True, False])
@pytest.mark.parametrize("B", R.HEAD_B)
def test_predict_head_meets_the_derived_bounds(B, use_entropy):
    e, W2, b2 = R.head_case(B)
    ref = R.head_reference(e, W2, b2)
    o = _head(e, W2, b2, use_entropy)
    assert all(np.all(np.isfinite(o[n])) for n in NAMES[:3])
    r = _head_ratios(o, ref, use_entropy)
    print("head B=%d entropy=%s: worst err / bound %s" % (B, use_entropy, {n: float("%.3g" % v) for n, v in r.items()}))
    assert max(r.values()) <= 1.0, r
    np.testing.assert_array_equal(o["pred"][ref["decided"]], ref["pred"][ref["decided"]])
    np.testing.assert_array_equal(o["pred"], o["logits"].argmax(1))


@pytest.mark.parametrize("use_entropy", [True, False])
def test_predict_head_takes_the_first_of_tied_logits(use_entropy):
    e, W2, b2 = R.head_case(37, "tie")
    lo, hi = R.tie_pair(W2, b2)
    ref = R.head_reference(e, W2, b2)
    o = _head(e, W2, b2, use_entropy)
    np.testing.assert_array_equal(_bits(o["logits"][:, lo]), _bits(o["logits"][:, hi]))
    on_top = ref["pred"] == lo
    assert np.all(o["pred"][on_top] == lo) and not (o["pred"] == hi).any()
    other = ~on_top & ref["decided"]
    np.testing.assert_array_equal(o["pred"][other], ref["pred"][other])
    r = _head_ratios(o, ref, use_entropy)
    assert max(r.values()) <= 1.0, r
    e, W2, b2 = R.head_case(5, "all_tie")
    o = _head(e, W2, b2, use_entropy)
    assert np.all(_bits(o["logits"]) == _bits(o["logits"][:, :1])) and np.all(o["pred"] == 0)
    np.testing.assert_array_equal(o["probs"], np.full((5, 4), 0.25, np.float32))


@pytest.mark.parametrize("use_entropy", [True, False])
def test_predict_head_survives_underflowing_probabilities(use_entropy):
    e, W2, b2 = R.head_case(37, "wide")
    ref = R.head_reference(e, W2, b2)
    o = _head(e, W2, b2, use_entropy)
    assert all(np.all(np.isfinite(o[n])) for n in NAMES[:3])
    assert (o["probs"] == 0).any() and np.all(o["probs"] >= 0)
    r = _head_ratios(o, ref, use_entropy, probs=False)
    print("head wide entropy=%s: %d probabilities are 0; worst err / bound %s" % (
        use_entropy, (o["probs"] == 0).sum(), {n: float("%.3g" % v) for n, v in r.items()}))
    assert max(r.values()) <= 1.0, r
    np.testing.assert_array_equal(o["pred"][ref["decided"]], ref["pred"][ref["decided"]])


def test_predict_head_null_outputs_in_any_combination():
    e, W2, b2 = R.head_case(5)
    full = _head(e, W2, b2, True)
    for n in range(len(NAMES) + 1):
        for want in itertools.combinations(NAMES, n):
            o = _head(e, W2, b2, True, want=want)
            for name in want:
                np.testing.assert_array_equal(_bits(o[name]), _bits(full[name]), err_msg="%s of %s" % (name, want))
    ed = _cuda(e)
    assert L.lib().dad_predict_head(ed.data_ptr(), 0, _cuda(W2).data_ptr(), _cuda(b2).data_ptr(), 1, None, None, None,
                                    None, _stream()) == L.E_SHAPE
