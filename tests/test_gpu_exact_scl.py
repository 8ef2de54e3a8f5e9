"""The fused step WITH the supervised-contrastive term (csrc/scl.hip, TARGET_SCL_WEIGHT > 0), in all three precisions,
held to tests/exact_problem.py's float64 reference with the term the way tests/test_gpu_exact_operands.py holds the
step without it (its _check: losses at 1e-4, scl_loss and the total including it, mask equal, every err / bound <= 1,
range flag 0).

The term reaches the weight gradient by the most delicate route of the step: dad_scl_final writes
ge_ecda[u] = (eflag[u] ? ge_ecda[u] : 0) + w_scl g_u and sets the flag, and every weight-gradient variant
(wgrad_f32.hip, wgrad_direct.h in fp16 with its per-hidden-unit power-of-two scale and in bf16, the _rg and _cp
siblings, reduce.hip for db1) adds the flagged rows through fused_ge1_v.  tests/test_gpu_scl.py holds that route to
1e-4 of the gradient norm in fp32 and to a direction cosine in fp16; here every element of dW1 and db1 is held to
    |g - g_ref| <= (eps_op + n_rows 2^-24 + 1e-4) S_g + tail term + the term's allowance
where S_g adds |base| and w_scl |term| without cancellation and the allowance is 1e-4 of max |g_scl| (dad_scl's own
bound) plus 4x the term's measured sensitivity to the embeddings' fp32 error, per element of a member row
(exact_problem's docstring, "contrastive term").  tests/test_exact_problem_cpu.py shows that a float32 restatement
sits inside the bounds of all three precisions, that the term carries at least 3 % of S_W1 wherever there is an
anchor, and that the term dropped, overwriting the ECDA part, with the wrong members, labels, embeddings,
normalisation backward, temperature, mean or input lies at least 10x outside the bf16 bound.

Settings unless stated: TARGET_SCL_WEIGHT = 1 (2 at B64T40/Bn64Tn40: exact_problem.SCL_WEIGHT), SCL_START_EPOCH = 0,
SCL_TEMPERATURE = 0.1, epoch 60.  The noisy batch's labels handed to the step differ from the pseudo-label in every
masked-in row (exact_problem.case): no step may read them.

  matrix      {fp32, fp16, bf16} x the five edge geometries x {ECDA on, USE_ECDA=False: the term alone flags rows}.
              B1T1/Bn2Tn3 has three members of three classes and no anchor: scl_loss == 0 exactly and the bounds are
              the weight-0 step's
  weight 8    B16T64/Bn16Tn64, ECDA on: the term and ECDA are of one size in the flagged rows (the fp16 weight
              gradient's per-unit scale on their sum; test_exact_problem_cpu.py measures the two sizes)
  split-K     splits auto, 3 and 5 on B5T33/Bn7Tn31 and B12T45/Bn20Tn70, fp32 and fp16
  store-fed   B5T33/Bn7Tn31 read in place from f32 / fp16 / bf16 stores, dense and ragged, fp16 and bf16
  past 64     B65T33/Bn66Tn31 (exact_problem.PAST64): the general tail (dad_tail_ecda), and 131 candidate rows for
              dad_scl: a third row tile and a second column chunk.  dad_scl run on the step's own embeddings reports
              the reference's member and anchor counts
  long        L1: embeddings summed past one pool batch feed the term
Every case prints its ratios and the term's share of S_W1 before asserting; with DAD_EXACT_SCL_JSON set the ratios are
also written there (profiles/exact_scl.json is that file from an MI355X run)."""
import json
import os

import numpy as np
import pytest
import torch

import dadpkg
import exact_problem as X
import gpu_harness as gh
import test_gpu_exact_operands as E
import test_gpu_long_utterances as LU
from test_gpu_parity import EDGE

pytestmark = pytest.mark.gpu
PRECS = ["fp32", "fp16", "bf16"]
EPOCH = 60
_MINE = []          # the keys of E._MEASURED this module wrote


@pytest.fixture(scope="module", autouse=True)
def _dump_measured():
    yield
    path = os.environ.get("DAD_EXACT_SCL_JSON")
    if path and _MINE:
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "w") as f:
            json.dump({k: E._MEASURED[k] for k in _MINE}, f, indent=1, sort_keys=True)


def _step(prec, st, over, splits=0):
    step = gh.make_step(dict(X.cfg(), **over), precision=prec, splits=splits)
    gh.load_state(step, st)
    return step


def _check(o, step, ref, prec, what):
    s = ref["scl"]
    print("%s: weight %g, members %d, anchors %s, the term's share of S_W1 %.4f" % (
        what, s["w"], s["members"], [int(a) for a in s["anchors"]], s["share"]))
    _MINE.append(what)
    E._check(o, step, ref, prec, EPOCH, what)
    E._MEASURED[what]["scl_share"] = float("%.4g" % s["share"])
    assert "scl_loss" in o and int(step.range_flag()) == 0, what


def _run(prec, geom, over, what, splits=0):
    inp, st, ref = X.case(geom, EPOCH, **over)
    step = _step(prec, st, over, splits)
    o = gh.run_step(step, inp, EPOCH)
    _check(o, step, ref, prec, what)
    return inp, ref, o, step


@pytest.mark.parametrize("ecda", [True, False], ids=["ecda", "noecda"])
@pytest.mark.parametrize("geom", EDGE, ids=X.geom_id)
@pytest.mark.parametrize("prec", PRECS)
def test_step_with_the_term_on_exact_operands(prec, geom, ecda):
    over = X.scl_over(geom, ecda)
    _, ref, o, _ = _run(prec, geom, over, "%s %s scl%s" % (prec, X.geom_id(geom), "" if ecda else " noecda"))
    if geom["B"] == 1:
        # no anchor: the loss is exactly 0 and the bounds are those of the step without the term
        off = X.case(geom, EPOCH, **({} if ecda else {"USE_ECDA": False}))[2]
        assert ref["scl"]["V"] == 0 and o["scl_loss"] == 0.0
        for n in X.GRAD_NAMES:
            np.testing.assert_array_equal(X.grad_limit(n, prec, ref), X.grad_limit(n, prec, off))
    else:
        assert ref["scl"]["V"] > 0 and o["scl_loss"] > 0.0
        assert (ref["oracle"]["ecda_loss"] != 0.0) == (ecda and geom["B"] >= 12)


@pytest.mark.parametrize("prec", PRECS)
def test_term_and_ecda_of_one_size_in_the_flagged_rows(prec):
    geom = EDGE[2]
    over = X.scl_over(geom, weight=8.0)
    _run(prec, geom, over, "%s %s scl weight 8" % (prec, X.geom_id(geom)))


@pytest.mark.parametrize("splits", [0, 3, 5], ids=["auto", "3", "5"])
@pytest.mark.parametrize("geom", [EDGE[1], EDGE[3]], ids=X.geom_id)
@pytest.mark.parametrize("prec", ["fp32", "fp16"])
def test_split_k_with_the_term(prec, geom, splits):
    what = "%s %s scl splits %s" % (prec, X.geom_id(geom), splits or "auto")
    inp, _, _, step = _run(prec, geom, X.scl_over(geom), what, splits=splits)
    used = E._splits_used(step, inp, EPOCH)
    print("%s: the plan uses %d splits" % (what, used))
    E._MEASURED[what]["splits_used"] = used


@pytest.mark.parametrize("ragged", [False, True], ids=["dense", "ragged"])
@pytest.mark.parametrize("store_dtype", [torch.float32, torch.float16, torch.bfloat16], ids=["f32", "fp16", "bf16"])
@pytest.mark.parametrize("prec", ["fp16", "bf16"])
def test_store_fed_step_with_the_term(prec, store_dtype, ragged, monkeypatch):
    geom = EDGE[1]
    over = X.scl_over(geom)
    inp, st, ref = X.case(geom, EPOCH, **over)

    def refuse(self):
        raise AssertionError("StoreFeats.materialize(): the step made a padded copy of a store batch")
    monkeypatch.setattr(dadpkg.pkg().data.StoreFeats, "materialize", refuse)
    step = _step(prec, st, over)
    step.ragged = ragged
    clean = E._store(inp["xc"], inp["mc"], inp["yc"], store_dtype)
    noisy = E._store(inp["xn"], inp["mn"], None, store_dtype)
    assert clean["net_input"]["padding_mask"].shape == inp["mc"].shape
    assert noisy["net_input"]["padding_mask"].shape == inp["mn"].shape
    draws = gh.batches(inp)[2]
    cfg = step._batch_structs(clean, noisy, EPOCH, None, draws)[0]
    assert cfg.ragged == int(ragged) and cfg.scl_on == 1
    losses = step.step(clean, noisy, EPOCH, draws=draws)
    torch.cuda.synchronize()
    Bc, Bn = inp["xc"].shape[0], inp["xn"].shape[0]
    o = {k: (v.detach().cpu().numpy() if torch.is_tensor(v) else v) for k, v in step.outputs(Bc, Bn).items()}
    o.update({k: float(v) for k, v in losses.items()})
    o["grads"] = gh.unflat(o["grad"])
    _check(o, step, ref, prec, "%s %s scl store %s %s" % (prec, X.geom_id(geom), str(store_dtype).split(".")[-1],
                                                         "ragged" if ragged else "dense"))


def _dad_scl_stats(o, inp, tau):
    """dad_scl's result block on the step's own embeddings, pseudo-labels and mask."""
    lib = dadpkg.pkg()._lib
    L = dadpkg.pkg().lib()
    emb = torch.from_numpy(np.ascontiguousarray(np.concatenate([o["e_clean"], o["e_strong"]], 0), np.float32)).cuda()
    lab = torch.from_numpy(np.concatenate([inp["yc"], o["pred"].astype(np.int64)])).cuda()
    mem = torch.from_numpy(np.concatenate([np.ones(len(inp["yc"]), np.uint8), (o["mask"] != 0).astype(np.uint8)])).cuda()
    n = emb.shape[0]
    out = torch.full((lib.SCL_SLOTS,), -7.0, device="cuda")
    ws = torch.empty(int(L.dad_scl_workspace_bytes(n)), dtype=torch.uint8, device="cuda")
    lib.check(L.dad_scl(emb.data_ptr(), lab.data_ptr(), mem.data_ptr(), n, tau, out.data_ptr(), None, ws.data_ptr(),
                        torch.cuda.current_stream().cuda_stream), "dad_scl")
    torch.cuda.synchronize()
    return out.cpu().numpy()


@pytest.mark.parametrize("prec", PRECS)
def test_step_with_the_term_past_64_utterances(prec):
    geom = X.PAST64
    over = X.scl_over(geom)
    inp, st, ref = X.case(geom, EPOCH, **over)
    step = _step(prec, st, over)
    info, _ = LU._plan(step, inp, EPOCH)
    assert info.tail == b"dad_tail_ecda", info.tail
    o = gh.run_step(step, inp, EPOCH)
    lib = dadpkg.pkg()._lib
    out = _dad_scl_stats(o, inp, over["SCL_TEMPERATURE"])
    s = ref["scl"]
    print("%s past 64: dad_scl reports V %d, members %d, anchors %s, loss %.7g (the step's %.7g)" % (
        prec, out[lib.SCL_V], out[lib.SCL_MEMBERS], list(out[lib.SCL_ANCHORS:lib.SCL_ANCHORS + 4]), out[lib.SCL_LOSS], o["scl_loss"]))
    _check(o, step, ref, prec, "%s %s scl" % (prec, X.geom_id(geom)))
    assert len(s["member"]) > 128 and s["members"] > 64
    assert out[lib.SCL_V] == s["V"] and out[lib.SCL_MEMBERS] == s["members"] and out[lib.SCL_NONFINITE] == 0
    assert list(out[lib.SCL_ANCHORS:lib.SCL_ANCHORS + 4]) == list(s["anchors"])


@pytest.mark.parametrize("prec", PRECS)
def test_step_with_the_term_past_one_pool_batch(prec):
    geom = X.LONG["L1"]
    ref = _run(prec, geom, X.scl_over(geom), "%s L1 scl" % prec)[1]
    assert ref["scl"]["V"] > 0
