"""The fused step at long utterances and past 21 weight-gradient splits, held to tests/exact_problem.py's float64
reference exactly as tests/test_gpu_exact_operands.py holds it at the edge geometries (its _check, unchanged: losses
at 1e-4, mask equal, every err / bound <= 1, range flag 0).

The reference collator pads a batch to its longest utterance and emotion2vec frames arrive at 50 Hz, so an epoch holds
batches far beyond the T = 300 every other step test stops at.  The problems (exact_problem.LONG_GEOMS):

  L1  B2 T544 / Bn3 Tn577     17 / 19 slabs per utterance: csrc/pool.h sums the slab partials and active counts in
                              batches of 16, here one slab into the second batch; utterances that end before, on and
                              after frame 512 (the pad-byte loop past its unrolled part, one and two trips); a last slab
                              of one frame
  L2  B2 T1056 / Bn2 Tn1025   33 slabs: a third batch
  L3  B16 T1400 / Bn16 Tn1400 1408 slabs = 22 x 64: dad_wgd_min_splits binds (22 splits, 21 below), every split holds
                              WGD_MAXU = 64 slabs, boundaries inside utterances, 12 x 22 + 4 workgroups on 256 CUs,
                              dad_reduce_w over 22 partials
  S1  B32 T32 / Bn32 Tn32     with splits = 1: one split of 64 slabs AND 64 utterances (the full dL/de table of
                              dad_wgrad_direct, eight batches of eight, the fp16 row-maximum pass over all of them)
L1, L2 and L3 carry sentinel channels: a slab the weight gradient drops or counts twice lies at least 10x outside the
bound there, which the plain problems cannot show past about 100 slabs (tests/test_exact_problem_cpu.py shows both,
and that the pooling loops' possible mistakes lie 10x outside the forward bounds).

  epochs      0 runs dad_pool and dad_tail (warm-up); 60 pools on dad_tail_ecda_w's spare waves; with
              USE_CLASS_AWARE_MMD off, 60 runs dad_pool on the weak and strong items too
  store-fed   L1 read in place from f32 / fp16 / bf16 stores, dense and ragged (pool_item<.., RG>: 7 live of 17 padded
              slabs), L3 from an fp16 store, ragged (the `_rg` weight gradient at 22 splits)
  ahead       at L3's shape a three-step chain that names each next batch equals the plain chain bit for bit
              (dad_wgrad_direct_f16_cp and the tail's row preparation at 22 splits)
No case runs an fp32 step on a 16-bit store.  With DAD_EXACT_JSON=<dir>/<name>.json set, the ratios are written to
<dir>/<name>_long.json (profiles/exact_operands_long.json is that file from an MI355X run)."""
import ctypes
import gc
import json
import os

import numpy as np
import pytest
import torch

import dadpkg
import exact_problem as X
import gpu_harness as gh
import test_gpu_exact_operands as E
from test_gpu_graph import _device_batches, _state
from test_gpu_parity import EDGE

pytestmark = pytest.mark.gpu
PRECS = ["fp32", "fp16", "bf16"]
L1, L2, L3, S1 = (X.LONG[k] for k in ("L1", "L2", "L3", "S1"))
_MINE = []          # the keys of E._MEASURED this module wrote


@pytest.fixture(scope="module", autouse=True)
def _dump_and_free():
    yield
    path = os.environ.get("DAD_EXACT_JSON")
    if path and _MINE:
        root, ext = os.path.splitext(os.path.abspath(path))
        os.makedirs(os.path.dirname(root), exist_ok=True)
        with open(root + "_long" + ext, "w") as f:
            json.dump({k: E._MEASURED[k] for k in _MINE}, f, indent=1, sort_keys=True)
    for key in [k for k in X._CASES if k[0] in X.LONG or k[0] == X.S1_PLUS["id"]]:
        del X._CASES[key]           # (L3's reference holds 0.5 GB on the host)
    gc.collect()
    torch.cuda.empty_cache()


def _check(o, step, ref, prec, epoch, what):
    _MINE.append(what)
    E._check(o, step, ref, prec, epoch, what)


def _step(prec, st, splits=0, **cfg_over):
    step = gh.make_step(dict(X.cfg(), **cfg_over), precision=prec, splits=splits)
    gh.load_state(step, st)
    return step


def _plan(step, inp, epoch):
    """(plan info of the step dad_step_plan reports, the device's CU count)"""
    lib = dadpkg.pkg()._lib
    (Bc, Tc), (Bn, Tn) = inp["mc"].shape, inp["mn"].shape
    info = lib.DadStepPlanInfo()
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    assert lib.lib().dad_step_plan(step.make_config(Bc, Tc, Bn, Tn, epoch), None, None, 0, cus, ctypes.byref(info)) == 0
    return info, cus


@pytest.mark.parametrize("epoch", [0, 60])
@pytest.mark.parametrize("geom", [L1, L2], ids=X.geom_id)
@pytest.mark.parametrize("prec", PRECS)
def test_step_past_one_pool_batch(prec, geom, epoch):
    inp, st, ref = X.case(geom, epoch)
    step = _step(prec, st)
    o = gh.run_step(step, inp, epoch)
    _check(o, step, ref, prec, epoch, "%s %s e%d" % (prec, X.geom_id(geom), epoch))


@pytest.mark.parametrize("prec", ["fp32", "fp16"])
def test_separate_pool_launch_past_one_pool_batch(prec):
    """Without class-aware MMD the step pools every item, the weak and strong ones too, in dad_pool."""
    inp, st, ref = X.case(L1, 60, USE_CLASS_AWARE_MMD=False)
    step = _step(prec, st, USE_CLASS_AWARE_MMD=False)
    info, _ = _plan(step, inp, 60)
    assert info.pool_grid == inp["xc"].shape[0] + 2 * inp["xn"].shape[0] and info.tail == b"dad_tail_ecda", (info.pool_grid, info.tail)
    o = gh.run_step(step, inp, 60)
    _check(o, step, ref, prec, 60, "%s L1 e60 dad_pool" % prec)


@pytest.mark.parametrize("prec", PRECS)
def test_step_past_21_splits(prec):
    inp, st, ref = X.case(L3, 60)
    step = _step(prec, st)
    info, cus = _plan(step, inp, 60)
    if prec == "fp32":
        assert info.splits == 42, info.splits
    else:
        assert info.splits == 22 and info.wgrad_grid > cus, (info.splits, info.wgrad_grid, cus)
    o = gh.run_step(step, inp, 60)
    _check(o, step, ref, prec, 60, "%s L3 e60" % prec)


@pytest.mark.parametrize("geom,want", [(S1, 1), (X.S1_PLUS, 2)], ids=["S1", "S1plus"])
@pytest.mark.parametrize("prec", ["fp16", "bf16"])
def test_one_split_of_64_slabs_and_utterances(prec, geom, want):
    """splits = 1 holds for 64 slabs (one utterance each); the 65th raises it to 2, as the plan reports."""
    inp, st, ref = X.case(geom, 60)
    step = _step(prec, st, splits=1)
    used = _plan(step, inp, 60)[0].splits
    assert used == want, used
    o = gh.run_step(step, inp, 60)
    _check(o, step, ref, prec, 60, "%s %s splits 1" % (prec, X.geom_id(geom)))


@pytest.mark.parametrize("prec", ["fp32", "fp16"])
def test_trailing_empty_splits_contribute_nothing(prec):
    """64 slabs over 24 splits: 3 slabs each, so splits 22 and 23 start past the list's end.  The step meets the bounds,
    and equals the step with 22 splits (the same 22 ranges, summed in the same order) bit for bit: an empty split's
    partial is exact zeros."""
    inp, st, ref = X.case(EDGE[2], 60)
    assert sum(a.shape[0] * ((a.shape[1] + 31) // 32) for a in (inp["mc"], inp["mn"])) == 64
    grads = {}
    for splits in (22, 24):
        step = _step(prec, st, splits=splits)
        assert _plan(step, inp, 60)[0].splits == splits
        o = gh.run_step(step, inp, 60)
        grads[splits] = o["grad"].copy()
        if splits == 24:
            _check(o, step, ref, prec, 60, "%s %s splits 24" % (prec, X.geom_id(EDGE[2])))
    np.testing.assert_array_equal(grads[24], grads[22])


def _store_fed(geom, prec, store_dtype, ragged, monkeypatch):
    inp, st, ref = X.case(geom, 60)

    def refuse(self):
        raise AssertionError("StoreFeats.materialize(): the step made a padded copy of a store batch")
    monkeypatch.setattr(dadpkg.pkg().data.StoreFeats, "materialize", refuse)
    step = _step(prec, st)
    step.ragged = ragged
    clean = E._store(inp["xc"], inp["mc"], inp["yc"], store_dtype)
    noisy = E._store(inp["xn"], inp["mn"], None, store_dtype)
    assert clean["net_input"]["padding_mask"].shape == inp["mc"].shape
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
    _check(o, step, ref, prec, 60, "%s %s store %s %s" % (prec, X.geom_id(geom), str(store_dtype).split(".")[-1],
                                                         "ragged" if ragged else "dense"))


@pytest.mark.parametrize("ragged", [False, True], ids=["dense", "ragged"])
@pytest.mark.parametrize("store_dtype", [torch.float32, torch.float16, torch.bfloat16], ids=["f32", "fp16", "bf16"])
@pytest.mark.parametrize("prec", ["fp16", "bf16"])
def test_store_fed_step_past_one_pool_batch(prec, store_dtype, ragged, monkeypatch):
    _store_fed(L1, prec, store_dtype, ragged, monkeypatch)


def test_store_fed_ragged_step_past_21_splits(monkeypatch):
    _store_fed(L3, "fp16", torch.float16, True, monkeypatch)


def test_prepared_ahead_chain_past_21_splits():
    """tests/test_gpu_prefetch.py's chain at L3's shape (counter RNG, fp16, no reference): every step but the first takes
    the rows the previous step's launches prepared, and the chain equals the plain one bit for bit."""
    inp = X.case(L3, 60)[0]
    small = {k: inp[k][:1] for k in ("nw", "ns")}       # (the draws are not used: counter RNG)
    batches = []
    for order in (np.arange(16), np.arange(16)[::-1].copy(), np.roll(np.arange(16), 5)):      # three batches of the shape
        v = dict(inp, **small, **{k: np.ascontiguousarray(inp[k][order]) for k in ("xc", "mc", "yc", "xn", "mn", "yn")})
        batches.append(_device_batches(v)[:2])
    st = X.state()
    runs = []
    for ahead in (False, True):
        step = gh.make_step(X.cfg(), precision="fp16", rng="counter", seed=5)
        gh.load_state(step, st)
        losses, prepped = [], []
        for k in range(3):
            c, n = batches[k]
            out = step.step(c, n, 60, next_batch=batches[(k + 1) % 3] if ahead else None)
            losses.append({key: float(v) for key, v in out.items()})
            prepped.append(step.last_prepped)
        torch.cuda.synchronize()
        assert int(step.range_flag()) == 0
        runs.append((_state(step), losses, prepped))
    (want, want_losses, plain_prepped), (got, got_losses, prepped) = runs
    assert plain_prepped == [False, False, False] and prepped == [False, True, True], (plain_prepped, prepped)
    for name, a, b in zip(("student", "teacher", "exp_avg", "exp_avg_sq", "dacp", "grad"), got, want):
        assert torch.equal(a, b), "%s differs (max %.3g)" % (name, float((a - b).abs().max()))
    assert got_losses == want_losses
    assert all(np.isfinite(v) for d in want_losses for v in d.values())
