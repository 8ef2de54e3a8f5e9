"""A train step depends on nothing an earlier step left behind (tests/hidden_state.py holds the cases, and
tests/test_hidden_state_cpu.py the conditions they rely on).

One DADStep lives for a whole run while (B, T, Bn, Tn) changes from step to step, the warm-up flag flips and one
byte buffer is carved anew for every geometry (dad_ws_layout, csrc/dad_common.h), so a region of step k lies over
other regions' bytes of step k - 1.  "Same" below is bit for bit over everything test_gpu_store16._snapshot
collects (losses, outputs(), parameters, Adam moments, DACP state), DADStep.grad, and range_flag() == 0.

  1  a dense step from a workspace of 0xFF or of 0x01 bytes is the step from the zero-filled one, and the steps on
     the problems' own draws (fp32, and fp16 / bf16 with explicit draws) also meet every assertion of
     test_gpu_exact_operands.test_step_on_exact_operands (its _check is called): held to float64, not only to
     themselves.  The counter units cannot be: their draws are not on exact_problem's grid.  The SCL units on the
     problems' own draws go through the same check against exact_problem's reference WITH the supervised-contrastive
     term (tests/test_gpu_exact_scl.py); the SCL units on counter draws are compared bit for bit only.
  2  ten steps over G0 .. G4 at both epochs through one DADStep, the seeded state reloaded and adam_step /
     global_step pinned before each: every step is that step alone on a new DADStep.  Once as is, once with the
     whole workspace 0xFF between steps.  The buffer's size per step is hidden_state.sequence_trace's.
  3  chains with carried state whose geometry changes in mid-chain and whose next batches are named ahead (fp16,
     bf16; in-launch, PREP_CLEAN and PREP_CLEAN | PREP_NOISY deferred) equal the chain without next_batch whose
     workspace is zeroed before every step; last_prepped / last_ahead are hidden_state.CHAIN's.  A named batch of
     another geometry is refused as in test_gpu_prefetch.test_prefetch_refused_for_other_geometry.  fp32 ignores
     next_batch (one case).
  4  DADStep.grad and _buffers_for's tail / emb / logits filled with 0xFF before a step change nothing.

Words a kernel waits on.  The step has one wait: pool_wait (csrc/pool.h) in dad_tail_ecda_w[_s16|_rg]'s tail and
class blocks polls the DAD_POOL_SHARDS `ready` shards of the workspace until the tail launch's own pooling waves
have published Bc + 2 Bn items, and on a timeout (2^23 polls) sets the abort word behind them, which the reduce's
loss-total block reads (wgrad_common.h).  All nine words are stored as 0 by workgroup 0, thread 0 of the ENCODER
launch of the same step, which the stream orders before the tail launch:
  fp32         dad_encode_f32 (encode.hip), its first statement after the block-size guard
  fp16, bf16   encode_wp_body (encode_ws.hip; dad_encode_wp, dad_encode_wp_f16 and their _rg siblings are this one
               body), after its job range and before the early return of a workgroup without jobs
  warm-up      the same encoders store the zeros, and nothing waits: plan_step (step_plan.h) gives a warm-up step
               dad_tail and a separate dad_pool launch, pool_args leaves `ready` NULL when pool_grid != 0, and
               reduce_args passes no abort word.  The same holds past 64 utterances (dad_tail_ecda).
DadEncodeArgs.pool_ready is set unconditionally (dad_abi.hip encode_args), and dad_step_encode / dad_step_compute
launch the encoder in every step, prepared ahead or not.  The supervised-contrastive launches (scl.hip) and
dad_step_apply wait on nothing.  So no poison here can make a kernel wait on garbage; no kernel had to change.

Carried by the code's own documentation, hence exempt where live:
  xs16      the rows a step prepared for the batch it named (step.py _workspace: "rows the last step prepared ahead
            stay where this step looks for them"; dad_abi.hip StepWs: "the next step's is the other one").  Live
            only between a step that named a batch and the next one: parts 1, 2 and 4 name none, and part 3's
            reference zeroes the workspace where the chain under test keeps it.
  SCL       _workspace copies the old buffer only when scl_on, for the prepared rows above; the region behind the
            layout itself (scl.hip scl_ws_layout) is written by dad_scl_prep and the passes before it is read and
            carries nothing, so part 1 poisons it too.
  tail      DAD_T_RANGE is sticky ("only the caller clears them; the buffer starts zero-filled", include/dad.h):
            part 4 keeps that word.  No other word of tail, emb, logits or grad is documented as carried.
  warm-up   outputs() keeps its keys in a warm-up step, which writes only DADStep.WARMUP_OUTPUTS (its docstring);
            the extras [0, 12) of DADStep.grad (DACP thresholds and statistics) are neither written nor read then
            (optim.hip gates on !warmup).  A warm-up step is compared in what it defines.

With DAD_HIDDEN_JSON set the module writes its case count, wall time and workspace sizes there
(profiles/hidden_state.json holds them from an MI355X run)."""
import json
import os
import time

import numpy as np
import pytest
import torch

import exact_problem as X
import gpu_harness as gh
import hidden_state as H
import test_gpu_exact_operands as E
import test_gpu_store16 as S

pytestmark = pytest.mark.gpu
PKG, D, LIB = S.PKG, S.D, S.LIB
NP = LIB.DAD_NPARAM
_STATS = {"cases": 0, "sequences": {}}


@pytest.fixture(scope="module", autouse=True)
def _module_stats():
    t0 = time.time()
    yield
    _STATS["wall_s"] = round(time.time() - t0, 2)
    path = os.environ.get("DAD_HIDDEN_JSON")
    if path:
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "w") as f:
            json.dump(_STATS, f, indent=1, sort_keys=True)
    _SOLO.clear()
    _CHAIN_REF.clear()
    torch.cuda.empty_cache()


@pytest.fixture(autouse=True)
def _count():
    _STATS["cases"] += 1


# ------------------------------------------------------------------ steps, batches, snapshots
def _make(unit, st, scl=False, defer=None, gstep=0):
    prec, rng = H.ALL_UNITS[unit]
    cfg = H.cfg(scl)
    step = PKG.DADStep(PKG.SSRLModel().cuda(), PKG.ConfigView(cfg, flavor=cfg["flavor"]), precision=prec, rng=rng,
                       seed=9, prep_under_exchange=defer)
    _load(step, st, gstep)
    return step


def _load(step, st, gstep):
    """The seeded state, and the counters pinned: the bias correction and the counter RNG of a single step."""
    gh.load_state(step, st)
    step.dacp[8:16].zero_()           # (the epoch's score sums and counts: state too, which load_state leaves alone)
    step.global_step = gstep


def _store_dtype(unit, mode):
    return "f32" if mode == "store-f32" else H.ALL_UNITS[unit][0]


def _batch(inp, unit, mode, seed=0, device=False):
    """(clean, noisy, draws) of problem `inp`: padded host tensors (device: resident ones, which a step may be
    named ahead), or store batches read in place from stores of this batch's own."""
    clean, noisy, draws = gh.batches(inp)
    if mode == "padded":
        if device:
            clean = {"net_input": {k: v.cuda() for k, v in clean["net_input"].items()}, "labels": clean["labels"].cuda()}
            noisy = {"net_input": {k: v.cuda() for k, v in noisy["net_input"].items()}, "labels": noisy["labels"].cuda()}
        return clean, noisy, draws
    dt = S.DT[_store_dtype(unit, mode)]
    (fc, sc, oc, ic), (fn, sn, on, inn) = H.store_layouts(inp, seed)
    clean = D.FeatureStore(fc, sc, oc, inp["yc"], dtype=dt).batch_index(np.asarray(ic))
    noisy = D.FeatureStore(fn, sn, on, dtype=dt).batch_index(np.asarray(inn), with_labels=False)
    assert tuple(clean["net_input"]["padding_mask"].shape) == inp["mc"].shape
    assert tuple(noisy["net_input"]["padding_mask"].shape) == inp["mn"].shape
    return clean, noisy, draws


def _modes(unit):
    return ["padded", "store-f32"] + ([] if H.ALL_UNITS[unit][0] == "fp32" else ["store-16"])


def _go(step, unit, batch, epoch, next_batch=None):
    draws = batch[2] if H.ALL_UNITS[unit][1] == "explicit" else None
    return step.step(batch[0], batch[1], epoch, draws=draws, next_batch=next_batch)


def _snap(step, losses, g, epoch):
    """_snapshot, DADStep.grad and the range flag; of a warm-up step, what it defines (module docstring)."""
    Bc, Bn = g["B"], g["Bn"]
    s = S._snapshot(step, losses, Bc, Bn)
    full = step.grad.detach().cpu().numpy()
    if epoch < 30:
        stale = {k for k, v in step.outputs(Bc, Bn).items() if torch.is_tensor(v)} - set(step.WARMUP_OUTPUTS)
        s = {k: v for k, v in s.items() if k not in stale}
        full = np.concatenate([full[:NP], full[NP + 12:]])
    s["step.grad"] = full
    s["range_flag"] = np.int32(int(step.range_flag()))
    assert s["range_flag"] == 0
    return s


_SOLO = {}


def _case(gi, epoch, scl=False):
    """exact_problem's (inputs, state, reference); with `scl`, the reference with the term (H.SCL's settings)."""
    return X.case(H.geom(gi), epoch, **(H.SCL if scl else {}))


def _solo(unit, mode, gi, epoch, gstep=0, scl=False):
    """The step alone on a new DADStep from the zero-filled workspace (computed once, never changed)."""
    key = (unit, mode, gi, epoch, gstep, scl)
    if key not in _SOLO:
        inp, st, _ = _case(gi, epoch, scl)
        step = _make(unit, st, scl, gstep=gstep)
        losses = _go(step, unit, _batch(inp, unit, mode), epoch)
        _SOLO[key] = _snap(step, losses, H.geom(gi), epoch)
    return _SOLO[key]


# ------------------------------------------------------------------ 1. a poisoned workspace
def _part1():
    cases = []
    for unit, (prec, rng) in H.ALL_UNITS.items():
        geoms = [1, 3] if prec == "fp32" else [1, 3, 65]
        for mode in (_modes(unit) if unit in H.UNITS else ["padded"]):
            for gi in geoms:
                for epoch in H.EPOCHS:
                    # both patterns; one of them, alternating, in the repeats across store dtypes and draws
                    both = unit in H.UNITS and mode != "store-16"
                    for byte in (H.PATTERNS if both else [H.PATTERNS[(gi + epoch // 60 + (prec == "bf16")) % 2]]):
                        cases.append((unit, mode, gi, epoch, byte, False))
    for unit, byte in (("fp32-explicit", 0xFF), ("fp16-counter", 0x01), ("bf16-counter", 0xFF),
                       ("fp16-explicit", 0xFF), ("bf16-explicit", 0x01)):
        cases.append((unit, "padded", 3, 60, byte, True))
    return cases


def _id1(c):
    return "%s-%s-G%d-e%d-%02x%s" % (c[0], c[1], c[2], c[3], c[4], "-scl" if c[5] else "")


@pytest.mark.parametrize("case", _part1(), ids=_id1)
def test_dense_step_from_a_poisoned_workspace(case, monkeypatch):
    unit, mode, gi, epoch, byte, scl = case
    g = H.geom(gi)
    want = _solo(unit, mode, gi, epoch, scl=scl)
    if mode != "padded":
        S._no_materialize(monkeypatch)
    inp, st, ref = _case(gi, epoch, scl)
    step = _make(unit, st, scl)
    batch = _batch(inp, unit, mode)
    draws = batch[2] if H.ALL_UNITS[unit][1] == "explicit" else None
    cfg = step._prepare(batch[0], batch[1], epoch, None, draws)[0]
    assert bool(cfg.scl_on) == (scl and epoch >= 30) and not cfg.ragged
    ws = step._workspace(cfg)
    ws.fill_(byte)                                   # every byte, the SCL region behind the layout included
    losses = _go(step, unit, batch, epoch)
    assert step._ws is ws
    got = _snap(step, losses, g, epoch)
    S._assert_same([got], [want])
    if H.ALL_UNITS[unit][1] == "explicit":
        # the problem's own draws: test_step_on_exact_operands' assertions for this geometry and precision (with the
        # term: test_gpu_exact_scl's, the same function on the reference that holds the term)
        assert ("scl" in ref) == (scl and epoch >= 30)
        o = {k: (v.detach().cpu().numpy() if torch.is_tensor(v) else v) for k, v in step.outputs(g["B"], g["Bn"]).items()}
        o.update({k: float(v) for k, v in losses.items()})
        o["grads"] = gh.unflat(o["grad"])
        E._check(o, step, ref, H.ALL_UNITS[unit][0], epoch, "poisoned " + _id1(case))


# ------------------------------------------------------------------ 2. a sequence of geometries
def _seq_mode(unit):
    return "store-f32" if H.ALL_UNITS[unit][0] == "fp32" else "store-16"


@pytest.mark.parametrize("overwrite", [False, True], ids=["as_is", "ff_between"])
@pytest.mark.parametrize("store", [False, True], ids=["padded", "store"])
@pytest.mark.parametrize("unit", list(H.UNITS))
def test_sequence_of_geometries_through_one_step(unit, store, overwrite, monkeypatch):
    mode = _seq_mode(unit) if store else "padded"
    if store:
        S._no_materialize(monkeypatch)
    trace = H.sequence_trace(H.UNITS[unit][0])
    step, sizes, last_ws = None, [], None
    for k, (gi, epoch) in enumerate(H.SEQUENCE):
        g = H.geom(gi)
        want = _solo(unit, mode, gi, epoch, gstep=k)
        inp, st, _ = X.case(g, epoch)
        if step is None:
            step = _make(unit, st, gstep=k)
        else:
            _load(step, st, k)
        if overwrite and step._ws is not None:
            step._ws.fill_(0xFF)
        losses = _go(step, unit, _batch(inp, unit, mode), epoch)
        got = _snap(step, losses, g, epoch)
        # the buffer this step ran in is the one the CPU module reasons about
        assert step._ws.numel() == trace[k]["capacity"] and (step._ws is not last_ws) == trace[k]["grew"], k
        last_ws = step._ws
        sizes.append(step._ws.numel())
        for name in got:
            np.testing.assert_array_equal(got[name], want[name], err_msg="step %d (G%d, epoch %d): %s" % (k, gi, epoch, name))
        assert set(got) == set(want)
    _STATS["sequences"][H.UNITS[unit][0]] = {
        "workspace_bytes": sizes, "need": [t["need"] for t in trace],
        "inherited_steps": [k for k, t in enumerate(trace) if t["inherited"]],
        "grew_steps": [k for k, t in enumerate(trace) if t["grew"]]}


# ------------------------------------------------------------------ 3. chains, batches named ahead
def _chain_batches(unit, mode):
    return {name: _batch(H.chain_problem(name)[0], unit, mode, seed=i, device=True)
            for i, name in enumerate(sorted(H.CHAIN_BATCHES))}


def _chain_state():
    return X.state(tau_range=X.tau_range(H.chain_problem("a")[1]["Bn"]))


def _run_chain(unit, batches, script, ahead, defer=None):
    """The chain `script` (hidden_state.CHAIN's rows) with carried state.  ahead: the next batches named; else none
    is, and the workspace is zeroed before every step (part 2 ties that to new instances)."""
    step = _make(unit, _chain_state(), defer=defer if ahead else None)
    snaps, seen = [], []
    for name, epoch, named, _, _ in script:
        if not ahead and step._ws is not None:
            step._ws.zero_()
        nxt = batches[named][:2] if ahead and named is not None else None
        losses = _go(step, unit, batches[name], epoch, next_batch=nxt)
        seen.append((step.last_prepped, step.last_ahead))
        snaps.append(_snap(step, losses, H.geom(H.CHAIN_BATCHES.get(name, (1,))[0]), epoch))
    return snaps, seen, step


_CHAIN_REF = {}


@pytest.mark.parametrize("defer", [0, LIB.PREP_CLEAN, LIB.PREP_CLEAN | LIB.PREP_NOISY],
                         ids=["in_launch", "split_clean", "split_all"])
@pytest.mark.parametrize("store", [False, True], ids=["padded", "store"])
@pytest.mark.parametrize("unit", ["fp16-counter", "bf16-counter"])
def test_chain_with_batches_named_ahead(unit, store, defer, monkeypatch):
    mode = "store-16" if store else "padded"
    if store:
        S._no_materialize(monkeypatch)
    if (unit, mode) not in _CHAIN_REF:
        batches = _chain_batches(unit, mode)
        want, plain, _ = _run_chain(unit, batches, H.CHAIN, ahead=False)
        assert plain == [(False, (0, 0))] * len(H.CHAIN)
        _CHAIN_REF[(unit, mode)] = (batches, want)
    batches, want = _CHAIN_REF[(unit, mode)]
    got, seen, step = _run_chain(unit, batches, H.CHAIN, ahead=True, defer=defer or None)
    assert seen == [(prepped, (1, defer) if accepted else (0, 0)) for _, _, _, prepped, accepted in H.CHAIN], seen
    S._assert_same(got, want)
    # the batch that arrived in place of the named one shares no pointer of the preparation's key with it
    kb = step._batch_structs(batches["b"][0], batches["b"][1], 60, None, None)[1]
    kc = step._batch_structs(batches["c"][0], batches["c"][1], 60, None, None)[1]
    fields = [f for f in step._PREP_BT if getattr(kb, f)]
    assert set(fields) >= set(H.PADDED_FIELDS) and (not store or set(fields) >= {"rowc", "lenc", "rown", "lenn"})
    assert all(getattr(kb, f) != getattr(kc, f) for f in fields)


def _swap(named, other, field):
    """The named batch with ONE tensor of the preparation's key taken from `other`."""
    clean = {"net_input": dict(named[0]["net_input"]), "labels": named[0]["labels"]}
    noisy = {"net_input": dict(named[1]["net_input"]), "labels": named[1]["labels"]}
    side = clean if field in ("xc", "mc") else noisy
    src = other[0] if field in ("xc", "mc") else other[1]
    key = "feats" if field in ("xc", "xn") else "padding_mask"
    side["net_input"][key] = src["net_input"][key]
    return clean, noisy, named[2]


@pytest.mark.parametrize("defer", [0, LIB.PREP_CLEAN | LIB.PREP_NOISY], ids=["in_launch", "split_all"])
@pytest.mark.parametrize("field", H.PADDED_FIELDS)
def test_named_batch_with_one_tensor_replaced_is_not_prepared(field, defer):
    """Every pointer of DADStep._prep_key decides by itself: batch b is named, and b with one tensor of c's arrives."""
    unit = "fp16-counter"
    batches = _chain_batches(unit, "padded")
    batches["x"] = _swap(batches["b"], batches["c"], field)
    script = [("a", 60, "b", False, True), ("x", 60, None, False, False)]
    want, _, _ = _run_chain(unit, batches, script, ahead=False)
    got, seen, _ = _run_chain(unit, batches, script, ahead=True, defer=defer or None)
    assert seen == [(False, (1, defer)), (False, (0, 0))], seen
    S._assert_same(got, want)
    prepared, seen, _ = _run_chain(unit, batches, [script[0], ("b", 60, None, True, False)], ahead=True, defer=defer or None)
    assert seen[1][0] is True
    assert not np.array_equal(prepared[1]["step.grad"], got[1]["step.grad"])       # (the tensor matters to the result)


def test_fp32_ignores_next_batch():
    unit = "fp32-counter"
    batches = _chain_batches(unit, "padded")
    script = [("a", 60, "b", False, False), ("b", 60, "a", False, False), ("p", 60, None, False, False)]
    want, _, _ = _run_chain(unit, batches, script, ahead=False)
    got, seen, step = _run_chain(unit, batches, script, ahead=True, defer=LIB.PREP_CLEAN)
    assert seen == [(False, (0, 0))] * 3 and step._prepped_key is None and step._side is None
    S._assert_same(got, want)


# ------------------------------------------------------------------ 4. output buffers that are never zero again
# words of the output buffers the documentation carries from step to step (include/dad.h): the sticky range flag
TAIL_EXEMPT = (LIB.T_RANGE,)


@pytest.mark.parametrize("epoch", H.EPOCHS)
@pytest.mark.parametrize("gi", [1, 3])
@pytest.mark.parametrize("unit", list(H.UNITS))
def test_poisoned_output_buffers_change_nothing(unit, gi, epoch):
    g = H.geom(gi)
    want = _solo(unit, "padded", gi, epoch)
    inp, st, _ = X.case(g, epoch)
    step = _make(unit, st)
    bufs = step._buffers_for(g["B"], g["Bn"])
    assert sorted(bufs) == ["emb", "logits", "tail"]
    H.poison_(step.grad, 0xFF)
    H.poison_(bufs["tail"], 0xFF, exempt=TAIL_EXEMPT)
    H.poison_(bufs["emb"], 0xFF)
    H.poison_(bufs["logits"], 0xFF)
    losses = _go(step, unit, _batch(inp, unit, "padded"), epoch)
    assert step._last is bufs
    S._assert_same([_snap(step, losses, g, epoch)], [want])
