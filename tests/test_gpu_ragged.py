"""Ragged mode of the FP16 / BF16 store-fed step (dad_config.ragged, DADStep(ragged=True)): no launch reads,
computes or writes anything for a 32-frame slab that lies wholly past its utterance's end.

What makes the checks exact: a row's encoder output depends on that row only and pooling adds the live
slabs' partials in slab order (the dead slabs' partials of the dense step are exact zeros), so the forward
pass -- embeddings, logits, losses, the tail's per-sample arrays, the DACP state -- is bit-identical to the
dense step's on the same batch.  The weight gradient's splits share the live slabs, so the fp32 split
partials are summed in another order: gradient and parameters are held to gpu_harness.close_grad's own
bounds (1e-4 norm-relative, 1e-3 elementwise, the project's numbers for the comparison with the oracle).
When every slab is live the live list is the dense list and the whole step is bit-identical.

Shapes (each store holds two batches' utterances at odd rows with unrelated rows between, test_gpu_store16's
layout):
  R  clean [1, 32, 33, 64, 65, 96, 97, 129], noisy [129, 1, 64, 33, 97]: T = 129, 5 slabs per utterance, 21 of
     40 clean slabs live, the shortest utterance first; second group: the reverse order
  A  test_gpu_store16's shape A: two slabs per utterance, the second often dead
  F  clean in [65, 96] with one at 96, noisy in [33, 64] with one at 64: every slab live
  B  65 utterances per side with R's lengths repeated: the general tail, dad_pool, rows through dad_src_row
  Z  R with a clean utterance of 0 frames between live ones and a noisy index outside the store (length 0)"""
import ctypes

import numpy as np
import pytest
import torch

import gpu_harness as gh
import test_gpu_store16 as S

pytestmark = pytest.mark.gpu
LIB = S.LIB
D = S.D
LENS_R = ([1, 32, 33, 64, 65, 96, 97, 129], [129, 1, 64, 33, 97])
# what the gradient reaches: compared with close_grad unless every slab is live
GRAD_SIDE = ("grad", "clip_norm", "clip_coef", "student", "teacher", "exp_avg", "exp_avg_sq")
WORST = {}      # the largest figures seen, printed by each test that compares gradients


def _problem(shape):
    if shape == "A":
        return S._problem("A")
    key = "ragged-" + shape
    if key not in S._PROBLEMS:
        rs = np.random.RandomState({"R": 501, "F": 502, "B": 503, "Z": 504}[shape])
        if shape in ("R", "Z"):
            lc, ln = LENS_R
            gc, gn = [list(lc), lc[::-1]], [list(ln), ln[::-1]]
            if shape == "Z":
                gc[0][3] = gc[1][4] = 0        # no frames, between live utterances
        elif shape == "F":
            gc = [[96] + list(rs.randint(65, 97, size=4)), list(rs.randint(65, 97, size=4)) + [96]]
            gn = [[64] + list(rs.randint(33, 65, size=2)), list(rs.randint(33, 65, size=2)) + [64]]
        else:
            rep = lambda v: [v[i % len(v)] for i in range(65)]
            gc, gn = [rep(LENS_R[0]), rep(LENS_R[0])[::-1]], [rep(LENS_R[1]), rep(LENS_R[1])[::-1]]
        S._PROBLEMS[key] = (S._layout(rs, gc), S._layout(rs, gn), rs.randint(0, 4, size=2 * len(gc[0])))
    return S._PROBLEMS[key]


def _stores(shape, clean_dtype, noisy_dtype):
    (fc, sc, oc, ic), (fn, sn, on, inn), labels = _problem(shape)
    return (D.FeatureStore(fc, sc, oc, labels, dtype=S.DT[clean_dtype]), ic,
            D.FeatureStore(fn, sn, on, dtype=S.DT[noisy_dtype]), inn)


def _batches(shape, stores, k, padded=False):
    cs, ic, ns, inn = stores
    Tc = 129 if shape == "Z" else None             # (Z's longest clean utterance is not in every group)
    if shape == "Z":
        # the noisy batch's second utterance is an index outside the store: length 0, all padding
        idx = np.array(inn[k % 2])
        idx_d = torch.from_numpy(idx).cuda()
        idx_d[1] = len(ns)
        clean = cs.batch_index(ic[k % 2], T=Tc)
        noisy = ns.batch_index(idx, index_d=idx_d, T=129, with_labels=False)
    else:
        clean, noisy = cs.batch_index(ic[k % 2]), ns.batch_index(inn[k % 2], with_labels=False)
    if padded:
        for b in (clean, noisy):
            b["net_input"]["feats"] = b["net_input"]["feats"].materialize()
    return clean, noisy


def _run(shape, stores, precision, steps, ragged, ahead=False, defer=None, epoch=S.EPOCH, padded=False, poison=False):
    """`steps` steps over the stores' batches; (snapshot after each, last_ahead after each, the step)."""
    step = S._make_step(precision, "counter", defer)
    step.ragged = ragged
    batches = [_batches(shape, stores, k, padded) for k in range(steps)]
    noisy = lambda k: None if epoch < 30 else batches[k][1]
    Bc = batches[0][0]["net_input"]["padding_mask"].shape[0]
    Bn = 0 if epoch < 30 else batches[0][1]["net_input"]["padding_mask"].shape[0]
    if poison:
        cfg = step._prepare(batches[0][0], noisy(0), epoch, None, None)[0]
        assert cfg.ragged == (1 if ragged and not padded else 0)
        step._workspace(cfg).fill_(0xFF)           # NaN patterns in every format, in every byte of the workspace
    snaps, reported = [], []
    for k in range(steps):
        nxt = (batches[k + 1][0], noisy(k + 1)) if ahead and k + 1 < steps else None
        losses = step.step(batches[k][0], noisy(k), epoch, next_batch=nxt)
        reported.append(step.last_ahead)
        snaps.append(S._snapshot(step, losses, Bc, Bn))     # (asserts finite losses)
    assert int(step.range_flag()) == 0
    return snaps, reported, step


_DENSE = {}


def _dense(shape, dtypes, precision, steps, ahead=False, epoch=S.EPOCH):
    """The dense chain (computed once per case, never changed)."""
    key = (shape, dtypes, precision, steps, ahead, epoch)
    if key not in _DENSE:
        _DENSE[key] = _run(shape, _stores(shape, *dtypes), precision, steps, False, ahead=ahead, epoch=epoch)[:2]
    return _DENSE[key]


def _forward_identical(got, want, what):
    assert set(got) == set(want)
    for name in sorted(set(got) - set(GRAD_SIDE)):
        np.testing.assert_array_equal(got[name], want[name], err_msg="%s: %s" % (what, name))


def _grad_close(got, want, what):
    for name in ("grad", "student"):
        a, b = got[name].astype(np.float64).ravel(), want[name].astype(np.float64).ravel()
        rn = float(np.linalg.norm(a - b) / max(1e-12, float(np.linalg.norm(b))))
        re = float(np.abs(a - b).max() / max(1e-6, float(np.abs(b).max())))
        WORST[name] = max(WORST.get(name, (0.0, 0.0)), (rn, re))
        print("%s: %s norm-rel %.3e elementwise %.3e" % (what, name, rn, re))
    for name in ("grad", "student"):
        gh.close_grad(got[name], want[name], "%s: %s" % (what, name))


def _standard(got, want, what):
    """Test 1's standard: the forward bit for bit, gradient and post-step parameters by close_grad."""
    _forward_identical(got, want, what)
    _grad_close(got, want, what)


# ------------------------------------------------------------------ 1. forward identity
@pytest.mark.parametrize("precision,store_dtype", [("fp16", "f32"), ("fp16", "fp16"), ("bf16", "f32"), ("bf16", "bf16")])
@pytest.mark.parametrize("shape", ["R", "A"])
def test_forward_identical_and_gradient_close(shape, precision, store_dtype, monkeypatch):
    S._no_materialize(monkeypatch)
    dt = (store_dtype, store_dtype)
    want = _dense(shape, dt, precision, 1)[0]
    got = _run(shape, _stores(shape, *dt), precision, 1, True)[0]
    _standard(got[0], want[0], "%s %s store %s" % (shape, precision, store_dtype))


# ------------------------------------------------------------------ 2. all-live identity
def test_all_live_chain_is_bit_identical(monkeypatch):
    S._no_materialize(monkeypatch)
    want, want_reported = _dense("F", ("f32", "f32"), "fp16", 3, ahead=True)
    got, reported, _ = _run("F", _stores("F", "f32", "f32"), "fp16", 3, True, ahead=True)
    assert reported == want_reported == [(1, 0), (1, 0), (0, 0)]
    S._assert_same(got, want)


# ------------------------------------------------------------------ 3. chain with preparation ahead
@pytest.mark.parametrize("defer", [0, LIB.PREP_CLEAN | LIB.PREP_NOISY], ids=["in_launch", "deferred"])
@pytest.mark.parametrize("precision", ["fp16", "bf16"])
def test_chain_prepared_ahead(precision, defer, monkeypatch):
    """Three steps that name their next batch: prepared in the tail and weight-gradient launches, or left to
    dad_step_prepare_rows (prep_under_exchange).  The prepared set must not depend on who prepared it."""
    S._no_materialize(monkeypatch)
    stores = _stores("R", "f32", "f32")
    plain, plain_reported, _ = _run("R", stores, precision, 3, True)
    assert plain_reported == [(0, 0)] * 3
    got, reported, _ = _run("R", stores, precision, 3, True, ahead=True, defer=defer or None)
    assert reported == [(1, defer), (1, defer), (0, 0)], reported
    S._assert_same(got, plain)
    dense = _dense("R", ("f32", "f32"), precision, 3)[0]
    _standard(got[0], dense[0], "chain %s step 0" % precision)
    for k in (1, 2):
        for name in ("z_clean", "z_teacher", "z_strong"):
            r = gh.rel(got[k][name], dense[k][name])
            print("chain %s step %d: %s rel %.3e" % (precision, k, name, r))
            assert r <= 1e-4, (k, name, r)


# ------------------------------------------------------------------ 4. nothing dead is read
@pytest.mark.parametrize("steps,ahead", [(1, False), (3, True)], ids=["single", "chain_ahead"])
def test_poisoned_workspace_changes_nothing(steps, ahead, monkeypatch):
    """Every byte of the workspace 0xFF before the first step (the dead slabs' partials, ReLU' masks and
    prepared rows are never written in ragged mode): bit-identical to the zero-filled workspace, finite
    losses, range flag 0 (_run asserts both)."""
    S._no_materialize(monkeypatch)
    stores = _stores("R", "f32", "f32")
    want, want_reported, _ = _run("R", stores, "fp16", steps, True, ahead=ahead)
    got, reported, step = _run("R", stores, "fp16", steps, True, ahead=ahead, poison=True)
    assert reported == want_reported
    S._assert_same(got, want)
    if steps == 1:
        # ... and nothing dead is written: the workspace starts with part_sum, f32 [clean | weak | strong
        # slabs][256] in dense slab order (dad_common.h DadWs); a dead slab's row still holds the poison,
        # a live slab's row does not
        ws = step._ws.cpu().numpy()
        lc, ln = LENS_R
        slab = 0
        for lens in (lc, ln, ln):
            for n in lens:
                for c in range(5):
                    row = ws[slab * 1024:(slab + 1) * 1024]
                    assert (row == 0xFF).all() == (c >= -(-n // 32)), (slab, n, c)
                    slab += 1


# ------------------------------------------------------------------ 5. lengths are read on the device
def _state(step):
    return [t.detach().clone() for t in (step.model.student_flat, step.model.teacher_flat, step.exp_avg,
                                         step.exp_avg_sq, step.dacp, step.grad)]


def _copy_batch(dst, src):
    for d, s in zip(dst, src):
        fd, fs = d["net_input"]["feats"], s["net_input"]["feats"]
        fd.rows.copy_(fs.rows)
        fd.lens.copy_(fs.lens)
        d["net_input"]["padding_mask"].copy_(s["net_input"]["padding_mask"])
        if d.get("labels") is not None:
            d["labels"].copy_(s["labels"])


def test_captured_ragged_step_follows_the_lengths_in_its_buffers(monkeypatch):
    """One captured ragged step; between replays the other group's rows / lens / mask / labels are copied
    into the same device buffers.  Each replay equals the eager ragged step on that group (test_gpu_graph's
    pattern: a captured step bakes its host scalars, so the eager side pins them too)."""
    S._no_materialize(monkeypatch)
    stores = _stores("R", "f32", "f32")
    groups = [_batches("R", stores, k) for k in (0, 1)]
    order = [0, 1, 1, 0]

    eager = S._make_step("fp16", "counter")
    eager.ragged = True
    n0, g0 = eager.adam_step, eager.global_step
    want = []
    for k in order:
        eager.adam_step, eager.global_step = n0, g0
        eager.step(groups[k][0], groups[k][1], S.EPOCH)
        torch.cuda.synchronize()
        want.append(_state(eager))

    cap = S._make_step("fp16", "counter")
    cap.ragged = True
    start = _state(cap)
    buf = _batches("R", stores, 0)                 # the captured step's device buffers
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        cap.step(buf[0], buf[1], S.EPOCH)          # (lazy buffers first, then back to the start state)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    with torch.no_grad():
        for t, s in zip((cap.model.student_flat, cap.model.teacher_flat, cap.exp_avg, cap.exp_avg_sq, cap.dacp), start):
            t.copy_(s)
    cap.refresh_shadow()
    cap.adam_step, cap.global_step = n0, g0
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        cap.step(buf[0], buf[1], S.EPOCH)
    for i, k in enumerate(order):
        _copy_batch(buf, groups[k])
        g.replay()
        torch.cuda.synchronize()
        for name, a, b in zip(("student", "teacher", "exp_avg", "exp_avg_sq", "dacp", "grad"), _state(cap), want[i]):
            assert torch.equal(a, b), "replay %d (group %d): %s differs" % (i, k, name)
    assert int(cap.range_flag()) == 0


# ------------------------------------------------------------------ 6. other tails
def test_general_tail_past_64_utterances(monkeypatch):
    S._no_materialize(monkeypatch)
    want = _dense("B", ("f32", "f32"), "fp16", 1)[0]
    got = _run("B", _stores("B", "f32", "f32"), "fp16", 1, True)[0]
    _standard(got[0], want[0], "B fp16")


def test_warmup_epoch_without_a_noisy_batch(monkeypatch):
    S._no_materialize(monkeypatch)
    want = _dense("R", ("f32", "f32"), "fp16", 1, epoch=0)[0]
    got = _run("R", _stores("R", "f32", "f32"), "fp16", 1, True, epoch=0)[0]
    _standard(got[0], want[0], "R warm-up")


def test_utterances_without_frames(monkeypatch):
    """A clean utterance of 0 frames between live ones and a noisy index outside the store (length 0, all
    padding): no live slab, no slot of the weight gradient's per-split table."""
    S._no_materialize(monkeypatch)
    want = _dense("Z", ("f32", "f32"), "fp16", 1)[0]
    got = _run("Z", _stores("Z", "f32", "f32"), "fp16", 1, True)[0]
    _standard(got[0], want[0], "Z step 0")


# ------------------------------------------------------------------ 7. refusals
def test_c_abi_refusals():
    L = LIB.lib()
    step, cfg, bt, st, ws, keep = S._abi_case("fp16", padded=True)      # ragged needs store batches
    cfg.ragged = 1
    before = S._device_state(step)
    ncfg = LIB.DadConfig.from_buffer_copy(cfg)
    ncfg.counter = cfg.counter + 1
    for name, call in S._entry_points(L, cfg, bt, st, ws, step._stream(), None, None).items():
        assert call() == LIB.E_ARG, name
    step2, cfg2, bt2, st2, ws2, keep2 = S._abi_case("fp16", padded=False)
    cfg2.ragged = 1
    half = LIB.DadBatch.from_buffer_copy(bt2)
    half.rown, half.lenn = None, None                                   # a padded noisy side
    half.xn = bt.xn
    assert L.dad_step_encode(cfg2, half, st2, ws2, step2._stream()) == LIB.E_ARG
    for a, b in zip(S._device_state(step), before):
        assert torch.equal(a, b)
    step3, cfg3, bt3, st3, ws3, keep3 = S._abi_case("fp32", padded=False)
    cfg3.ragged = 1
    for name, call in S._entry_points(L, cfg3, bt3, st3, ws3, step3._stream(), None, None).items():
        assert call() == LIB.E_UNSUPPORTED, name


def test_fp32_step_refuses_ragged():
    with pytest.raises(ValueError, match="fp16"):
        S.PKG.DADStep(S.PKG.SSRLModel().cuda(), S.PKG.ConfigView(S.dad_oracle.make_cfg("iemocap"), flavor="iemocap"),
                      precision="fp32", rng="explicit", ragged=True)
    with pytest.raises(ValueError, match="fp16"):
        S.PKG.pretrain.PretrainStep(precision="fp32", ragged=True)


def test_padded_batches_fall_back_to_the_dense_step():
    stores = _stores("R", "f32", "f32")
    want = _run("R", stores, "fp16", 2, False, padded=True)[0]
    got = _run("R", stores, "fp16", 2, True, padded=True)[0]
    S._assert_same(got, want)
