"""The 16-bit train step fed in place from fp16 / bf16 feature stores (ABI 10: dad_batch.xc_dtype /
xn_dtype; dad_prep.h and the weight gradient's clean-row conversion read the store rows in their own
type and widen them exactly).

The yardstick is test_gpu_data.test_store_mode_step_equals_padded_step: a step from a store equals the
step on the padded f32 batches the same store collates (StoreFeats.materialize()), bit for bit.  For a
16-bit store the padded batch holds the widened values, so the in-place step must give the same bits
in everything a step leaves behind.

Shape A (B=5, T=37, Bn=3, Tn=41): clean lengths {1, 31, 32, 33, 37} and noisy lengths {1, 33, 41} (a
length of 1, both sides of the 32-frame slab, a length equal to T); every utterance starts at an odd
store row with unrelated rows in between; B T + 2 Bn Tn = 431 rows, odd, so the clamped tail of the
two-rows-per-wave load loop runs.  Shape B (B=Bn=65, T=Tn=8): past the 64 utterances of the
in-register utterance tables.  Features are finite with |x| in [2^-8, 8]: nothing rounds to an fp16
subnormal or overflows, so the store's conversion (torch) and the kernels' cannot differ by a
flush-to-zero mode."""
import ctypes

import numpy as np
import pytest
import torch

import dadpkg
import gpu_harness as gh
from oracle import dad_oracle, synth

pytestmark = pytest.mark.gpu
PKG = dadpkg.pkg()
D = PKG.data
LIB = PKG._lib
EPOCH = 60          # post-warm-up: DACP and ECDA on
DT = {"f32": torch.float32, "fp16": torch.float16, "bf16": torch.bfloat16}
LENS_A = ([1, 31, 32, 33, 37], [1, 33, 41])


def _features(rs, n):
    mag = np.exp2(rs.uniform(-8.0, 3.0, size=(n, 768)))
    return (np.where(rs.rand(n, 768) < 0.5, -1.0, 1.0) * mag).astype(np.float32)


def _layout(rs, groups, filler=None, utterances=None):
    """Store layout of `groups` lists of utterance lengths: (features, sizes, offsets, index per group);
    each utterance starts at an odd row, with 1 or 3 unrelated rows before it and some after the last.
    filler(n) -> [n, 768]: what the unrelated rows hold instead of features (the utterances' rows and
    the draws from `rs` are the same either way).  utterances: one [length, 768] array per utterance, in
    the groups' order, written over the drawn rows of that utterance (tests/hidden_state.py)."""
    sizes, offsets, index, row = [], [], [], 0
    for lens in groups:
        ids = []
        for n in lens:
            row += 1 if row % 2 == 0 else 2
            ids.append(len(sizes))
            sizes.append(n)
            offsets.append(row)
            row += n
        index.append(ids)
    assert all(o % 2 == 1 for o in offsets)
    feats = _features(rs, row + 3)
    if filler is not None:
        unrelated = np.ones(row + 3, bool)
        for o, n in zip(offsets, sizes):
            unrelated[o:o + n] = False
        feats[unrelated] = filler(int(unrelated.sum()))
    if utterances is not None:
        assert len(utterances) == len(sizes)
        for o, n, rows in zip(offsets, sizes, utterances):
            assert rows.shape == (n, 768)
            feats[o:o + n] = rows
    return feats, np.array(sizes), np.array(offsets), index


_PROBLEMS = {}


def _problem(shape):
    """(features and layout of the clean and the noisy store, each holding two batches' utterances)"""
    if shape not in _PROBLEMS:
        rs = np.random.RandomState(160 + len(shape))
        if shape == "A":
            lc, ln = LENS_A
            groups_c, groups_n = [lc, lc[::-1]], [ln, [33, 41, 1]]
        else:
            mk = lambda: [8] + list(rs.randint(1, 9, size=64))
            groups_c, groups_n = [mk(), mk()], [mk(), mk()]
        _PROBLEMS[shape] = (_layout(rs, groups_c), _layout(rs, groups_n), rs.randint(0, 4, size=2 * len(groups_c[0])))
    return _PROBLEMS[shape]


def _stores(shape, clean_dtype, noisy_dtype):
    (fc, sc, oc, ic), (fn, sn, on, inn), labels = _problem(shape)
    return (D.FeatureStore(fc, sc, oc, labels, dtype=DT[clean_dtype]), ic,
            D.FeatureStore(fn, sn, on, dtype=DT[noisy_dtype]), inn)


def _batches(stores, k, padded=False):
    """Batch k (the stores' utterance group k % 2), store mode or materialised."""
    cs, ic, ns, inn = stores
    clean, noisy = cs.batch_index(ic[k % 2]), ns.batch_index(inn[k % 2], with_labels=False)
    if padded:
        for b in (clean, noisy):
            b["net_input"]["feats"] = b["net_input"]["feats"].materialize()
    return clean, noisy


def _draws(shape, k, rng):
    if rng != "explicit":
        return None
    (_, _, _, ic), (_, sn, _, inn), _ = _problem(shape)
    B, Bn, Tn = len(ic[0]), len(inn[0]), int(sn[inn[k % 2]].max())
    rs = np.random.RandomState(900 + k)
    return {"nw": rs.standard_normal((Bn, Tn, 768)).astype(np.float32),
            "ns": rs.standard_normal((Bn, Tn, 768)).astype(np.float32), "u": rs.rand(768).astype(np.float32),
            "start": rs.randint(0, max(1, Tn - 4), size=Bn), "keep1": rs.rand(B, 256) > 0.1,
            "keep2": rs.rand(Bn, 256) > 0.1}


def _make_step(precision, rng, prep_under_exchange=None):
    cfg = dad_oracle.make_cfg("iemocap")
    step = PKG.DADStep(PKG.SSRLModel().cuda(), PKG.ConfigView(cfg, flavor="iemocap"), precision=precision, rng=rng,
                       seed=9, prep_under_exchange=prep_under_exchange)
    gh.load_state(step, synth.make_state(40, 1))
    return step


def _snapshot(step, losses, Bc, Bn):
    """Everything a step leaves behind: the loss dict, outputs() (logits, score, pred, mask, embeddings,
    gradient ...), the parameters, the Adam moments and the DACP state."""
    torch.cuda.synchronize()
    out = {k: v.detach().cpu().numpy() for k, v in step.outputs(Bc, Bn).items() if torch.is_tensor(v)}
    out.update({k: np.float32(float(v)) for k, v in losses.items()})
    out["student"] = step.model.student_flat.detach().cpu().numpy()
    out["teacher"] = step.model.teacher_flat.detach().cpu().numpy()
    out["exp_avg"], out["exp_avg_sq"] = step.exp_avg.cpu().numpy(), step.exp_avg_sq.cpu().numpy()
    out["dacp"] = step.dacp.cpu().numpy()
    assert all(np.isfinite(float(v)) for v in losses.values()), losses
    return out


def _run(shape, stores, precision, rng, steps, padded=False, epoch=EPOCH, ahead=False, prep_under_exchange=None):
    """`steps` steps over the stores' batches; the snapshot after each, and what the library reported
    about each next batch (DADStep.last_ahead)."""
    step = _make_step(precision, rng, prep_under_exchange)
    batches = [_batches(stores, k, padded) for k in range(steps)]
    Bc, Bn = batches[0][0]["net_input"]["padding_mask"].shape[0], batches[0][1]["net_input"]["padding_mask"].shape[0]
    snaps, reported = [], []
    for k in range(steps):
        nxt = batches[k + 1] if ahead and k + 1 < steps else None
        losses = step.step(batches[k][0], batches[k][1], epoch, draws=_draws(shape, k, rng), next_batch=nxt)
        reported.append(step.last_ahead)
        snaps.append(_snapshot(step, losses, Bc, Bn))
    assert int(step.range_flag()) == 0
    return snaps, reported, step


def _assert_same(got, want):
    assert len(got) == len(want)
    for k, (a, b) in enumerate(zip(got, want)):
        assert set(a) == set(b)
        for name in a:
            np.testing.assert_array_equal(a[name], b[name], err_msg="step %d: %s" % (k, name))


_REFS = {}


def _materialised(shape, clean_dtype, noisy_dtype, precision, rng, steps):
    """The steps on the padded f32 batches the stores collate (computed once per case, never changed)."""
    key = (shape, clean_dtype, noisy_dtype, precision, rng, steps)
    if key not in _REFS:
        _REFS[key] = _run(shape, _stores(shape, clean_dtype, noisy_dtype), precision, rng, steps, padded=True)[0]
    return _REFS[key]


def _no_materialize(monkeypatch):
    def refuse(self):
        raise AssertionError("StoreFeats.materialize(): the step made a padded copy of a store batch")
    monkeypatch.setattr(D.StoreFeats, "materialize", refuse)


# ------------------------------------------------------------------ 1. in place equals widened
@pytest.mark.parametrize("rng", ["explicit", "counter"])
@pytest.mark.parametrize("precision", ["fp16", "bf16"])
@pytest.mark.parametrize("store_dtype", ["fp16", "bf16"])
def test_in_place_step_equals_widened_step(store_dtype, precision, rng, monkeypatch):
    want = _materialised("A", store_dtype, store_dtype, precision, rng, 3)
    _no_materialize(monkeypatch)
    got = _run("A", _stores("A", store_dtype, store_dtype), precision, rng, 3)[0]
    _assert_same(got, want)


def test_in_place_step_equals_widened_step_past_the_register_tables(monkeypatch):
    """B = Bn = 65: the source rows come through dad_src_row, not the in-register utterance tables."""
    want = _materialised("B", "fp16", "fp16", "fp16", "counter", 1)
    _no_materialize(monkeypatch)
    _assert_same(_run("B", _stores("B", "fp16", "fp16"), "fp16", "counter", 1)[0], want)


# ------------------------------------------------------------------ 2. no copy is made
def test_fp16_step_reads_fp16_stores_without_a_copy(monkeypatch):
    stores = _stores("A", "fp16", "fp16")
    _no_materialize(monkeypatch)
    _run("A", stores, "fp16", "counter", 1)


def test_fp32_step_still_widens_16bit_stores(monkeypatch):
    """precision='fp32' keeps the fallback: both batches go through materialize(), and the results are
    those of the materialised step."""
    want = _materialised("A", "fp16", "fp16", "fp32", "explicit", 1)
    calls = []
    real = D.StoreFeats.materialize
    monkeypatch.setattr(D.StoreFeats, "materialize", lambda self: (calls.append(self), real(self))[1])
    got = _run("A", _stores("A", "fp16", "fp16"), "fp32", "explicit", 1)[0]
    assert len(calls) == 2
    _assert_same(got, want)


# ------------------------------------------------------------------ 3. prepared ahead
@pytest.mark.parametrize("defer", [0, LIB.PREP_CLEAN, LIB.PREP_CLEAN | LIB.PREP_NOISY],
                         ids=["in_launch", "split_clean", "split_all"])
@pytest.mark.parametrize("store_dtype,precision", [("fp16", "fp16"), ("bf16", "fp16"), ("fp16", "bf16")])
def test_chain_prepared_ahead_from_16bit_stores(store_dtype, precision, defer, monkeypatch):
    """Four steps that name their next batch: in this step's launches (dad_step_backward_ahead), or with
    parts left to dad_step_prepare_rows on the side stream (dad_step_backward_ahead_split).  Bit-identical
    to the chain without next_batch, and the library reported *prepped = 1 (and the deferred parts as
    pending) for every step but the last."""
    _no_materialize(monkeypatch)
    stores = _stores("A", store_dtype, store_dtype)
    want, plain, _ = _run("A", stores, precision, "counter", 4)
    assert plain == [(0, 0)] * 4
    got, reported, step = _run("A", stores, precision, "counter", 4, ahead=True, prep_under_exchange=defer or None)
    assert reported == [(1, defer)] * 3 + [(0, 0)], reported
    _assert_same(got, want)


# ------------------------------------------------------------------ 4. mixed stores
@pytest.mark.parametrize("clean_dtype,noisy_dtype", [("f32", "fp16"), ("fp16", "f32"), ("fp16", "bf16")])
@pytest.mark.parametrize("precision", ["fp16", "bf16"])
def test_mixed_store_dtypes(clean_dtype, noisy_dtype, precision, monkeypatch):
    """The clean and the noisy store are separate objects and may differ in dtype; both are read in
    place, in a chain that prepares ahead and in one that does not."""
    want = _materialised("A", clean_dtype, noisy_dtype, precision, "counter", 3)
    _no_materialize(monkeypatch)
    stores = _stores("A", clean_dtype, noisy_dtype)
    _assert_same(_run("A", stores, precision, "counter", 3)[0], want)
    got, reported, _ = _run("A", stores, precision, "counter", 3, ahead=True)
    assert reported == [(1, 0), (1, 0), (0, 0)]
    _assert_same(got, want)


# ------------------------------------------------------------------ 5. the clean branch is the store's bytes
def test_fp16_clean_branch_sees_the_same_bytes_from_fp16_and_f32_stores(monkeypatch):
    """Warm-up epoch (cross-entropy on the clean batch only), fp16 operands: the fp16 store that
    FeatureStore(dtype=torch.float16) makes from f32 features holds the bytes the preparation rounds the
    f32 store's rows to."""
    _no_materialize(monkeypatch)
    a = _run("A", _stores("A", "f32", "f32"), "fp16", "counter", 3, epoch=0)[0]
    b = _run("A", _stores("A", "fp16", "fp16"), "fp16", "counter", 3, epoch=0)[0]
    for k in range(3):
        for name in ("total_loss", "supervised_ce_loss", "consistency_loss", "ecda_loss", "z_clean", "e_clean",
                     "student", "teacher", "exp_avg", "exp_avg_sq"):
            np.testing.assert_array_equal(b[k][name], a[k][name], err_msg="step %d: %s" % (k, name))


# ------------------------------------------------------------------ 6. C ABI errors
def _abi_case(precision, padded):
    rng = "explicit" if precision == "fp32" else "counter"
    step = _make_step(precision, rng)
    clean, noisy = _batches(_stores("A", "f32", "f32"), 0, padded)
    cfg, bt, st = step._prepare(clean, noisy, EPOCH, None, _draws("A", 0, rng))
    return step, cfg, bt, st, LIB.ptr(step._workspace(cfg)), (clean, noisy)


def _device_state(step):
    torch.cuda.synchronize()
    b = step._last
    return [t.clone() for t in (step.model.student_flat.detach(), step.model.teacher_flat.detach(), step.exp_avg,
                                step.exp_avg_sq, step.grad, step.dacp, b["tail"], b["emb"], b["logits"],
                                step.w1bf_student.view(torch.int16), step.w1bf_teacher.view(torch.int16))]


def _entry_points(L, cfg, bt, st, ws, stream, ncfg, nbt):
    done, pend = ctypes.c_int(7), ctypes.c_int(7)
    return {"dad_step": lambda: L.dad_step(cfg, bt, st, ws, stream),
            "dad_step_encode": lambda: L.dad_step_encode(cfg, bt, st, ws, stream),
            "dad_step_compute": lambda: L.dad_step_compute(cfg, bt, st, ws, stream),
            "dad_step_backward_ahead": lambda: L.dad_step_backward_ahead(cfg, bt, st, ws, stream, ncfg, nbt,
                                                                          ctypes.byref(done)),
            "dad_step_backward_ahead_split": lambda: L.dad_step_backward_ahead_split(
                cfg, bt, st, ws, stream, ncfg, nbt, 0, ctypes.byref(done), ctypes.byref(pend)),
            "dad_step_prepare_rows": lambda: L.dad_step_prepare_rows(cfg, bt, ws, stream, 3)}


def test_c_abi_refuses_16bit_rows_in_fp32_and_dtypes_on_padded_batches():
    L = LIB.lib()
    # FP32 precision, a store batch marked fp16: DAD_E_UNSUPPORTED, as this batch and as the next one
    step, cfg, bt, st, ws, keep = _abi_case("fp32", padded=False)
    before = _device_state(step)
    ok = LIB.DadBatch.from_buffer_copy(bt)
    bad = LIB.DadBatch.from_buffer_copy(bt)
    bad.xc_dtype = LIB.STORE_F16
    ncfg = LIB.DadConfig.from_buffer_copy(cfg)
    ncfg.counter = cfg.counter + 1
    stream = step._stream()
    for name, call in _entry_points(L, cfg, bad, st, ws, stream, None, None).items():
        assert call() == LIB.E_UNSUPPORTED, name
    for name in ("dad_step_backward_ahead", "dad_step_backward_ahead_split"):
        assert _entry_points(L, cfg, ok, st, ws, stream, ncfg, bad)[name]() == LIB.E_UNSUPPORTED, name
    bad.xc_dtype, bad.xn_dtype = LIB.STORE_F32, LIB.STORE_BF16
    assert L.dad_step(cfg, bad, st, ws, stream) == LIB.E_UNSUPPORTED
    for a, b in zip(_device_state(step), before):
        assert torch.equal(a, b)
    # a padded batch with a dtype: DAD_E_ARG in every precision
    for precision in ("fp16", "fp32"):
        step, cfg, bt, st, ws, keep = _abi_case(precision, padded=True)
        before = _device_state(step)
        ok = LIB.DadBatch.from_buffer_copy(bt)
        ncfg = LIB.DadConfig.from_buffer_copy(cfg)
        ncfg.counter = cfg.counter + 1
        stream = step._stream()
        for field in ("xc_dtype", "xn_dtype"):
            bad = LIB.DadBatch.from_buffer_copy(bt)
            setattr(bad, field, LIB.STORE_F16)
            for name, call in _entry_points(L, cfg, bad, st, ws, stream, None, None).items():
                if precision == "fp32" and name == "dad_step_prepare_rows":
                    assert call() == LIB.E_UNSUPPORTED      # (FP32 has no row preparation at all)
                else:
                    assert call() == LIB.E_ARG, (precision, field, name)
            if precision == "fp16":
                for name in ("dad_step_backward_ahead", "dad_step_backward_ahead_split"):
                    assert _entry_points(L, cfg, ok, st, ws, stream, ncfg, bad)[name]() == LIB.E_ARG, name
        for a, b in zip(_device_state(step), before):
            assert torch.equal(a, b)
