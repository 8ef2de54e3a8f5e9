"""Data outside the utterances cannot reach a step's results.

The 16-bit path reads 32-frame slabs that cross utterance ends, and the weight gradient's loader reads
padding rows into the MFMA; every other fused-step test has zeros (padded batches) or finite feature
rows (stores) where the kernels must not look, so a row masked by multiplying with zero would pass them
all and leak 0 x inf = NaN here.  include/dad.h states no precondition on padded frames and the reference
needs none (it multiplies finite values by the mask).

test_gpu_store16's shape A throughout: clean lengths {1, 31, 32, 33, 37}, noisy lengths {1, 33, 41}, every
utterance at an odd store row with unrelated rows around it."""
import numpy as np
import pytest
import torch

import test_gpu_store16 as S

pytestmark = pytest.mark.gpu
LIB = S.LIB
STATE = ("student", "teacher", "exp_avg", "exp_avg_sq", "dacp")


def _snapshot(step, losses, Bc, Bn):
    """test_gpu_store16._snapshot without its demand that the losses be finite."""
    torch.cuda.synchronize()
    out = {k: v.detach().cpu().numpy() for k, v in step.outputs(Bc, Bn).items() if torch.is_tensor(v)}
    out.update({k: np.float32(float(v)) for k, v in losses.items()})
    out["student"] = step.model.student_flat.detach().cpu().numpy()
    out["teacher"] = step.model.teacher_flat.detach().cpu().numpy()
    out["exp_avg"], out["exp_avg_sq"] = step.exp_avg.cpu().numpy(), step.exp_avg_sq.cpu().numpy()
    out["dacp"] = step.dacp.cpu().numpy()
    return out


def _state(step):
    torch.cuda.synchronize()
    return {"student": step.model.student_flat.detach().cpu().numpy(),
            "teacher": step.model.teacher_flat.detach().cpu().numpy(),
            "exp_avg": step.exp_avg.cpu().numpy(), "exp_avg_sq": step.exp_avg_sq.cpu().numpy(),
            "dacp": step.dacp.cpu().numpy()}


def _same(a, b, names=None, what=""):
    for name in (names or sorted(set(a) | set(b))):
        np.testing.assert_array_equal(a[name].view(np.int32) if a[name].dtype == np.float32 else a[name],
                                      b[name].view(np.int32) if b[name].dtype == np.float32 else b[name],
                                      err_msg="%s: %s" % (what, name))


# ------------------------------------------------------------------ padded batches
def _padded_batches(steps, fill):
    """The padded f32 batches shape A's f32 stores collate, the padded frames overwritten by fill(n)."""
    stores = S._stores("A", "f32", "f32")
    out = []
    for k in range(steps):
        pair = S._batches(stores, k, padded=True)
        for b in pair:
            f, pm = b["net_input"]["feats"], b["net_input"]["padding_mask"]
            assert pm.dtype == torch.bool and int(pm.sum()) > 0
            assert float(f[pm].abs().max()) == 0.0                  # the collator's zeros
            if fill is not None:
                f[pm] = torch.from_numpy(fill(int(pm.sum()))).to(f.device)
        out.append(pair)
    return out


def _run_padded(precision, steps, ahead, fill, finite=True):
    step = S._make_step(precision, "counter")
    batches = _padded_batches(steps, fill)
    Bc, Bn = (b["net_input"]["padding_mask"].shape[0] for b in batches[0])
    snaps, reported, states = [], [], [_state(step)]
    for k in range(steps):
        nxt = batches[k + 1] if ahead and k + 1 < steps else None
        losses = step.step(batches[k][0], batches[k][1], S.EPOCH, next_batch=nxt)
        reported.append(step.last_ahead)
        snaps.append(_snapshot(step, losses, Bc, Bn))
        if finite:
            assert all(np.isfinite(snaps[-1][n]) for n in losses), losses
        states.append(_state(step))
    return snaps, reported, states, step


_ZERO = {}


def _zero_padded(precision, steps, ahead):
    key = (precision, steps, ahead)
    if key not in _ZERO:
        snaps, reported, _, step = _run_padded(precision, steps, ahead, None)
        assert int(step.range_flag()) == 0
        _ZERO[key] = (snaps, reported)
    return _ZERO[key]


def _finite_garbage(seed):
    rs = np.random.RandomState(seed)
    return lambda n: rs.uniform(-8.0, 8.0, size=(n, 768)).astype(np.float32)


@pytest.mark.parametrize("steps,ahead", [(1, False), (3, True)], ids=["single", "chain_ahead"])
@pytest.mark.parametrize("precision", ["fp32", "fp16", "bf16"])
def test_finite_garbage_in_padded_frames_changes_nothing(precision, steps, ahead):
    """|x| <= 8 instead of zeros in the padded frames of xc and xn.  In the chain every step names its next
    batch: its clean rows are converted inside the weight gradient, its noisy rows on the tail launch's
    spare blocks."""
    want, want_reported = _zero_padded(precision, steps, ahead)
    got, reported, _, step = _run_padded(precision, steps, ahead, _finite_garbage(5))
    assert int(step.range_flag()) == 0
    assert reported == want_reported
    if ahead and precision != "fp32":
        assert reported == [(1, 0), (1, 0), (0, 0)], reported
    for k in range(steps):
        _same(got[k], want[k], what="%s step %d" % (precision, k))


def _out_of_range_garbage(seed):
    rs = np.random.RandomState(seed)

    def fill(n):
        g = rs.uniform(-8.0, 8.0, size=(n, 768)).astype(np.float32)
        g[rs.rand(n, 768) < 0.1] = 1.0e5
        g[0], g[-1] = 1.0e5, 1.0e5
        return g
    return fill


@pytest.mark.parametrize("steps,ahead", [(1, False), (3, True)], ids=["single", "chain_ahead"])
def test_out_of_range_garbage_in_padded_frames_is_ignored_or_skipped(steps, ahead):
    """1e5 (beyond fp16) in padded frames only, FP16 step.  Each step either equals the zero-padded run bit
    for bit with a clear range flag, or is skipped -- the state bit-identical to before it -- with
    `nonfinite` flagged.  Never a state that is neither, never a non-finite parameter."""
    want, _ = _zero_padded("fp16", steps, ahead)
    got, _, states, step = _run_padded("fp16", steps, ahead, _out_of_range_garbage(6), finite=False)
    flag = int(step.range_flag())
    skipped_before = False
    for k in range(steps):
        after = states[k + 1]
        assert all(np.isfinite(after[n]).all() for n in STATE), "step %d left a non-finite state" % k
        unchanged = all(np.array_equal(after[n].view(np.int32), states[k][n].view(np.int32)) for n in STATE)
        if unchanged:
            assert flag & LIB.RANGE_NONFINITE, "step %d was skipped without the nonfinite flag" % k
            skipped_before = True
        elif not skipped_before:
            _same(got[k], want[k], what="step %d differs from the zero-padded run and was not skipped" % k)
    print("out-of-range padding, %d step(s): %s, range flag %d" % (
        steps, "skipped" if skipped_before else "identical to the zero-padded run", flag))
    if not skipped_before:
        assert flag == 0


# ------------------------------------------------------------------ stores
def _nonfinite_rows(n):
    """Rows of NaN, +inf and -inf in turn, and every fourth row a mix of the three with finite values."""
    out = np.empty((n, 768), np.float32)
    vals = np.array([np.nan, np.inf, -np.inf], np.float32)
    for r in range(n):
        out[r] = vals[r % 3]
        if r % 4 == 3:
            out[r, ::2] = vals[np.arange(384) % 3]
            out[r, 1::2] = 1.0
    return out


def _poisoned_stores(clean_dtype, noisy_dtype):
    """Shape A's stores (test_gpu_store16._problem) with the rows of no utterance non-finite: the rows
    directly before and after every utterance and the store's last rows among them."""
    (fc, sc, oc, ic), (fn, sn, on, inn), labels = S._problem("A")
    rs = np.random.RandomState(160 + len("A"))
    lc, ln = S.LENS_A
    pc = S._layout(rs, [lc, lc[::-1]], filler=_nonfinite_rows)
    pn = S._layout(rs, [ln, [33, 41, 1]], filler=_nonfinite_rows)
    for (f, s, o, _), (f0, s0, o0, _) in ((pc, (fc, sc, oc, ic)), (pn, (fn, sn, on, inn))):
        assert np.array_equal(s, s0) and np.array_equal(o, o0) and f.shape == f0.shape
        own = np.zeros(len(f), bool)
        for a, n in zip(o, s):
            own[a:a + n] = True
            assert not np.isfinite(f[a - 1]).all() and not np.isfinite(f[a + n]).all()
        assert np.array_equal(f[own], f0[own]) and np.isfinite(f[own]).all()
        assert not np.isfinite(f[~own]).all(axis=1).any() and not own[-3:].any() and not own[0]
    D = S.D
    return (D.FeatureStore(pc[0], sc, oc, labels, dtype=S.DT[clean_dtype]), ic,
            D.FeatureStore(pn[0], sn, on, dtype=S.DT[noisy_dtype]), inn)


_FINITE = {}


def _finite_store_run(store_dtype, precision, steps, ahead):
    key = (store_dtype, precision, steps, ahead)
    if key not in _FINITE:
        _FINITE[key] = S._run("A", S._stores("A", store_dtype, store_dtype), precision, "counter", steps,
                              ahead=ahead)[:2]
    return _FINITE[key]


@pytest.mark.parametrize("steps,ahead", [(1, False), (3, True)], ids=["single", "chain_ahead"])
@pytest.mark.parametrize("store_dtype,precision", [("f32", "fp16"), ("fp16", "fp16"), ("bf16", "bf16"),
                                                   ("f32", "fp32")])
def test_nonfinite_rows_between_utterances_change_nothing(store_dtype, precision, steps, ahead):
    """NaN and +-inf in every store row that belongs to no utterance: bit-identical to the store whose
    unrelated rows are finite, with a clear range flag (test_gpu_store16._run asserts it, and that the
    losses are finite)."""
    want, want_reported = _finite_store_run(store_dtype, precision, steps, ahead)
    got, reported, _ = S._run("A", _poisoned_stores(store_dtype, store_dtype), precision, "counter", steps,
                              ahead=ahead)
    assert reported == want_reported
    if ahead and precision != "fp32":
        assert reported == [(1, 0), (1, 0), (0, 0)], reported
    S._assert_same(got, want)
