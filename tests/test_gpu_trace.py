"""The confirmation-bias log appended on the device (dad_trace_append, trace.TrainingTrace) on the MI355X:
the kernel alone against NumPy, overflow, the log of replayed golden steps against the golden arrays and
against the step's own outputs, no side effect on the step, and a whole train_epoch run."""
import numpy as np
import pytest
import torch

import dadpkg
import goldens
import gpu_harness as gh
from oracle import dad_oracle, synth

pytestmark = pytest.mark.gpu
PKG = dadpkg.pkg()
LIB = PKG._lib
H, R = 4, 4            # DAD_TRACE_HDR_WORDS, DAD_TRACE_REC_WORDS
N = 5000


def _np_append(words, capacity, tail, Bn, ids, tracked, n_samples, epoch):
    """dad.h's semantics of dad_trace_append on a NumPy copy of the trace words."""
    T = LIB.DAD_TAIL_HDR
    bits = tail.view(np.int32)
    for i in range(Bn):
        s = int(ids[i])
        if not (0 <= s < n_samples) or s not in tracked:
            continue
        pos = int(words[0])
        words[0] = pos + 1
        if pos < capacity:
            w2 = (int(tail[T + Bn + i]) & 0xff) | (0x100 if tail[T + 2 * Bn + i] != 0 else 0)
            words[H + R * pos:H + R * pos + R] = [epoch, s, w2, bits[T + i]]
    return words


def _tail(rs, Bn):
    """A synthetic tail buffer: random header, scores, labels 0..3 (as float) and masks."""
    T = LIB.DAD_TAIL_HDR
    t = rs.standard_normal(LIB.tail_floats(Bn)).astype(np.float32)
    t[T:T + Bn] = rs.random_sample(Bn).astype(np.float32)
    t[T + Bn:T + 2 * Bn] = rs.randint(0, 4, Bn).astype(np.float32)
    t[T + 2 * Bn:T + 3 * Bn] = rs.randint(0, 2, Bn).astype(np.float32)
    return t


def _append(tail, Bn, ids, bitmap, n_samples, epoch, trace, capacity):
    LIB.check(LIB.lib().dad_trace_append(LIB.ptr(tail), Bn, LIB.ptr(ids), LIB.ptr(bitmap), n_samples, epoch,
                                         LIB.ptr(trace), capacity, torch.cuda.current_stream().cuda_stream),
              "dad_trace_append")


def _bitmap(tracked, n_samples):
    return torch.from_numpy(PKG.trace.pack_bitmap(sorted(tracked), n_samples).view(np.int32)).cuda()


@pytest.mark.parametrize("Bn", [1, 63, 64, 65, 255, 256, 257, 1024])
def test_kernel_alone_matches_numpy(Bn):
    """Every wave and pass boundary; three successive appends into one trace per tracked set."""
    rs = np.random.RandomState(100 + Bn)
    base = rs.choice(N, Bn, replace=False).astype(np.int64)
    steps = []
    for k, epoch in enumerate((5, 6, 7)):
        ids = base if k == 0 else base[rs.permutation(Bn)]
        ids = ids.copy()
        if Bn >= 4:                               # two rows with an id outside [0, n_samples), never row 0 or Bn - 1
            a, b = rs.choice(np.arange(1, Bn - 1), 2, replace=False)
            ids[a], ids[b] = -1, N
        elif k:
            ids[0] = (-1, N)[k - 1]
        steps.append((epoch, ids, _tail(rs, Bn)))
    ids0 = steps[0][1]
    wave = ids0[64:128] if Bn >= 128 else ids0[:64]
    valid = lambda a: {int(i) for i in a if 0 <= i < N}
    sets = {"none": set(), "all": set(range(N)), "random50": valid(rs.choice(N, 50, replace=False)) | valid(base[:3]),
            "one_wave": valid(wave), "first_last": valid([ids0[0], ids0[Bn - 1]])}
    capacity = 3 * Bn
    dev = [(e, torch.from_numpy(i).cuda(), torch.from_numpy(t).cuda()) for e, i, t in steps]
    for name, tracked in sets.items():
        trace = torch.zeros(H + R * capacity, dtype=torch.int32, device="cuda")
        bitmap = _bitmap(tracked, N)
        want = np.zeros(H + R * capacity, np.int32)
        for (epoch, ids, tail), (_, ids_d, tail_d) in zip(steps, dev):
            _append(tail_d, Bn, ids_d, bitmap, N, epoch, trace, capacity)
            _np_append(want, capacity, tail, Bn, ids, tracked, N, epoch)
        got = trace.cpu().numpy()
        assert got[0] == want[0], (name, got[0], want[0])
        np.testing.assert_array_equal(got, want, err_msg=name)        # the records, their order, the score bits
        if name == "all":
            assert want[0] == sum(int(((i >= 0) & (i < N)).sum()) for _, i, _ in steps)
        if name == "first_last":
            assert want[0] >= 2 if Bn > 1 else want[0] == 1
        if name == "none":
            assert want[0] == 0


def test_overflow_drops_records_and_writes_nothing_past_the_capacity():
    rs = np.random.RandomState(7)
    Bn, capacity, alloc, canary = 200, 10, 64, 0x5A5A5A5A
    ids = rs.choice(N, Bn, replace=False).astype(np.int64)
    tracked = {int(i) for i in ids[[3, 60, 63, 64, 65, 127, 128, 199]]}        # 8 rows over four waves
    trace = torch.full((H + R * alloc,), canary, dtype=torch.int32, device="cuda")
    trace[:H + R * capacity] = 0
    want = np.zeros(H + R * capacity, np.int32)
    bitmap = _bitmap(tracked, N)
    for epoch in (1, 2, 3):
        perm = ids[rs.permutation(Bn)]
        tail = _tail(rs, Bn)
        _append(torch.from_numpy(tail).cuda(), Bn, torch.from_numpy(perm).cuda(), bitmap, N, epoch, trace, capacity)
        _np_append(want, capacity, tail, Bn, perm, tracked, N, epoch)
    got = trace.cpu().numpy()
    assert got[0] == want[0] == 24
    np.testing.assert_array_equal(got[:H + R * capacity], want)
    assert (got[H + R * capacity:] == canary).all()
    assert (want[H:].reshape(capacity, R)[:, 0] == [1] * 8 + [2] * 2).all()


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


@pytest.mark.parametrize("name", ["iemocap_default", "emodb_b8", "iemocap_fixed_thr"])
def test_log_of_replayed_golden_steps(name):
    """The fp32 replay of test_fused_step_matches_reference_goldens with a trace attached: the log against
    entries built from the golden arrays, and bit for bit against entries built from step.outputs()."""
    d, spec, cfg = goldens.load(name)
    Bn = goldens.step_inputs(spec, 0)["xn"].shape[0]
    n_samples = 4 * Bn + 3
    perm = np.random.RandomState(spec["seed"]).permutation(n_samples).astype(np.int64)
    tracked_ids, other_ids = perm[:(Bn + 1) // 2], perm[(Bn + 1) // 2:]
    step = gh.make_step(cfg, anchors=d["anchors"])
    sched = goldens.schedule(d)
    orc = None
    if not any(("s%d_mask" % s) in d for s, _ in sched):       # fixed threshold: the golden holds no mask
        orc = dad_oracle.DADOracle(*goldens.problem(spec), cfg, anchors=d["anchors"])
    tr = PKG.TrainingTrace(n_samples, tracked=tracked_ids.tolist(), epochs=len(sched))
    step.trace = tr
    want_out, want_gold, n_post = [], [], 0
    for s, epoch in sched:
        p = "s%d_" % s
        st = goldens.state(spec, s)
        gh.load_state(step, st)
        inp = goldens.step_inputs(spec, s)
        rs = np.random.RandomState(1000 + s)
        ids = np.empty(Bn, np.int64)              # tracked ids at the even batch positions, in a new order per step
        ids[0::2] = rs.permutation(tracked_ids)
        ids[1::2] = rs.permutation(other_ids)[:Bn // 2]
        clean, noisy, draws = gh.batches(inp)
        noisy["id"] = torch.from_numpy(ids)       # a host tensor: moved to the device by the step
        before = len(tr.bias_log())
        step.step(clean, noisy, epoch, lr=float(d[p + "lr"]), draws=draws)
        torch.cuda.synchronize()
        if epoch < cfg["WARMUP_EPOCHS"]:
            assert len(tr.bias_log()) == before, (name, s)          # warm-up steps add nothing
            continue
        n_post += 1
        o = {k: v.detach().cpu().numpy() for k, v in step.outputs(inp["xc"].shape[0], Bn).items()
             if k in ("score", "pred", "mask")}
        if p + "mask" in d:
            mask, score = d[p + "mask"], d[p + "score"]
        else:                                     # fixed threshold: the oracle's mask, as the parity test does
            orc.load_state(st)
            r = orc.step(inp, epoch, lr=float(d[p + "lr"]))
            mask, score = r["mask"], r["score"]
        pred = np.argmax(d[p + "z_teacher"], 1)
        for i in range(0, Bn, 2):
            want_out.append((epoch, int(ids[i]), int(o["pred"][i]), int(_bits(o["score"])[i]), bool(o["mask"][i] != 0)))
            want_gold.append((epoch, int(ids[i]), int(pred[i]), bool(np.asarray(mask).reshape(-1)[i] != 0)))
        got = np.array([e["certainty_score"] for e in tr.bias_log()[-((Bn + 1) // 2):]])
        assert gh.rel(got, np.asarray(score).reshape(-1)[0::2]) < 1e-4, (name, s)
    log = tr.bias_log()
    assert n_post >= 1 and len(log) == n_post * ((Bn + 1) // 2) == len(want_out)      # an empty log cannot pass
    assert tr.dropped == 0
    assert [(e["epoch"], e["sample_id"], e["pseudo_label"], int(_bits([e["certainty_score"]])[0]), e["is_masked_in"])
            for e in log] == want_out
    assert [(e["epoch"], e["sample_id"], e["pseudo_label"], e["is_masked_in"]) for e in log] == want_gold


def test_a_trace_changes_nothing_in_the_step():
    """Four chained fp16 counter-RNG steps that name their next batch, with and without a trace."""
    from test_gpu_graph import _device_batches, _state
    from test_gpu_parity import _problem
    cfg = dad_oracle.make_cfg("iemocap")
    data = []
    for k, seed in enumerate((41, 42, 43, 44)):
        c, n, _ = _device_batches(_problem(B=16, T=40, seed=seed, Bn=12, Tn=50))
        n["id"] = torch.arange(12 * k, 12 * k + 12, device="cuda")
        data.append((c, n))
    runs = []
    for with_trace in (False, True):
        s = gh.make_step(cfg, precision="fp16", rng="counter", seed=3)
        gh.load_state(s, synth.make_state(21, 1))
        if with_trace:
            s.trace = PKG.TrainingTrace(48, tracked="all", epochs=1)
        losses = []
        for i in range(4):
            l = s.step(*data[i], 60, next_batch=data[i + 1] if i < 3 else None)
            losses.append(torch.stack([l[k] for k in sorted(l)]))
        torch.cuda.synchronize()
        runs.append((s, _state(s), torch.stack(losses)))
    (a, sa, la), (b, sb, lb) = runs
    for name, x, y in zip(("student", "teacher", "exp_avg", "exp_avg_sq", "dacp", "grad"), sa, sb):
        assert torch.equal(x, y), name
    assert torch.equal(la, lb)
    log = b.trace.bias_log()
    assert [e["sample_id"] for e in log] == list(range(48)) and {e["epoch"] for e in log} == {60}
    # a batch without 'id' (the CASIA / EMODB collators' dict) logs nothing
    noid = {k: v for k, v in data[0][1].items() if k != "id"}
    b.step(data[0][0], noid, 60)
    torch.cuda.synchronize()
    assert len(b.trace.bias_log()) == 48 and b.trace.offered == 48
    # an 'id' of another length is refused
    bad = dict(data[0][1], id=torch.arange(11, device="cuda"))
    with pytest.raises(ValueError):
        b.step(data[0][0], bad, 60)


def test_train_epoch_fills_log_and_history():
    rs = np.random.RandomState(9)
    CK = PKG.checkpoint

    def store(labels):
        sizes = rs.randint(5, 41, size=64)
        feats = rs.standard_normal((int(sizes.sum()), 768)).astype(np.float16)
        offsets = np.concatenate([[0], np.cumsum(sizes)[:-1]])
        return PKG.data.FeatureStore(feats, sizes, offsets, rs.randint(0, 4, size=64) if labels else None)

    cs, ns = store(True), store(False)
    tracked = [0, 5, 9, 17, 31, 32, 40, 55, 62, 63]
    cfg = dad_oracle.make_cfg("iemocap", WARMUP_EPOCHS=1)
    lam = cfg["ECDA_CLASS_ATTENTION_LAMBDA"]
    runs = []
    for with_trace in (False, True):
        clean = PKG.DeviceLoader(cs, 8, shuffle=True, fused=True)
        noisy = PKG.DeviceLoader(ns, 8, shuffle=True, with_labels=False, fused=True)
        torch.manual_seed(0)
        model = PKG.SSRLModel().cuda()
        step = PKG.DADStep(model, PKG.ConfigView(cfg, flavor="iemocap"), precision="fp16", rng="counter", seed=2)
        tr = None
        if with_trace:
            tr = step.trace = PKG.TrainingTrace.for_loader(noisy, tracked=tracked, epochs=3)
            assert tr.n_samples == 64 and tr.capacity == 30
        avgs, rows = [], []
        for epoch in range(3):
            torch.manual_seed(100 + epoch)
            avgs.append(CK.train_epoch(step, clean, noisy, epoch))
            rows.append((step.ema_thresholds.cpu().clone(), step.class_quality_scores.cpu().clone()))
            if with_trace and epoch == 0:
                assert tr.bias_log() == [] and tr.history()["dacp_ema_thresholds"] == []      # warm-up adds nothing
        runs.append((avgs, rows, tr))
    (avg_a, _, _), (avg_b, rows, tr) = runs
    assert avg_a == avg_b                                   # train_epoch's dict with and without a trace
    log = tr.bias_log()
    assert tr.dropped == 0 and len(log) == 20
    for epoch in (1, 2):
        assert sorted(e["sample_id"] for e in log if e["epoch"] == epoch) == tracked     # each exactly once
    assert [e["epoch"] for e in log] == sorted(e["epoch"] for e in log)
    h = tr.history()
    assert set(h) == {"dacp_ema_thresholds", "dacp_class_quality", "ecda_class_attention"}
    for j, (tau, q) in enumerate(rows[1:]):
        np.testing.assert_array_equal(np.float32(h["dacp_ema_thresholds"][j]), tau.numpy())
        np.testing.assert_array_equal(np.float32(h["dacp_class_quality"][j]), q.numpy())
        np.testing.assert_allclose(h["ecda_class_attention"][j], torch.exp(lam * (q.mean() - q)).numpy(), rtol=1e-6)
    assert all(len(h[k]) == 2 for k in h)
