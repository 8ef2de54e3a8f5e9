"""dad_rank_metrics and dad_rank_eval_columns on the MI355X (csrc/rank.hip, evaluate.rank_metrics,
certainty_ranking_store, validate_store(ranking=True), firewall_report) against the NumPy restatement
tests/rank_ref.py (computed once per input on the CPU).  The inputs are tests/rank_cases.py: the wave, tile and chunk
edges with every key pattern, threshold kind, Q and B; tests/test_rank_ref_cpu.py shows that each wrong-answer control
of rank_ref.WRONG fails compare() on one of them.

Bounds: every integer, `order`, `cum_pos`, `tie_end` and the float32 quantiles are equal; each double is within
(M + 4) 2^-53 sum |terms|, the bound of a sum of M doubles in any order (rank_ref.value_bound).  Worst ratio of an
error to that bound measured on the MI355X over the ten cases and every chunk count: 0.082 (n = 65, m = 10; 0 at
n <= 2 and n = 64 with m = 1, 0.047 / 0.012 / 0.022 / 0.011 / 0.0028 / 0.00072 at n = 63 / 255 / 256 / 257 / 1,100 /
4,097)."""
import ctypes
import functools
import os
import sys

import numpy as np
import pytest
import torch

import dadpkg
import gpu_harness as gh
import rank_cases
import rank_ref as R
from oracle import data_oracle as do

sys.path.insert(0, os.path.join(dadpkg.ROOT, "tests", "golden"))
from gen_rank_golden import probs_of  # noqa: E402

pytestmark = pytest.mark.gpu
PKG = dadpkg.pkg()
D = PKG.data
E = PKG.evaluate
L = PKG._lib
GUARD = 256
OUTPUTS = ("order", "cum_pos", "tie_end", "counts", "values", "quant", "bin_counts", "bin_sum")
DTYPES = {"order": np.int32, "cum_pos": np.int32, "tie_end": np.uint8, "counts": np.int64, "values": np.float64,
          "quant": np.float32, "bin_counts": np.int64, "bin_sum": np.float64}
STORE_DTYPES = {"f32": torch.float32, "f16": torch.float16}


def _shapes(n, m, Q, B):
    return {"order": (m, n), "cum_pos": (m, n), "tie_end": (m, n), "counts": (m, L.RK_COUNTS), "values": (m, L.RK_VALUES),
            "quant": (m, Q), "bin_counts": (m, B, 2), "bin_sum": (m, B)}


def _guarded(nbytes):
    """A device buffer of nbytes (0x5A) between two guards of 0xA5."""
    g = torch.full((nbytes + 2 * GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
    g[GUARD:GUARD + nbytes] = 0x5A
    return g


def _run(c, chunks=0, curves=True, fn="dad_rank_metrics", **override):
    """One call on buffers with guard bytes: ({name: host array}, return code).  Asserts that the inputs are unchanged
    and that no byte outside an output's [m][...] block was written."""
    key, flags = np.ascontiguousarray(c["key"]), np.ascontiguousarray(c["flags"])
    m, n = key.shape
    Q, B = len(c["gammas"]), int(c["bins"])
    dev = {"key": torch.from_numpy(key).cuda(), "flags": torch.from_numpy(flags).cuda(),
           "thr": torch.from_numpy(np.asarray(c["thr"], np.float32)).cuda(),
           "gammas": torch.tensor(list(c["gammas"]) or [0.0], dtype=torch.float32).cuda()}
    before = {k: v.clone() for k, v in dev.items()}
    shapes = _shapes(n, m, Q, B)
    bufs = {name: _guarded(int(np.prod(shapes[name])) * np.dtype(DTYPES[name]).itemsize) for name in OUTPUTS}
    ws = torch.empty(int(L.lib().dad_rank_workspace_bytes(n, m)), dtype=torch.uint8, device="cuda")
    ws.fill_(0xCD)        # (the workspace needs no initialisation: any content will do)
    a = L.DadRankArgs()
    for name, t in dev.items():
        setattr(a, name, t.data_ptr())
    for name in OUTPUTS:
        setattr(a, name, bufs[name].data_ptr() + GUARD)
    if not curves:
        a.order = a.cum_pos = a.tie_end = None
    if Q == 0:
        a.gammas = a.quant = None
    if B == 0:
        a.bin_counts = a.bin_sum = None
    a.n, a.m, a.Q, a.B = n, m, Q, B
    a.bin_lo, a.bin_hi = c["bin_range"]
    for k, v in override.items():
        setattr(a, k, v)
    stream = torch.cuda.current_stream().cuda_stream
    if chunks or fn == "dad_rank_metrics_chunked":
        rc = L.lib().dad_rank_metrics_chunked(a, int(chunks), L.ptr(ws), stream)
    else:
        rc = L.lib().dad_rank_metrics(a, L.ptr(ws), stream)
    torch.cuda.synchronize()
    for k, v in dev.items():
        assert torch.equal(v.view(torch.uint8), before[k].view(torch.uint8)), "input %s was written" % k
    out = {}
    for name in OUTPUTS:
        host = bufs[name].cpu().numpy()
        assert np.all(host[:GUARD] == 0xA5) and np.all(host[len(host) - GUARD:] == 0xA5), "write outside %s" % name
        out[name] = host[GUARD:len(host) - GUARD].copy().view(DTYPES[name]).reshape(shapes[name])
    return out, rc


def _untouched(out, names=OUTPUTS):
    return all(np.all(out[name].view(np.uint8) == 0x5A) for name in names)


def _same_bits(a, b, names=OUTPUTS):
    return [name for name in names if a[name].tobytes() != b[name].tobytes()]


# ---------------------------------------------------------------- 1. the case list against rank_ref, and the identities
@pytest.mark.parametrize("index", range(len(rank_cases.SHAPES)), ids=[rank_cases.case(i)["name"] for i in range(10)])
def test_cases_against_the_restatement_and_the_identities(index):
    c, ref = rank_cases.case(index), rank_cases.reference(index)
    got, rc = _run(c)
    assert rc == 0
    bad, worst = rank_cases.compare(got, ref)
    print("%s: worst |double - rank_ref| / bound %.3e" % (c["name"], worst))
    assert not bad, bad
    again, _ = _run(c)
    assert not _same_bits(got, again)                         # two calls
    for chunks in (1, 3):
        other, rc = _run(c, chunks=chunks)
        assert rc == 0 and not _same_bits(got, other), chunks  # every chunk count
    bare, rc = _run(c, curves=False)                          # curve pointers NULL
    assert rc == 0 and _untouched(bare, OUTPUTS[:3]) and not _same_bits(got, bare, OUTPUTS[3:])


@pytest.mark.parametrize("index", [4, 6, 8], ids=["n65_m10", "n256_m16", "n1100_m10"])
def test_a_row_permutation_changes_no_bit_of_the_blocks(index):
    c = rank_cases.case(index)
    n = c["key"].shape[1]
    perm = np.random.RandomState(77 + index).permutation(n)
    got, _ = _run(c)
    moved, _ = _run(dict(c, key=c["key"][:, perm], flags=c["flags"][:, perm]))
    assert not _same_bits(got, moved, ("counts", "values", "quant", "bin_counts", "bin_sum"))
    assert np.array_equal(got["tie_end"], moved["tie_end"])
    for j in range(c["key"].shape[0]):
        M = int(got["counts"][j, R.C_MEMBERS])
        ends = got["tie_end"][j] != 0                # (inside a run the positives come in index order)
        assert np.array_equal(got["cum_pos"][j][ends], moved["cum_pos"][j][ends])
        back = perm[moved["order"][j, :M]]
        # the same rows at the same positions up to the order inside a run of equal keys, which follows the index
        assert np.array_equal(c["key"][j][back] + np.float32(0), c["key"][j][got["order"][j, :M]] + np.float32(0))
        assert sorted(back.tolist()) == sorted(got["order"][j, :M].tolist())
        assert np.all(moved["order"][j, M:] == -1)


def test_the_planned_chunk_count_at_4097_rows_is_more_than_one():
    rt, ch, per = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    assert L.lib().dad_rank_plan(4097, 16, cus, ctypes.byref(rt), ctypes.byref(ch), ctypes.byref(per)) == 0
    assert rt.value == 17 and ch.value > 1


# ---------------------------------------------------------------- 2. error codes
def test_every_error_leaves_the_outputs_untouched():
    c = rank_cases.case(3)                           # Q = 8, B = 64: every pointer is required
    assert len(c["gammas"]) == 8 and c["bins"] == 64
    for fn in ("dad_rank_metrics", "dad_rank_metrics_chunked"):
        for kw in (dict(n=0), dict(n=L.RK_MAX_N + 1), dict(m=0), dict(m=L.RK_MAX_M + 1), dict(Q=-1),
                   dict(Q=L.RK_MAX_Q + 1), dict(B=-1), dict(B=L.RK_MAX_BINS + 1)):
            out, rc = _run(c, fn=fn, **kw)
            assert rc == L.E_SHAPE and _untouched(out), (fn, kw)
        for kw in (dict(key=None), dict(flags=None), dict(thr=None), dict(counts=None), dict(values=None),
                   dict(gammas=None), dict(quant=None), dict(bin_sum=None), dict(bin_counts=None),
                   dict(bin_lo=0.75), dict(bin_hi=float("nan"))):
            out, rc = _run(c, fn=fn, **kw)
            assert rc == L.E_ARG and _untouched(out), (fn, kw)


# ---------------------------------------------------------------- 3. dad_rank_eval_columns
def _columns(score, probs, pred, labels):
    n = len(score)
    key = torch.full((L.RK_EVAL_COLUMNS, n), -7.0, dtype=torch.float32, device="cuda")
    flags = torch.full((L.RK_EVAL_COLUMNS, n), 0xEE, dtype=torch.uint8, device="cuda")
    dev = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()
    s, p, q, y = dev(score), dev(probs), dev(pred), dev(labels)
    rc = L.lib().dad_rank_eval_columns(L.ptr(s), L.ptr(p), L.ptr(q), L.ptr(y), n, L.ptr(key), L.ptr(flags),
                                       torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert rc == 0
    return key, flags


@pytest.mark.parametrize("n", [1, 257, 1100])
@pytest.mark.parametrize("labelled", [True, False], ids=["labels", "no_labels"])
def test_eval_columns_are_the_restatements(n, labelled):
    rs = np.random.RandomState(900 + n)
    probs = probs_of(900 + n, n)
    score = (probs.max(axis=1) * rs.random_sample(n)).astype(np.float32)
    pred = probs.argmax(axis=1).astype(np.int64)
    labels = rs.randint(0, 4, n).astype(np.int64)
    if n > 1:
        pred[rs.randint(0, n, 5)] = (-1, 4, 7, -100, 2 ** 40)
        labels[rs.randint(0, n, 5)] = (-1, 4, 9, -3, 2 ** 33)
    key, flags = _columns(score, probs, pred, labels if labelled else None)
    want_key, want_flags = R.eval_columns(score, probs, pred, labels if labelled else None)
    assert np.array_equal(key.cpu().numpy().view(np.uint32), want_key.view(np.uint32))
    assert np.array_equal(flags.cpu().numpy(), want_flags)
    if not labelled:
        assert not np.any(want_flags & R.POSITIVE) and np.any(want_flags & R.MEMBER)


# ---------------------------------------------------------------- 4. the Python surface for columns of one's own
def test_rank_metrics_with_curves_and_its_helpers():
    c, ref = rank_cases.case(7), rank_cases.reference(7)           # n = 257, m = 10, Q = 0, B = 0
    member = torch.from_numpy((c["flags"] & R.MEMBER) != 0)
    positive = torch.from_numpy((c["flags"] & R.POSITIVE) != 0)
    cols = E.rank_metrics(torch.from_numpy(c["key"]).cuda(), member, positive, thresholds=c["thr"], curves=True)
    bare = E.rank_metrics(torch.from_numpy(c["key"]).cuda(), member, positive, thresholds=c["thr"], _chunks=2)
    assert len(cols) == 10
    for j, col in enumerate(cols):
        cnt = ref["counts"][j]
        assert (col["members"], col["positives"], col["nonfinite"], col["runs"], col["u2"], col["accepted"],
                col["accepted_positives"]) == tuple(int(v) for v in cnt[:7])
        one = {k: ref[k][j] for k in ("counts", "tie_end", "cum_pos")}
        for mine, theirs in zip(E.risk_coverage(col), R.risk_coverage(one)):
            assert np.array_equal(mine, theirs)
        for mine, theirs in zip(E.roc_points(col), R.roc_points(one)):
            assert np.array_equal(mine, theirs)
        assert np.array_equal(col["order"].cpu().numpy(), ref["order"][j])
        assert all(col[k] == bare[j][k] for k in ("auroc", "average_precision", "aurc", "key_mean", "key_std"))
    with pytest.raises(ValueError, match="rows"):
        E.rank_metrics(torch.zeros(17, 4, device="cuda"), True, True)


# ---------------------------------------------------------------- 5. end to end on the tests' synthetic stores
@functools.lru_cache(None)
def _model(seed=11):
    stu, tea = do.eval_weights(seed)
    model = PKG.SSRLModel().cuda()
    with torch.no_grad():
        model.student_flat.copy_(torch.from_numpy(gh.flat(stu)))
        model.teacher_flat.copy_(torch.from_numpy(gh.flat(tea)))
    return model


@functools.lru_cache(None)
def _store(dt):
    """The 37-utterance shuffled subset of tests/test_gpu_eval_split.py (39 rows, two samples twice, two labels of -1),
    rebuilt from its seeds."""
    sizes = np.concatenate([[0, 1, 3, 31, 32, 33, 63, 64, 65, 96], np.random.RandomState(13).randint(1, 71, 27)])
    labels = np.random.RandomState(14).randint(0, 4, len(sizes))
    labels[[5, 20]] = -1
    perm = np.random.RandomState(15).permutation(len(sizes))
    order = np.concatenate([perm[:30], [perm[3], perm[11]], perm[30:]])
    offsets = np.concatenate([[0], np.cumsum(sizes)[:-1]])
    feats = np.random.RandomState(12).standard_normal((int(sizes.sum()), 768)).astype(np.float32)
    return D.FeatureStore(feats, sizes, offsets, labels.astype(np.int64), dtype=STORE_DTYPES[dt]).subset(order)


def _ref_of(r, labels, thr, gammas, bins):
    host = lambda t: t.cpu().numpy()
    key, flags = R.eval_columns(host(r["score"]), host(r["probs"]), host(r["pred"]), labels)
    full = np.full(10, np.nan, np.float32)
    if thr is not None:
        full[1:5] = thr
    return R.rank_metrics(key, flags, full, gammas, bins, (0.0, 1.0))


def _blocks_of(r):
    cols = r["columns"]
    return {"counts": np.array([[c["members"], c["positives"], c["nonfinite"], c["runs"], c["u2"], c["accepted"],
                                 c["accepted_positives"], int(c["auroc_valid"])] for c in cols], np.int64),
            "values": np.array([[c["auroc"], c["average_precision"], c["aurc"], c["key_mean"], c["key_std"],
                                 c["key_min"], c["key_max"], 0.0] for c in cols]),
            "quant": np.stack([c["quantiles"] for c in cols]),
            "bin_counts": np.stack([np.stack([c["bin_counts"], c["bin_positives"]], axis=1) for c in cols]),
            "bin_sum": np.stack([c["bin_key_sum"] for c in cols])}


@pytest.mark.parametrize("use_teacher", [False, True], ids=["student", "teacher"])
@pytest.mark.parametrize("precision", ["fp32", "fp16"])
@pytest.mark.parametrize("dt", ["f32", "f16"])
def test_certainty_ranking_store_is_the_restatement_of_its_own_scores(dt, precision, use_teacher):
    model, store = _model(), _store(dt)
    thr = np.array([0.05, 0.1, 0.02, 0.2], np.float32)
    gam = (0.4, 0.8, 0.613)
    r = E.certainty_ranking_store(model, store, use_teacher=use_teacher, thresholds=thr, quantiles=gam, bins=20,
                                  precision=precision, outputs=("t_emb",) if use_teacher else ())
    labels = store.labels_d.cpu().numpy()
    ref = _ref_of(r, labels, thr, gam, 20)
    bad, worst = rank_cases.compare(_blocks_of(r), ref, curves=False)
    assert not bad, bad
    if use_teacher:        # the ranked model is the teacher: dad_predict_head on the pass's t_emb
        cls = model.teacher_classifier
        want = {"probs": torch.empty(len(store), 4, device="cuda"), "score": torch.empty(len(store), device="cuda"),
                "pred": torch.empty(len(store), dtype=torch.int64, device="cuda")}
        w2, b2 = cls.fc_layer.weight.detach().contiguous(), cls.fc_layer.bias.detach().contiguous()
        L.check(L.lib().dad_predict_head(L.ptr(r["t_emb"]), len(store), L.ptr(w2), L.ptr(b2), 1, None, L.ptr(want["probs"]),
                                         L.ptr(want["score"]), L.ptr(want["pred"]),
                                         torch.cuda.current_stream().cuda_stream), "dad_predict_head")
        torch.cuda.synchronize()
        for k, v in want.items():
            assert torch.equal(r[k], v), k
    # the derived blocks say what the columns say
    assert r["selective"]["overall"]["n"] == 37 and r["quantile_thresholds"].shape == (4, 3)
    assert np.array_equal(r["quantile_thresholds"].view(np.uint32), ref["quant"][1:5].view(np.uint32))
    for c, g in enumerate(r["gate"]):
        cnt = ref["counts"][1 + c]
        assert g["members"] == cnt[R.C_MEMBERS] and g["passed"] == cnt[R.C_ACCEPTED]
        assert g["passed_right"] + g["passed_wrong"] == g["passed"]
        assert g["passed_right"] + g["passed_wrong"] + g["blocked_right"] + g["blocked_wrong"] == g["members"]
    assert sum(r["reliability"]["count"]) == 37
    assert r["ovr"]["auroc_macro"] == float(np.mean([c["auroc"] for c in r["columns"][6:10]]))
    cs = r["confidence_stats"]
    assert cs["min_confidence"] <= cs["mean_confidence"] <= cs["max_confidence"] and cs["std_confidence"] >= 0.0


def test_an_unlabelled_store_still_gives_quantiles_and_gate_counts():
    lab = _store("f32")
    store = lab.subset(np.arange(len(lab)), with_labels=False)
    assert store.labels_d is None
    r = E.certainty_ranking_store(_model(), store, thresholds=[0.1] * 4, quantiles=(0.5,))
    ref = _ref_of(r, None, np.full(4, 0.1, np.float32), (0.5,), 20)
    bad, _ = rank_cases.compare(_blocks_of(r), ref, curves=False)
    assert not bad, bad
    assert sum(g["members"] for g in r["gate"]) == len(store) and all(g["passed_right"] == 0 for g in r["gate"])
    assert not np.any(np.isnan(r["quantile_thresholds"][[g["members"] > 0 for g in r["gate"]]]))


def test_the_fixtures_thresholds_through_the_device_path():
    g = np.load(os.path.join(dadpkg.ROOT, "tests", "golden", "eval_rank.npz"))
    n = int(g["n"])
    probs = probs_of(int(g["seed"]), n)
    key, flags = _columns(g["score"], probs, g["pred"], None)
    c = {"key": key.cpu().numpy(), "flags": flags.cpu().numpy(), "thr": g["tau_hat"][[0, 0, 1, 2, 3, 0, 0, 0, 0, 0]],
         "gammas": (float(g["gamma"]),), "bins": 0, "bin_range": (0.0, 1.0)}
    got, rc = _run(c)
    assert rc == 0
    assert np.array_equal(got["order"][0], g["rank"])
    assert np.array_equal(got["quant"][1:5, 0].view(np.uint32), g["tau_hat"].view(np.uint32))
    v = got["values"][5]
    stats = np.array([v[R.V_KEY_MEAN], v[R.V_KEY_STD], v[R.V_KEY_MIN], v[R.V_KEY_MAX]])
    assert np.all(np.abs(stats - g["stats"]) <= (n + 4) * R.U * np.abs(g["stats"]))
    # the rule of I/utils.py:501 at the class's own quantile: the rows from the quantile's rank up pass
    for cl in range(4):
        scores = g["score"][g["pred"] == cl]
        assert got["counts"][1 + cl, R.C_ACCEPTED] == int((scores >= g["tau_hat"][cl]).sum())


@pytest.mark.parametrize("teacher_disagreement", [False, True])
def test_validate_store_without_ranking_is_the_parents_and_with_it_gains_three_keys(teacher_disagreement):
    model, store = _model(), _store("f32")
    base = E.validate_store(model, store, teacher_disagreement=teacher_disagreement)
    off = E.validate_store(model, store, teacher_disagreement=teacher_disagreement, ranking=False)
    on = E.validate_store(model, store, teacher_disagreement=teacher_disagreement, ranking=True)
    assert sorted(off) == sorted(base)
    assert sorted(on) == sorted(list(base) + ["auroc_ovr_macro", "aurc", "confidence_stats"])
    for k, v in base.items():
        for r in (off, on):
            if k == "confusion_matrix":
                np.testing.assert_array_equal(r[k], v)
            else:
                assert r[k] == v, k
    full = E.certainty_ranking_store(model, store)
    assert on["auroc_ovr_macro"] == full["ovr"]["auroc_macro"] and on["aurc"] == full["selective"]["overall"]["aurc"]
    assert on["confidence_stats"] == full["confidence_stats"]


def test_validate_store_without_ranking_allocates_nothing_for_it():
    lab = _store("f32")
    store = lab.subset(np.arange(len(lab)))
    E.validate_store(_model(), store)
    assert "_rank" not in E.EvalPlan.of(store).__dict__
    E.validate_store(_model(), store, ranking=True)
    assert "_rank" in E.EvalPlan.of(store).__dict__


def test_reports_are_in_the_house_format():
    model, store = _model(), _store("f32")
    other = PKG.SSRLModel().cuda()
    with torch.no_grad():
        other.student_flat.copy_(model.teacher_flat)
        other.teacher_flat.copy_(model.student_flat)
    thr = [0.05, 0.1, 0.02, 0.2]
    fw = E.firewall_report(model, store, thr, initial_model=other)
    assert set(fw) == {"initial_weights", "trained_weights", "improvement", "gate"}
    for g in fw["gate"]:
        assert g["passed"] == g["passed_right"] + g["passed_wrong"]
        assert g["passed"] + g["blocked_right"] + g["blocked_wrong"] == g["members"]
    assert sum(g["members"] for g in fw["gate"]) == 37
    flat = lambda d: [x for v in d.values() for x in (v if isinstance(v, list) else [v])]
    assert all(type(x) is float for blk in ("initial_weights", "trained_weights", "improvement") for x in flat(fw[blk]))
    assert fw["improvement"]["leak_change"] == fw["trained_weights"]["leak"] - fw["initial_weights"]["leak"]
    same = E.firewall_report(model, store, thr)
    assert all(v == 0.0 for v in same["improvement"].values())
    rel = E.reliability_report(other, model, store, store)
    assert set(rel) == {"initial_weights", "trained_weights", "improvement"}
    assert all(type(x) is float for blk in rel.values() for x in blk.values())
    assert rel["trained_weights"]["clean_aurc"] == rel["trained_weights"]["noisy_aurc"]
