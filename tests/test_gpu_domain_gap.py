"""The clean-noisy domain gap on the MI355X (evaluate.domain_gap* + csrc/domain_gap.hip) against the fixture of the
reference's ECDALoss (tests/golden/eval_domain_gap.npz) and the float64 restatement tests/domain_gap_ref.py (computed
once per input on the CPU): the fixture cases, the tile edges and the chunked summation, the smallest inputs,
degenerate classes, poison and padding, permuted rows, the store path and graph capture.

The bounds come from the fixture, never from the kernel: a term, a bandwidth (relative) and the total may deviate
from float64 by 4 x the worst deviation of the reference's own float32 run from its float64 run over the three
fixture cases (the kernel's fp32 errors -- the Gram form on centred rows, v_exp_f32, another summation order -- are of
that size; the same inputs' float32 Gram-form CPU restatement stays within 1 x, tests/test_domain_gap_ref_cpu.py).
An mmd is (ss + tt) - 2 st of the kernel's own doubles, exactly, so it may deviate by 4 term bounds.  Centroids,
compactness, shift and repulsion are double arithmetic on the fp32 inputs: bounded relative to the restatement by
(m 256 + 8) 2^-53 max|x| / rms|x - centroid| of the input.

The bounds: term 1.484e-6, bandwidth 3.969e-7 relative, total 2.348e-6.  Worst |kernel - float64| measured on the
MI355X per input (the worst of 1 chunk, 3 chunks and the planner's count; profiles/domain_gap.json):
term / bandwidth relative / total / double quantities relative
  fixture 37 + 29    2.46e-7  1.32e-7  1.42e-7  4.4e-16      fixture 65 + 64    2.55e-7  1.31e-7  2.96e-7  2.2e-16
  fixture 129 + 140  2.96e-7  4.37e-8  2.09e-7  3.3e-16      n = 127            2.36e-7  1.60e-7  4.87e-8  5.6e-16
  n = 128            1.13e-7  1.44e-7  2.03e-7  4.4e-16      n = 129            2.65e-7  1.02e-7  4.15e-7  3.3e-16
  n = 257            1.89e-7  6.58e-8  1.74e-7  4.4e-16      2 + 2              8.39e-8  7.94e-8  2.39e-7  1.1e-15
  one repeated vector 9.65e-8 5.77e-8  2.32e-7  2.2e-16      zero noisy weights 9.23e-8  1.45e-7  1.17e-9  2.2e-16
  permuted (n = 129) 2.18e-7  9.67e-8  1.49e-7  3.3e-16
so the kernel errs like the reference's own float32 run (3.7e-7, 9.9e-8, 5.9e-7), a fifth to two fifths of the bounds.
"""
import functools
import os
import warnings

import numpy as np
import pytest
import torch

import dadpkg
import gpu_harness as gh
from domain_gap_ref import domain_gap_ref
from oracle import data_oracle as do

pytestmark = pytest.mark.gpu
PKG = dadpkg.pkg()
D = PKG.data
E = PKG.evaluate
L = PKG._lib
T = L.DG_TILE
GOLDEN = os.path.join(dadpkg.ROOT, "tests", "golden", "eval_domain_gap.npz")
CASES = (37, 65, 129)          # n_clean of the fixture cases
TERMS = ("term_ss", "term_tt", "term_st")


@functools.lru_cache(None)
def _fixture():
    return np.load(GOLDEN)


@functools.lru_cache(None)
def _bounds():
    """(term, relative bandwidth, total): 4 x the fixture's own float32-against-float64 deviation."""
    g = _fixture()
    term = bw = total = 0.0
    for nc in CASES:
        k = "c%d_" % nc
        term = max(term, np.abs(g[k + "f32_class_terms"] - g[k + "f64_class_terms"]).max(),
                   np.abs(g[k + "f32_global_terms"] - g[k + "f64_global_terms"]).max())
        b64 = np.append(g[k + "f64_class_bw"], g[k + "f64_global_bw"])
        b32 = np.append(g[k + "f32_class_bw"], g[k + "f32_global_bw"])
        bw = max(bw, np.abs(b32[b64 > 0] / b64[b64 > 0] - 1.0).max())
        total = max(total, abs(float(g[k + "f32_total"]) - float(g[k + "f64_total"])))
    assert 1e-7 < term < 1e-6 and 1e-8 < bw < 1e-6 and 1e-7 < total < 2e-6      # (the issue's figures)
    return 4 * float(term), 4 * float(bw), 4 * float(total)


def _synthetic(nc, nn, seed):
    """Two domains by the fixture's recipe: labels in [0, 4), two noisy rows labelled -1, noisy weights in [0.3, 1]."""
    rs = np.random.RandomState(seed)
    lc, ln = rs.randint(0, 4, nc).astype(np.int64), rs.randint(0, 4, nn).astype(np.int64)
    if nn > 8:
        ln[rs.permutation(nn)[:2]] = -1
    offsets, shift = 0.08 * rs.standard_normal((4, 256)), 0.03 * rs.standard_normal((4, 256))
    ec = (0.5 + 0.1 * np.abs(rs.standard_normal((nc, 256))) + offsets[lc]).astype(np.float32)
    k = np.maximum(ln, 0)
    en = (0.5 + 0.13 * np.abs(rs.standard_normal((nn, 256))) + offsets[k] + shift[k]).astype(np.float32)
    return {"emb_clean": ec, "labels_clean": lc, "emb_noisy": en, "labels_noisy": ln,
            "weights_noisy": rs.uniform(0.3, 1.0, nn).astype(np.float32),
            "class_weights": rs.uniform(0.5, 1.5, 4).astype(np.float32)}


def _flat(c):
    """(emb, labels, domain, weights) of both domains, clean rows first."""
    nc, nn = len(c["labels_clean"]), len(c["labels_noisy"])
    wn = c.get("weights_noisy")
    return (np.concatenate([c["emb_clean"], c["emb_noisy"]]), np.concatenate([c["labels_clean"], c["labels_noisy"]]),
            np.concatenate([np.zeros(nc, np.uint8), np.ones(nn, np.uint8)]),
            np.concatenate([np.ones(nc, np.float32), np.ones(nn, np.float32) if wn is None else wn]))


def _ref(c):
    emb, labels, domain, weights = _flat(c)
    return domain_gap_ref(emb, labels, domain, weights, c.get("class_weights"), 1.0, 0.1, 0.1)


@functools.lru_cache(None)
def _case(name):
    """(inputs, domain_gap_ref of them); computed once, never modified."""
    if name in CASES:
        g, key = _fixture(), "c%d_" % name
        c = {k[len(key):]: g[k] for k in g.files if k.startswith(key)}
        assert (float(g["lam"]), float(g["gamma"]), float(g["delta"])) == (1.0, 0.1, 0.1)    # the IEMOCAP defaults
    else:
        c = _synthetic(*name)
    return c, _ref(c)


def _run(c, chunks=0):
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    return E.domain_gap(dev(c["emb_clean"]), c["labels_clean"], dev(c["emb_noisy"]), c["labels_noisy"],
                        c.get("weights_noisy"), c.get("class_weights"), _chunks=chunks)


def _double_bound(c):
    emb, labels, domain, _ = _flat(c)
    x = emb.astype(np.float64)
    part = (labels >= 0) & (labels < 4)
    res = []
    for g in range(8):
        rows = part & (labels == g >> 1) & (domain == (g & 1))
        if rows.any():
            res.append(x[rows] - x[rows].mean(0))
    rms = np.sqrt(np.mean(np.concatenate(res) ** 2))
    return (int(part.sum()) * 256 + 8) * 2.0 ** -53 * np.abs(x[part]).max() / rms


def _errors(r, ref):
    p, q = r["per_class"], ref["per_class"]
    rel = lambda a, b: abs(a / b - 1.0) if b else abs(a)
    e = {"term": max(max(abs(a - b) for k in TERMS for a, b in zip(p[k], q[k])),
                     max(abs(r["global"][k] - ref["global"][k]) for k in TERMS)),
         "bw": max(max(rel(a, b) for a, b in zip(p["bandwidth"], q["bandwidth"])),
                   rel(r["global"]["bandwidth"], ref["global"]["bandwidth"])),
         "mmd": max(max(abs(a - b) for a, b in zip(p["mmd"], q["mmd"])), abs(r["global"]["mmd"] - ref["global"]["mmd"]),
                    abs(r["mmd_class_mean"] - ref["mmd_class_mean"])),
         "total": abs(r["ecda_loss"] - ref["ecda_loss"]),
         "double": max(max(rel(a, b) for k in ("compactness", "centroid_shift", "weight_noisy", "attention")
                           for a, b in zip(p[k], q[k])), rel(r["repulsion"], ref["repulsion"]))}
    return e


def _check(r, ref, c, what=""):
    term_b, bw_b, total_b = _bounds()
    e = _errors(r, ref)
    dbl = _double_bound(c)
    print("%s: |kernel - float64|: term %.3e (bound %.3e)  bandwidth rel %.3e (%.3e)  mmd %.3e  total %.3e (%.3e)  "
          "double rel %.3e (%.3e)" % (what, e["term"], term_b, e["bw"], bw_b, e["mmd"], e["total"], total_b,
                                      e["double"], dbl))
    assert r["valid"] == ref["valid"] and r["n_clean"] == ref["n_clean"] and r["n_noisy"] == ref["n_noisy"]
    assert r["nonfinite"] == 0 and r["global"]["gate"] == ref["global"]["gate"]
    for k in ("gate", "n_clean", "n_noisy"):
        assert r["per_class"][k] == ref["per_class"][k], k
    assert e["term"] <= term_b and e["bw"] <= bw_b and e["mmd"] <= 4 * term_b and e["total"] <= total_b, e
    assert e["double"] <= dbl, e
    # mmd is (ss + tt) - 2 st of the kernel's own doubles, exactly; a closed gate leaves zeros
    for s in [r["global"]] + [{k: v[k2] for k, v in r["per_class"].items()} for k2 in range(4)]:
        assert s["mmd"] == (s["term_ss"] + s["term_tt"]) - 2.0 * s["term_st"]
        if not s["gate"]:
            assert s["bandwidth"] == s["term_ss"] == s["term_tt"] == s["term_st"] == s["mmd"] == 0.0
            assert s.get("compactness", 0.0) == 0.0 and s.get("centroid_shift", 0.0) == 0.0
    p = r["per_class"]
    own = sum(p["attention"][k] * ((p["mmd"][k] + 0.1 * p["compactness"][k]) + 0.1 * r["repulsion"])
              for k in range(4) if p["gate"][k])
    assert abs(own - r["ecda_loss"]) <= 8 * 2.0 ** -53 * max(1.0, abs(own))
    return e


def _same_bits(a, b):
    return a["block"].tobytes() == b["block"].tobytes()


# ---------------------------------------------------------------- 1. the fixture cases
@pytest.mark.parametrize("nc", CASES)
def test_fixture_cases(nc):
    c, ref = _case(nc)
    r = _run(c)
    _check(r, ref, c, "fixture %d + %d" % (nc, len(c["labels_noisy"])))
    term_b, bw_b, total_b = _bounds()
    p, single = r["per_class"], int(c["single"])
    got = np.array([p[k] for k in TERMS]).T
    gt = np.array([r["global"][k] for k in TERMS])
    bw = np.array(p["bandwidth"] + [r["global"]["bandwidth"]])
    for tag in ("f64", "f32"):     # float64: the bound itself; the reference's float32 run is 1/4 bound further away
        slack = 1.0 if tag == "f64" else 1.25
        assert np.abs(got - c[tag + "_class_terms"]).max() <= slack * term_b
        assert np.abs(gt - c[tag + "_global_terms"]).max() <= slack * term_b
        want = np.append(c[tag + "_class_bw"], c[tag + "_global_bw"])
        assert np.abs(bw[want > 0] / want[want > 0] - 1.0).max() <= slack * bw_b and not bw[want == 0].any()
        assert abs(r["ecda_loss"] - float(c[tag + "_total"])) <= slack * total_b
    assert p["gate"] == [k != single for k in range(4)] and p["n_noisy"][single] == 1
    assert r["n_clean"] == nc and r["n_noisy"] == len(c["labels_noisy"]) - 2 and r["valid"]


# ---------------------------------------------------------------- 2. tile edges, chunked summation
# 2T - 1, 2T, 2T + 1 rows, half per domain: the domain boundary lies inside a tile, at 2T on one; 4T + 1 rows in 3
# chunks of 2 column tiles leave the last chunk one single column
@pytest.mark.parametrize("n", [2 * T - 1, 2 * T, 2 * T + 1, 4 * T + 1])
def test_tile_edges_and_chunks(n):
    c, ref = _case((n // 2, n - n // 2, 500 + n))
    runs = {}
    for chunks in (1, 3):
        a, b = _run(c, chunks), _run(c, chunks)
        _check(a, ref, c, "n=%d chunks=%d" % (n, chunks))
        assert _same_bits(a, b), chunks
        runs[chunks] = a
    a, b = _run(c), _run(c)
    _check(a, ref, c, "n=%d planned" % n)
    assert _same_bits(a, b)
    # the chunking moves fp32 row sums only: counts, weights, centroid quantities are the same bits
    for k in ("compactness", "centroid_shift", "weight_noisy", "attention", "n_clean", "n_noisy"):
        assert runs[1]["per_class"][k] == runs[3]["per_class"][k], k
    assert runs[1]["repulsion"] == runs[3]["repulsion"]


def test_single_column_chunk_really_is_one():
    """The geometry test 2 relies on, from the host plan's own rule."""
    n, want = 4 * T + 1, 3
    rt = -(-n // T)
    per = -(-rt // want)
    chunks = -(-rt // per)
    assert (rt, per, chunks) == (5, 2, 3) and n - T * per * (chunks - 1) == 1


# ---------------------------------------------------------------- 3. the smallest inputs
def test_two_plus_two_rows_open_the_gate():
    c = _synthetic(2, 2, 61)
    c["labels_clean"][:] = 3
    c["labels_noisy"][:] = 3
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        r = _run(c)
    _check(r, _ref(c), c, "2 + 2")
    assert r["valid"] and r["per_class"]["gate"] == [False, False, False, True] and r["repulsion"] == 0.0


def test_one_plus_three_rows_close_everything():
    c = _synthetic(1, 3, 62)
    c["labels_clean"][:] = 1
    c["labels_noisy"][:] = 1
    with pytest.warns(RuntimeWarning, match="every term is 0.0"):
        r = _run(c)
    assert r["valid"] is False and r["n_clean"] == 1 and r["n_noisy"] == 3
    assert r["ecda_loss"] == 0.0 and r["mmd_class_mean"] == 0.0 and r["repulsion"] == 0.0
    kept = set([L.DG_N_SRC, L.DG_N_TGT] + [s + k for s in (L.DG_C_N_SRC, L.DG_C_N_TGT, L.DG_C_W_TGT, L.DG_C_ATTENTION)
                                           for k in range(4)])
    assert not any(r["block"][s] for s in range(L.DG_SLOTS) if s not in kept)
    assert r["per_class"]["n_clean"] == [0, 1, 0, 0] and r["per_class"]["n_noisy"] == [0, 3, 0, 0]


# ---------------------------------------------------------------- 4. degenerate classes
def test_a_class_of_one_repeated_vector_has_bandwidth_zero():
    """Class 2's rows in both domains are one vector: every distance inside the class must be exactly 0 (the norms are
    the diagonal of the walk's own Gram block), so its bandwidth is 0, every kernel value 5 and every term
    5 W / (W + 1e-8); a distance of 1e-7 instead would give exp(-10) under the coefficient 1 / 1e-8."""
    c = dict(_case((70, 75, 71))[0])
    for k in ("emb_clean", "emb_noisy", "weights_noisy"):
        c[k] = c[k].copy()
    v = c["emb_clean"][np.where(c["labels_clean"] == 2)[0][0]].copy()
    c["emb_clean"][c["labels_clean"] == 2] = v
    c["emb_noisy"][c["labels_noisy"] == 2] = v
    rows = np.where(c["labels_noisy"] == 2)[0]
    c["weights_noisy"][rows] = np.array([0.5, 0.25, 0.75, 1.0], np.float32)[np.arange(len(rows)) % 4]
    r = _run(c)
    _check(r, _ref(c), c, "one repeated vector")
    p = r["per_class"]
    ws, wt = float(p["n_clean"][2]), float(c["weights_noisy"][rows].astype(np.float64).sum())
    assert p["gate"][2] and p["bandwidth"][2] == 0.0 and p["compactness"][2] == 0.0 and p["centroid_shift"][2] == 0.0
    for k, w in (("term_ss", ws * ws), ("term_tt", wt * wt), ("term_st", ws * wt)):
        assert p[k][2] == 5.0 * w / (w + 1e-8), k
    assert all(p["bandwidth"][k] > 0 for k in (0, 1, 3)) and r["global"]["bandwidth"] > 0


def test_a_class_of_zero_noisy_weights():
    c0, _ = _case((70, 75, 71))
    c = dict(c0)
    c["weights_noisy"] = c0["weights_noisy"].copy()
    c["weights_noisy"][c["labels_noisy"] == 1] = 0.0
    base, r = _run(c0), _run(c)
    _check(r, _ref(c), c, "zero noisy weights")
    p = r["per_class"]
    assert p["gate"][1] and p["term_tt"][1] == 0.0 and p["term_st"][1] == 0.0 and p["weight_noisy"][1] == 0.0
    assert p["term_ss"][1] == base["per_class"]["term_ss"][1] and p["mmd"][1] == p["term_ss"][1]
    assert p["bandwidth"] == base["per_class"]["bandwidth"] and r["global"] == base["global"]


# ---------------------------------------------------------------- 5. poison and padding
def test_nan_in_rows_that_take_no_part_changes_no_bit():
    c0, _ = _case(65)
    want = _run(c0)
    c = dict(c0)
    c["emb_noisy"] = c0["emb_noisy"].copy()
    out = np.where(c["labels_noisy"] < 0)[0]
    c["emb_noisy"][out[0]] = np.nan
    c["emb_noisy"][out[1], ::2] = np.inf
    c["emb_noisy"][out[1], 1::2] = -np.inf
    assert _same_bits(_run(c), want)


def test_poison_past_row_n_changes_no_bit():
    c, _ = _case(37)
    want = _run(c)
    emb, labels, domain, weights = _flat(c)
    n = len(labels)
    big = torch.full((n + 2 * T, 256), float("nan"), device="cuda")
    big[:n] = torch.from_numpy(emb).cuda()
    lab = torch.full((n + 2 * T,), 1, dtype=torch.int64, device="cuda")
    lab[:n] = torch.from_numpy(labels).cuda()
    dom = torch.ones(n + 2 * T, dtype=torch.uint8, device="cuda")
    dom[:n] = torch.from_numpy(domain).cuda()
    w = torch.full((n + 2 * T,), float("nan"), device="cuda")
    w[:n] = torch.from_numpy(weights).cuda()
    block = torch.empty(L.DG_SLOTS, dtype=torch.float64, device="cuda")
    E._enqueue_domain_gap(big[:n], lab[:n], dom[:n], w[:n], E._domain_gap_args(c["class_weights"], None), block,
                          E._domain_gap_workspace(n, big.device))
    assert block.cpu().numpy().tobytes() == want["block"].tobytes()
    assert torch.isnan(big[n:]).all()


def test_nan_in_a_participating_row_raises_with_the_count():
    c0, _ = _case(65)
    c = dict(c0)
    c["emb_clean"], c["emb_noisy"] = c0["emb_clean"].copy(), c0["emb_noisy"].copy()
    c["emb_clean"][11, 17] = np.nan
    c["emb_noisy"][np.where(c["labels_noisy"] >= 0)[0][40], 255] = np.inf
    with pytest.raises(L.DadError, match="2 of %d participating row" % (65 + 64 - 2)):
        _run(c)


def test_arguments_are_checked_before_any_launch():
    x = torch.zeros(5, 256, device="cuda")
    with pytest.raises(ValueError, match=r"labels_clean must be \[5\]"):
        E.domain_gap(x, [0, 1], x, [0] * 5)
    with pytest.raises(ValueError, match=r"weights_noisy must be \[5\]"):
        E.domain_gap(x, [0] * 5, x, [0] * 5, weights_noisy=[1.0])
    with pytest.raises(ValueError, match="65536"):
        E.domain_gap(x[:1].expand(40000, 256), [0] * 40000, x[:1].expand(30000, 256), [0] * 30000)


# ---------------------------------------------------------------- 6. permuted, interleaved rows through the ABI
def test_permuted_rows_stay_within_the_bounds():
    c, ref = _case((T, T + 1, 500 + 2 * T + 1))
    base = _run(c)
    emb, labels, domain, weights = _flat(c)
    perm = np.random.RandomState(81).permutation(len(labels))
    assert len(set(np.diff(domain[perm].astype(int)).tolist())) == 3          # the domains interleave
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a[perm])).cuda()
    block = torch.empty(L.DG_SLOTS, dtype=torch.float64, device="cuda")
    E._enqueue_domain_gap(dev(emb), dev(labels), dev(domain), dev(weights),
                          E._domain_gap_args(c["class_weights"], None), block,
                          E._domain_gap_workspace(len(labels), block.device))
    r = E._domain_gap_result(block.cpu().numpy())
    _check(r, ref, c, "permuted")
    e = _errors(r, {k: base[k] for k in ref})
    term_b, bw_b, total_b = _bounds()
    assert e["term"] <= term_b and e["bw"] <= bw_b and e["total"] <= total_b and e["double"] <= _double_bound(c)


# ---------------------------------------------------------------- 7. the store path
@functools.lru_cache(None)
def _model(seed=11):
    stu, tea = do.eval_weights(seed)
    model = PKG.SSRLModel().cuda()
    with torch.no_grad():
        model.student_flat.copy_(torch.from_numpy(gh.flat(stu)))
        model.teacher_flat.copy_(torch.from_numpy(gh.flat(tea)))
    return model


@functools.lru_cache(None)
def _store(kind):
    """Two small synthetic stores of different sizes: 'clean' 33 utterances, 'noisy' 41 (two labelled -1)."""
    seed, count = {"clean": (21, 33), "noisy": (31, 41)}[kind]
    rs = np.random.RandomState(seed)
    sizes = np.concatenate([[1, 31, 32, 33, 64, 65], rs.randint(1, 71, count - 6)])
    labels = rs.randint(0, 4, count)
    if kind == "noisy":
        labels[[4, 17]] = -1
    offsets = np.concatenate([[0], np.cumsum(sizes)[:-1]])
    feats = rs.standard_normal((int(sizes.sum()), 768)).astype(np.float32)
    return D.FeatureStore(feats, sizes, offsets, labels.astype(np.int64))


def test_store_path_with_true_labels_equals_the_two_step_path():
    model, clean, noisy = _model(), _store("clean"), _store("noisy")
    got = E.domain_gap_store(model, clean, noisy)
    want = E.domain_gap(E.embed_store(model, clean), clean.labels, E.embed_store(model, noisy), noisy.labels)
    assert got["valid"] and got["n_clean"] == 33 and got["n_noisy"] == 39
    assert _same_bits(got, want)
    plan = E.EvalPlan.of(noisy)
    bufs = plan._dg[33]
    ptrs = {k: v.data_ptr() for k, v in bufs.items()}
    again = E.domain_gap_store(model, clean, noisy)
    assert plan._dg[33] is bufs and len(plan._dg) == 1 and {k: v.data_ptr() for k, v in bufs.items()} == ptrs
    assert _same_bits(again, got)
    assert not hasattr(E.EvalPlan.of(clean), "_dg")          # (cached on the noisy split's plan alone)


def test_store_path_with_the_teacher_equals_the_two_step_path():
    model, clean, noisy = _model(), _store("clean"), _store("noisy")
    ev = E.evaluate_store(model, noisy, use_teacher=True, outputs=("t_pred", "t_logits"))
    score, _ = PKG.DACPManager.calculate_certainty_scores(torch.softmax(ev["t_logits"], dim=1))
    pred = ev["t_pred"]
    thr = torch.sort(score).values[len(score) // 3].repeat(4) + torch.tensor([0.0, 0.01, -0.01, 0.0], device="cuda")
    labels = torch.where(score > thr[pred], pred, torch.full_like(pred, -1))
    assert 0 < int((labels < 0).sum()) < len(labels)
    cw = [0.7, 1.2, 0.9, 1.4]
    emb_c, emb_n = E.embed_store(model, clean), E.embed_store(model, noisy)
    got = E.domain_gap_store(model, clean, noisy, assign="teacher", thresholds=thr, class_weights=cw)
    want = E.domain_gap(emb_c, clean.labels, emb_n, labels, weights_noisy=score, class_weights=cw)
    assert got["n_noisy"] == int((labels >= 0).sum()) and _same_bits(got, want)
    free = E.domain_gap_store(model, clean, noisy, assign="teacher", class_weights=cw)
    assert free["n_noisy"] == 41 and _same_bits(free, E.domain_gap(emb_c, clean.labels, emb_n, pred, score, cw))
    with pytest.raises(ValueError, match="assign"):
        E.domain_gap_store(model, clean, noisy, assign="student")


def test_alignment_report_of_two_models():
    model, clean, noisy = _model(), _store("clean"), _store("noisy")
    other = PKG.SSRLModel().cuda()
    with torch.no_grad():
        other.student_flat.copy_(model.teacher_flat)
        other.teacher_flat.copy_(model.teacher_flat)
    rep = E.alignment_report(model, other, clean, noisy)
    a, b = E.domain_gap_store(model, clean, noisy), E.domain_gap_store(other, clean, noisy)
    assert rep == E.alignment_from_gaps(a, b)
    assert rep["initial_weights"]["ecda_loss"] == a["ecda_loss"] and rep["trained_weights"]["mmd_global"] == b["global"]["mmd"]
    for k in ("mmd_global", "mmd_class_mean", "ecda_loss"):
        assert rep["improvement"][k + "_change"] == rep["trained_weights"][k] - rep["initial_weights"][k]


# ---------------------------------------------------------------- 8. graph capture; nothing new without the calls
def test_captured_enqueue_replays_like_eager():
    model, clean, noisy = _model(), _store("clean"), _store("noisy")
    cp, np_ = E.EvalPlan.of(clean), E.EvalPlan.of(noisy)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        want = E.domain_gap_store(model, clean, noisy, assign="teacher")      # (lazy buffers, then the eager block)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        bufs = E.enqueue_domain_gap_store(model, cp, np_, assign="teacher")
    for _ in range(2):
        bufs["block_d"].fill_(-1.0)
        g.replay()
        torch.cuda.synchronize()
        assert bufs["block_d"].cpu().numpy().tobytes() == want["block"].tobytes()


def test_validate_store_is_untouched_by_the_new_calls():
    model = _model()
    sizes = np.array([5, 40, 64, 7, 33, 12])
    feats = np.random.RandomState(91).standard_normal((int(sizes.sum()), 768)).astype(np.float32)
    fresh = D.FeatureStore(feats, sizes, np.concatenate([[0], np.cumsum(sizes)[:-1]]), np.array([0, 1, 2, 3, 1, 0]))
    before = E.validate_store(model, fresh, teacher_disagreement=True, cluster_metrics=True)
    assert not hasattr(E.EvalPlan.of(fresh), "_dg")           # no domain-gap buffer, workspace or launch
    E.domain_gap_store(model, _store("clean"), fresh)
    after = E.validate_store(model, fresh, teacher_disagreement=True, cluster_metrics=True)
    assert sorted(before) == sorted(after)
    for k, v in before.items():
        if k == "confusion_matrix":
            np.testing.assert_array_equal(after[k], v)
        else:
            assert after[k] == v, k
