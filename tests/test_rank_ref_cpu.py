"""tests/rank_ref.py (the NumPy restatement of dad_rank_metrics) held to outside yardsticks -- scikit-learn's
roc_auc_score and average_precision_score, torch.quantile, NumPy's moments, the reference's own numbers in
tests/golden/eval_rank.npz -- the wrong-answer controls against the GPU tests' case list, and the host-only parts of
the entry points: dad_rank_plan, dad_rank_workspace_bytes, every error decided before a launch, the DAD_RK_* defines."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest
import torch

import dadpkg
import rank_cases
import rank_ref as R

sys.path.insert(0, os.path.join(dadpkg.ROOT, "tests", "golden"))
from gen_rank_golden import probs_of  # noqa: E402

PKG = dadpkg.pkg()
L = PKG._lib
P = ctypes.c_void_p(256)        # never dereferenced: every call it goes to fails its checks first
TOL = 4 * R.U
GOLDEN = os.path.join(dadpkg.ROOT, "tests", "golden", "eval_rank.npz")


@pytest.fixture(scope="module", autouse=True)
def _built():
    PKG.build(verbose=False)


def _seeded(n, levels, seed):
    rs = np.random.RandomState(seed)
    key = rs.random_sample(n).astype(np.float32)
    if levels:
        key = (np.floor(key * levels) / levels).astype(np.float32)
    y = rs.random_sample(n) < 0.35
    y[:2] = (True, False)
    return key, y


@pytest.mark.parametrize("levels", [0, 3, 7], ids=["continuous", "levels3", "levels7"])
@pytest.mark.parametrize("n", [65, 1100])
def test_auroc_and_ap_are_scikit_learns(n, levels):
    from sklearn.metrics import average_precision_score, roc_auc_score
    key, y = _seeded(n, levels, 90 + n + levels)
    c = R.column(key, np.where(y, 3, 1).astype(np.uint8))
    Pn, Nn = int(y.sum()), int((~y).sum())
    auc = c["counts"][R.C_U2] / (2 * Pn * Nn)
    d_auc = abs(auc - roc_auc_score(y, key.astype(np.float64)))
    d_ap = abs(c["values"][R.V_AP] - average_precision_score(y, key.astype(np.float64)))
    print("n %d levels %d: |auroc - sklearn| %.3e  |ap - sklearn| %.3e" % (n, levels, d_auc, d_ap))
    assert c["values"][R.V_AUROC] == auc and d_auc <= TOL and d_ap <= TOL


@pytest.mark.parametrize("n", [65, 1100])
def test_macro_ovr_auroc_is_scikit_learns(n):
    from sklearn.metrics import roc_auc_score
    rs = np.random.RandomState(300 + n)
    probs = probs_of(300 + n, n)
    y = rs.randint(0, 4, n)
    score = probs.max(axis=1)
    key, flags = R.eval_columns(score, probs, probs.argmax(axis=1), y)
    ref = R.rank_metrics(key, flags)
    macro = float(np.mean(ref["values"][6:10, R.V_AUROC]))
    p64 = probs.astype(np.float64)
    want = roc_auc_score(y, p64, multi_class="ovr")       # (the float32 rows sum to 1 within its tolerance)
    per = [roc_auc_score(y == c, p64[:, c]) for c in range(4)]
    assert np.abs(ref["values"][6:10, R.V_AUROC] - per).max() <= TOL
    assert abs(macro - want) <= TOL


@pytest.mark.parametrize("n", [1, 2, 5, 64, 1100])
def test_quantile_is_torch_quantile_bit_for_bit(n):
    key = np.random.RandomState(500 + n).random_sample(n).astype(np.float32)
    gammas = (0.0, 0.4, 0.5, 0.613, 0.8, 1.0)
    got = R.column(key, np.ones(n, np.uint8), gammas=gammas)["quant"]
    want = torch.quantile(torch.from_numpy(key), torch.tensor(gammas, dtype=torch.float32)).numpy()
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (got, want)


@pytest.mark.parametrize("n", [65, 1100])
def test_moments_are_numpys(n):
    key, _ = _seeded(n, 0, 700 + n)
    v = R.column(key, np.ones(n, np.uint8))["values"]
    k = key.astype(np.float64)
    assert v[R.V_KEY_MEAN] == np.mean(k) and abs(v[R.V_KEY_STD] - np.std(k)) <= TOL * np.std(k)
    assert v[R.V_KEY_MIN] == np.min(k) and v[R.V_KEY_MAX] == np.max(k)


def test_golden_fixture_of_the_reference():
    g = np.load(GOLDEN)
    n = int(g["n"])
    probs = probs_of(int(g["seed"]), n)
    score, pred = g["score"], g["pred"]
    # the reference's scores are the product's own formula (I/utils.py:412-423) on these probabilities
    assert np.array_equal(pred, probs.argmax(axis=1))
    key, flags = R.eval_columns(score, probs, pred, None)
    ref = R.rank_metrics(key, flags, gammas=(float(g["gamma"]),))
    assert np.array_equal(ref["order"][0], g["rank"])                       # the scores' ranks
    assert np.array_equal(ref["quant"][1:5, 0].view(np.uint32), g["tau_hat"].view(np.uint32))
    v = ref["values"][5]
    got = np.array([v[R.V_KEY_MEAN], v[R.V_KEY_STD], v[R.V_KEY_MIN], v[R.V_KEY_MAX]])
    assert np.all(np.abs(got - g["stats"]) <= TOL * np.abs(g["stats"])), (got, g["stats"])
    assert ref["counts"][1:5, R.C_MEMBERS].tolist() == np.bincount(pred, minlength=4).tolist()


@pytest.mark.parametrize("variant", R.WRONG)
def test_each_wrong_answer_fails_a_case_of_the_gpu_list(variant):
    failing = []
    for i in range(len(rank_cases.SHAPES)):
        c = rank_cases.case(i)
        wrong = R.rank_metrics(c["key"], c["flags"], c["thr"], c["gammas"], c["bins"], c["bin_range"], variant)
        bad, _ = rank_cases.compare(wrong, rank_cases.reference(i))
        if bad:
            failing.append((c["name"], bad))
    print(variant, failing)
    assert failing, variant


def test_the_case_list_covers_what_it_promises():
    seen, thr_kinds, qs, bs = set(), set(), set(), set()
    for i, (n, m) in enumerate(rank_cases.SHAPES):
        c = rank_cases.case(i)
        ref = rank_cases.reference(i)
        assert rank_cases.compare(ref, ref) == ([], 0.0)
        qs.add(len(c["gammas"]))
        bs.add(c["bins"])
        for j in range(m):
            pattern = rank_cases.PATTERNS[(i + j) % len(rank_cases.PATTERNS)]
            if n >= 63:
                seen.add(pattern)
            M = ref["counts"][j, R.C_MEMBERS]
            if M > 1:
                a = ref["counts"][j, R.C_ACCEPTED]
                thr_kinds.add("nan" if np.isnan(c["thr"][j]) else "none" if a == 0 else "all" if a == M else "some")
    assert seen == set(rank_cases.PATTERNS) and thr_kinds == {"nan", "none", "all", "some"}
    assert qs == {0, 8} and bs == {0, 1, 64}
    assert {m for _, m in rank_cases.SHAPES} == {1, 10, 16}


# ---------------------------------------------------------------- the host-only parts of the entry points
@pytest.mark.parametrize("m", [1, 10, 16])
@pytest.mark.parametrize("n,cus", [(1, 256), (257, 256), (1100, 256), (5531, 256), (5531, 8), (65536, 256), (65536, 304)])
def test_plan_covers_every_key_tile_once(n, cus, m):
    fn = L.require("dad_rank_plan", "the plan")
    rt, ch, per = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    assert fn(n, m, cus, ctypes.byref(rt), ctypes.byref(ch), ctypes.byref(per)) == 0
    assert rt.value == -(-n // L.RK_TILE)
    assert 1 <= ch.value <= min(rt.value, L.RK_MAX_CHUNKS)
    assert (ch.value - 1) * per.value < rt.value <= ch.value * per.value        # every tile once, no empty chunk
    # chunks only while the grid is short of four workgroups a compute unit
    assert ch.value == 1 or rt.value * m * (ch.value - 1) < 4 * cus


def test_plan_and_workspace_refuse_what_the_calls_refuse():
    fn = L.require("dad_rank_plan", "the plan")
    ws = L.require("dad_rank_workspace_bytes", "the test")
    v = [ctypes.c_int() for _ in range(3)]
    for n, m, cus in ((0, 1, 256), (L.RK_MAX_N + 1, 1, 256), (100, 0, 256), (100, L.RK_MAX_M + 1, 256), (100, 1, 0)):
        assert fn(n, m, cus, *v) == L.E_SHAPE
        assert cus == 0 or ws(n, m) == 0
    assert fn(100, 1, 256, None, v[1], v[2]) == L.E_ARG
    assert 0 < ws(1, 1) < ws(257, 1) < ws(257, 10) < ws(1100, 10) < ws(L.RK_MAX_N, L.RK_MAX_M)
    for n, m in ((1, 1), (1100, 10), (L.RK_MAX_N, L.RK_MAX_M)):
        parts = 4 * min(-(-n // L.RK_TILE), L.RK_MAX_CHUNKS) * n * m       # the chunks' counts
        assert parts < ws(n, m) <= parts + 14 * n * m + 6 * 256 and ws(n, m) % 256 == 0


def _args(**kw):
    a = L.DadRankArgs()
    for name in ("key", "flags", "thr", "gammas", "counts", "values", "quant", "bin_counts", "bin_sum"):
        setattr(a, name, 256)
    a.n, a.m, a.Q, a.B, a.bin_lo, a.bin_hi = 100, 2, 2, 4, 0.0, 1.0
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def test_argument_errors_come_before_any_launch():
    for name, tail in (("dad_rank_metrics", ()), ("dad_rank_metrics_chunked", (3,))):
        fn = L.require(name, "the test")
        call = lambda ws=P, **kw: fn(_args(**kw), *tail, ws, None)
        assert fn(None, *tail, P, None) == L.E_ARG and call(ws=None) == L.E_ARG
        for ptr in ("key", "flags", "thr", "counts", "values", "gammas", "quant", "bin_counts", "bin_sum"):
            assert call(**{ptr: None}) == L.E_ARG, ptr
        for kw in (dict(bin_lo=1.0, bin_hi=1.0), dict(bin_lo=2.0), dict(bin_hi=float("inf")), dict(bin_lo=float("nan"))):
            assert call(**kw) == L.E_ARG, kw
        for kw in (dict(n=0), dict(n=L.RK_MAX_N + 1), dict(m=0), dict(m=L.RK_MAX_M + 1), dict(Q=-1),
                   dict(Q=L.RK_MAX_Q + 1), dict(B=-1), dict(B=L.RK_MAX_BINS + 1)):
            assert call(**kw) == L.E_SHAPE, kw
    fn = L.require("dad_rank_eval_columns", "the test")
    for i in (0, 1, 2, 5, 6):
        a = [P, P, P, None, 4, P, P, None]
        a[i] = None
        assert fn(*a) == L.E_ARG
    for n in (0, -1, L.RK_MAX_N + 1):
        assert fn(P, P, P, None, n, P, P, None) == L.E_SHAPE


def test_header_defines_equal_the_binding_and_the_struct_has_the_c_layout(tmp_path):
    import subprocess
    hdr = open(os.path.join(dadpkg.ROOT, "include", "dad.h")).read()
    defs = {k: int(v) for k, v in re.findall(r"^#define DAD_RK_([A-Z0-9_]+) (\d+)", hdr, flags=re.M)}
    assert len(defs) == 26
    for k, v in defs.items():
        assert getattr(L, "RK_" + k) == v, k
    assert (R.N_COUNTS, R.N_VALUES, R.MEMBER, R.POSITIVE) == (L.RK_COUNTS, L.RK_VALUES, L.RK_MEMBER, L.RK_POSITIVE)
    for k in ("MEMBERS", "POSITIVES", "NONFINITE", "RUNS", "U2", "ACCEPTED", "ACCEPTED_POS", "VALID_AUROC"):
        assert getattr(R, "C_" + k) == defs[k]
    for k in ("AUROC", "AP", "AURC", "KEY_MEAN", "KEY_STD", "KEY_MIN", "KEY_MAX"):
        assert getattr(R, "V_" + k) == defs[k]
    assert "#define DAD_ABI_VERSION 10" in hdr
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "dad.h"', "int main(void){",
             'printf("size %zu\\n", sizeof(dad_rank_args));']
    lines += ['printf("%s %%zu\\n", offsetof(dad_rank_args, %s));' % (f[0], f[0]) for f in L.DadRankArgs._fields_]
    (tmp_path / "probe.c").write_text("\n".join(lines + ["return 0;}"]))
    subprocess.check_call(["gcc", "-I", os.path.join(dadpkg.ROOT, "include"), str(tmp_path / "probe.c"), "-o",
                           str(tmp_path / "probe")])
    out = dict(l.split() for l in subprocess.check_output([str(tmp_path / "probe")]).decode().splitlines())
    assert int(out["size"]) == ctypes.sizeof(L.DadRankArgs)
    for f in L.DadRankArgs._fields_:
        assert int(out[f[0]]) == getattr(L.DadRankArgs, f[0]).offset, f[0]


def test_the_package_exports_the_surface():
    E = PKG.evaluate
    for name in ("rank_metrics", "risk_coverage", "roc_points", "enqueue_certainty_ranking", "certainty_ranking_store",
                 "firewall_report", "reliability_report"):
        assert getattr(PKG, name) is getattr(E, name) and name in PKG.__all__
