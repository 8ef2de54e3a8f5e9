"""The clean-noisy domain gap without a GPU: the float64 restatement (tests/domain_gap_ref.py) against the fixture of
the reference's ECDALoss (tests/golden/eval_domain_gap.npz) and against oracle.dad_oracle.ecda_loss, what the fixture
promises, the report's arithmetic, the DAD_DG_* slots of header and binding, and the host-only queries."""
import ctypes
import os
import re

import numpy as np
import pytest

import dadpkg
from domain_gap_ref import domain_gap_ref, gaussian_terms_f32
from oracle import dad_oracle

PKG = dadpkg.pkg()
E = PKG.evaluate
L = PKG._lib
GOLDEN = os.path.join(dadpkg.ROOT, "tests", "golden", "eval_domain_gap.npz")
CASES = ((37, 29), (65, 64), (129, 140))
TILE = L.DG_TILE      # (the binding's DAD_DG_* mirror: every test of this file needs the feature)


def load_case(nc):
    g = np.load(GOLDEN)
    key = "c%d_" % nc
    c = {k[len(key):]: g[k] for k in g.files if k.startswith(key)}
    c.update(lam=float(g["lam"]), gamma=float(g["gamma"]), delta=float(g["delta"]))
    return c


def ref_of(c):
    nc, nn = len(c["labels_clean"]), len(c["labels_noisy"])
    return domain_gap_ref(np.concatenate([c["emb_clean"], c["emb_noisy"]]),
                          np.concatenate([c["labels_clean"], c["labels_noisy"]]),
                          np.concatenate([np.zeros(nc, np.uint8), np.ones(nn, np.uint8)]),
                          np.concatenate([np.ones(nc, np.float32), c["weights_noisy"]]), c["class_weights"],
                          c["lam"], c["gamma"], c["delta"])


@pytest.mark.parametrize("nc,nn", CASES)
def test_restatement_reproduces_the_reference_in_float64(nc, nn):
    c = load_case(nc)
    assert c["emb_clean"].shape == (nc, 256) and c["emb_noisy"].shape == (nn, 256)
    assert c["emb_clean"].dtype == c["emb_noisy"].dtype == c["weights_noisy"].dtype == np.float32
    r = ref_of(c)
    # the fixture holds what the issue asks of it
    single = int(c["single"])
    assert sorted(set(c["labels_clean"].tolist())) == [0, 1, 2, 3]
    assert int((c["labels_noisy"] == single).sum()) == 1 and int((c["labels_noisy"] == -1).sum()) == 2
    assert r["per_class"]["gate"] == [k != single for k in range(4)] and r["global"]["gate"] and r["valid"]
    assert r["n_clean"] == nc and r["n_noisy"] == nn - 2
    i, j = c["dup"]
    assert c["labels_clean"][i] == c["labels_noisy"][j] >= 0 and np.array_equal(c["emb_clean"][i], c["emb_noisy"][j])
    assert 0.3 <= c["weights_noisy"].min() and c["weights_noisy"].max() <= 1.0
    assert 0.5 <= c["class_weights"].min() and c["class_weights"].max() <= 1.5
    assert not c["f64_class_terms"][single].any() and c["f64_class_bw"][single] == 0.0
    p = r["per_class"]
    got = np.array([p["term_ss"], p["term_tt"], p["term_st"]]).T
    e_term = max(np.abs(got - c["f64_class_terms"]).max(),
                 np.abs(np.array([r["global"][k] for k in ("term_ss", "term_tt", "term_st")]) - c["f64_global_terms"]).max())
    bw, bw_ref = np.array(p["bandwidth"] + [r["global"]["bandwidth"]]), np.append(c["f64_class_bw"], c["f64_global_bw"])
    open_ = bw_ref > 0
    e_bw = np.abs(bw[open_] / bw_ref[open_] - 1).max()
    e_total = abs(r["ecda_loss"] - float(c["f64_total"]))
    print("%d + %d: restatement - reference float64: term %.2e  bandwidth rel %.2e  total %.2e" % (nc, nn, e_term, e_bw, e_total))
    assert e_term <= 1e-12 and e_bw <= 1e-12 and e_total <= 1e-12 and not bw[~open_].any()
    assert p["compactness"][single] == 0.0 and p["centroid_shift"][single] == 0.0 and r["repulsion"] < 0
    # what rounding does to the reference itself: the figures the GPU test's bounds are built from
    dev = max(np.abs(c["f32_class_terms"] - c["f64_class_terms"]).max(), np.abs(c["f32_global_terms"] - c["f64_global_terms"]).max())
    assert 0 < dev < 1e-6 and abs(float(c["f32_total"]) - float(c["f64_total"])) < 2e-6


def test_restatement_reproduces_the_oracle_loss():
    c = load_case(37)
    r = ref_of(c)
    cfg = {"ECDA_CLASS_ATTENTION_LAMBDA": c["lam"], "ECDA_COMPACTNESS_WEIGHT_GAMMA": c["gamma"],
           "ECDA_REPULSION_WEIGHT_DELTA": c["delta"], "FIXED_CONFIDENCE_THRESHOLD": 0.9}
    total, _, _ = dad_oracle.ecda_loss(c["emb_clean"], c["emb_noisy"], c["labels_clean"], c["labels_noisy"],
                                       c["labels_noisy"] >= 0, c["weights_noisy"].astype(np.float64),
                                       c["class_weights"].astype(np.float64), cfg, True, False)
    assert abs(total - r["ecda_loss"]) <= 1e-12
    # the global term is the oracle's (and the reference's) USE_CLASS_AWARE_MMD = False branch
    g, _, _ = dad_oracle.ecda_loss(c["emb_clean"], c["emb_noisy"], c["labels_clean"], c["labels_noisy"],
                                   c["labels_noisy"] >= 0, c["weights_noisy"].astype(np.float64),
                                   c["class_weights"].astype(np.float64), cfg, False, False)
    assert abs(g - r["global"]["mmd"]) <= 1e-12


def test_gram_form_float32_restatement_stays_near_the_reference():
    """The device's form of the arithmetic on the CPU (centred Gram-form float32 distances, float32 coefficients and
    exponentials) deviates from the reference's float64 like the reference's own float32 does."""
    worst = ref_dev = 0.0
    for nc, _ in CASES:
        c = load_case(nc)
        keep = c["labels_noisy"] >= 0
        both = np.concatenate([c["emb_clean"], c["emb_noisy"][keep]]).astype(np.float64)
        mu = both.mean(0).astype(np.float32)
        t = gaussian_terms_f32(c["emb_clean"], c["emb_noisy"][keep], np.ones(nc, np.float32),
                               np.ones(int(keep.sum()), np.float32), mu)
        np.testing.assert_array_equal(np.array(t[:3]), c["gram32_terms"][4])
        worst = max(worst, np.abs(c["gram32_terms"][4] - c["f64_global_terms"]).max(),
                    np.abs(c["gram32_terms"][:4] - c["f64_class_terms"]).max())
        ref_dev = max(ref_dev, np.abs(c["f32_class_terms"] - c["f64_class_terms"]).max(),
                      np.abs(c["f32_global_terms"] - c["f64_global_terms"]).max())
    print("gram32 - float64 %.2e, reference float32 - float64 %.2e" % (worst, ref_dev))
    assert worst <= 4 * ref_dev


def test_closed_gates_and_the_smallest_sets():
    x = np.random.RandomState(3).rand(4, 256).astype(np.float32)
    r = domain_gap_ref(x, [1, 1, 1, 1], [0, 0, 1, 1])                 # 2 + 2 rows of one class
    assert r["valid"] and r["per_class"]["gate"] == [False, True, False, False] and r["global"]["gate"]
    assert r["repulsion"] == 0.0 and r["per_class"]["term_ss"][1] > 0
    assert r["global"]["mmd"] == pytest.approx(r["per_class"]["mmd"][1], abs=1e-15)
    r = domain_gap_ref(x, [1, 1, 1, 1], [0, 1, 1, 1])                 # 1 + 3
    assert not r["valid"] and r["ecda_loss"] == 0.0 and not any(r["per_class"]["mmd"])
    assert not any(r["per_class"]["compactness"]) and r["global"]["mmd"] == 0.0
    r = domain_gap_ref(x, [0, 0, 7, -1], [0, 0, 1, 1])                # the noisy rows take no part
    assert not r["valid"] and r["n_clean"] == 2 and r["n_noisy"] == 0


def test_alignment_report_arithmetic():
    a = {"global": {"mmd": 0.5}, "mmd_class_mean": 0.25, "ecda_loss": 1.5}
    b = {"global": {"mmd": 0.125}, "mmd_class_mean": np.float64(0.0625), "ecda_loss": 0.75}
    r = E.alignment_from_gaps(a, b)
    assert r["initial_weights"] == {"mmd_global": 0.5, "mmd_class_mean": 0.25, "ecda_loss": 1.5}
    assert r["trained_weights"] == {"mmd_global": 0.125, "mmd_class_mean": 0.0625, "ecda_loss": 0.75}
    assert r["improvement"] == {"mmd_global_change": -0.375, "mmd_class_mean_change": -0.1875,
                                "ecda_loss_change": -0.75, "mmd_global_percentage": -75.0}
    for block in r.values():
        assert all(type(v) is float for v in block.values())
    z = E.alignment_from_gaps({"global": {"mmd": 0.0}, "mmd_class_mean": 0.0, "ecda_loss": 0.0}, b)
    assert z["improvement"]["mmd_global_percentage"] == 0.0


def test_header_slots_equal_the_binding():
    hdr = open(os.path.join(dadpkg.ROOT, "include", "dad.h")).read()
    defs = {k: int(v) for k, v in re.findall(r"^#define DAD_DG_([A-Z_]+) (\d+)", hdr, flags=re.M)}
    assert len(defs) == 29
    for k, v in defs.items():
        assert getattr(L, "DG_" + k) == v, k
    per_class = sorted(v for k, v in defs.items() if k.startswith("C_"))
    assert per_class == list(range(16, 64, 4)) and defs["SLOTS"] == 64
    scalars = sorted(v for k, v in defs.items() if not k.startswith("C_") and k not in ("SLOTS", "MAX_N", "TILE", "MAX_CHUNKS"))
    assert scalars == list(range(7)) + list(range(8, 14))
    assert defs["MAX_N"] == 65536 and defs["TILE"] == 64
    # the ctypes mirror of dad_domain_gap_args: float[4], then three doubles
    A = L.DadDomainGapArgs
    assert ctypes.sizeof(A) == 40 and A.lam.offset == 16 and A.gamma.offset == 24 and A.delta.offset == 32


@pytest.mark.parametrize("n,cus", [(1, 256), (66, 256), (2200, 256), (11062, 256), (11062, 8), (65536, 256), (65536, 304)])
def test_plan_covers_every_column_tile_once(n, cus):
    PKG.build(verbose=False)
    fn = L.require("dad_domain_gap_plan", "the plan")
    rt, ch, per = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    assert fn(n, cus, ctypes.byref(rt), ctypes.byref(ch), ctypes.byref(per)) == 0
    assert rt.value == -(-n // TILE)
    assert 1 <= ch.value <= min(rt.value, L.DG_MAX_CHUNKS)
    assert (ch.value - 1) * per.value < rt.value <= ch.value * per.value        # every tile once, no empty chunk
    ws = L.lib().dad_domain_gap_workspace_bytes
    assert ws(n) > 0 and ws(0) == 0 and ws(L.DG_MAX_N + 1) == 0
    assert ws(65536) < 2 ** 28           # the chunk partials dominate: 16 x 65,536 x 4 floats
    assert fn(0, cus, ctypes.byref(rt), ctypes.byref(ch), ctypes.byref(per)) == L.E_SHAPE
    assert fn(L.DG_MAX_N + 1, cus, ctypes.byref(rt), ctypes.byref(ch), ctypes.byref(per)) == L.E_SHAPE
    assert fn(n, cus, None, ctypes.byref(ch), ctypes.byref(per)) == L.E_ARG


def test_argument_errors_come_before_any_launch():
    PKG.build(verbose=False)
    fn = L.require("dad_domain_gap", "the test")
    p = ctypes.c_void_p(256)        # never dereferenced: every call below fails its checks first
    a = L.DadDomainGapArgs()
    good = [p, p, p, None, 4, a, p, p, None]
    for k in (0, 1, 2, 5, 6, 7):    # emb, labels, domain, args, out, workspace
        args = list(good)
        args[k] = None
        assert fn(*args) == L.E_ARG, k
    for n in (0, -3, 65537):
        assert fn(p, p, p, None, n, a, p, p, None) == L.E_SHAPE
    ch = L.require("dad_domain_gap_chunked", "the test")
    assert ch(p, p, p, None, 0, a, p, 3, p, None) == L.E_SHAPE and ch(None, p, p, None, 4, a, p, 3, p, None) == L.E_ARG
