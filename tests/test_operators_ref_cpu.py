"""The conditions that keep tests/test_gpu_helper_ops.py and tests/test_gpu_encoder_ops.py honest, each checked on the
references of tests/operators_ref.py alone (no GPU): the inputs reach the branches the cases are named for, the discrete
outputs are decided far from their thresholds, the encoder operands are exact, and every bound or tolerance the GPU
modules apply rejects a wrong answer (one class skipped, a quantile one rank off, the last maximum, a pooled length
that counts padding, ReLU' bits past an utterance's end)."""
import numpy as np
import pytest
import torch

import exact_problem as X
import gpu_harness as gh
import operators_ref as R
from oracle import dad_oracle


def _rejects(fn, *a, **k):
    try:
        fn(*a, **k)
    except AssertionError:
        return True
    return False


# ------------------------------------------------------------------------------------- prediction head
@pytest.mark.parametrize("B", R.HEAD_B)
def test_head_rows_are_decided_and_bounds_reject_wrong_answers(B):
    e, W2, b2 = R.head_case(B)
    assert np.array_equal(e * 2.0 ** 10, np.round(e * 2.0 ** 10)) and e.min() >= 0
    ref = R.head_reference(e, W2, b2)
    print("B=%d: smallest top-two gap / 2 eps_z %.3g, largest logit bound %.3g" % (
        B, (ref["gap"] / (2 * ref["eps_z"])).min(), ref["z_lim"].max()))
    assert ref["decided"].all()
    # an fp32 evaluation in another order lies inside both bounds
    z32 = (e[:, ::-1] @ W2[:, ::-1].T + b2).astype(np.float32)
    assert R.worst(z32 - ref["z"], ref["z_lim"]) <= 1.0
    p32 = torch.softmax(torch.from_numpy(z32), 1).numpy()
    assert R.worst(p32 - ref["p"], ref["p_lim"]) <= 1.0
    # wrong answers: a bias left out, a softmax without the max's class, the score without the + 1e-8's partner
    assert R.worst(ref["z"] - b2.astype(np.float64) - ref["z"], ref["z_lim"]) > 10.0
    p_bad = dad_oracle.softmax(ref["z"] * (1.0 + 1e-3))
    assert R.worst(p_bad - ref["p"], ref["p_lim"]) > 1.0
    s_bad = ref["p"].max(1) * (1.0 - (-(ref["p"] * np.log(ref["p"] + 1e-8)).sum(1)) / np.log2(R.C))     # ln for log2
    assert R.worst(s_bad - ref["score"][True], R.score_lim(ref["score"][True])) > 10.0
    assert R.worst(ref["score"][False] - ref["score"][True], R.score_lim(ref["score"][True])) > 10.0


def test_head_tie_cases_tell_first_from_last_maximum():
    e, W2, b2 = R.head_case(37, "tie")
    lo, hi = R.tie_pair(W2, b2)
    ref, last = R.head_reference(e, W2, b2), R.head_reference(e, W2, b2, last_max=True)
    assert np.array_equal(ref["z"][:, lo], ref["z"][:, hi])
    tied = ref["pred"] == lo
    print("tie: classes %d and %d, %d of 37 rows have the tied pair on top" % (lo, hi, tied.sum()))
    assert tied.sum() >= 5 and np.all(last["pred"][tied] == hi) and not (ref["pred"] == hi).any()
    e, W2, b2 = R.head_case(5, "all_tie")
    assert np.all(R.head_reference(e, W2, b2)["pred"] == 0)
    assert np.all(R.head_reference(e, W2, b2, last_max=True)["pred"] == 3)


def test_head_wide_case_underflows_fp32_probabilities():
    e, W2, b2 = R.head_case(37, "wide")
    ref = R.head_reference(e, W2, b2)
    assert 70.0 <= np.abs(ref["z"]).max() <= 90.0
    under = ref["p"] < 2.0 ** -150                  # below half the smallest fp32 subnormal
    print("wide: logits in [%.1f, %.1f], %d of %d probabilities underflow" % (
        ref["z"].min(), ref["z"].max(), under.sum(), under.size))
    assert under.sum() >= 3
    assert np.all(np.isfinite(ref["score"][True])) and np.all(ref["score"][True] >= 0)


# ------------------------------------------------------------------------------------- certainty scores
@pytest.mark.parametrize("B", R.CERT_B)
def test_certainty_cases_hold_the_special_rows(B):
    p = R.certainty_case(B)
    assert p.shape == (B, 4) and p.dtype == np.float32
    s, pred = dad_oracle.certainty_scores(p, True)
    assert np.all(np.isfinite(s))
    for row, want, slot in zip(R.SPECIAL_ROWS, R.SPECIAL_PRED, R.special_slots(B)):
        assert np.array_equal(p[slot], row) and pred[slot] == want
    s1, p1 = dad_oracle.certainty_scores(R.SPECIAL_ROWS, True)
    assert tuple(p1) == R.SPECIAL_PRED
    assert abs(s1[0] - 1.0) < 1e-6 and abs(s1[1]) < 1e-6            # one-hot: 1; uniform: 0
    # last-maximum argmax differs on the tie rows; the max-prob score is rejected as the entropy score
    assert 3 - R.SPECIAL_ROWS[:, ::-1].argmax(1)[2] == 2
    assert _rejects(gh.close, dad_oracle.certainty_scores(p, False)[0], s, R.CERT_TOL, "no entropy")


# ------------------------------------------------------------------------------------------------ DACP
@pytest.mark.parametrize("case", R.DACP_CASES, ids=R.dacp_id)
def test_dacp_decisions_are_robust(case):
    Bn, kind, _ = case
    probs = R.dacp_case(case)[0]
    top = np.sort(probs, axis=1)
    assert (top[:, -1] - top[:, -2]).min() > R.DACP_TOP2
    calls, st = R.dacp_reference(case)
    margins = [np.abs(c["score"].astype(np.float64) - c["tau"].astype(np.float64)[c["pred"]]).min() for c in calls]
    counts = np.bincount(calls[0]["pred"], minlength=4)
    print("%s: margins %s, class counts %s, mask %d/%d" % (R.dacp_id(case), ["%.3f" % m for m in margins], counts,
                                                            calls[0]["mask"].sum(), Bn))
    assert min(margins) >= R.DACP_MARGIN
    if kind == "empty":
        assert counts[2] == 0 and min(counts[[0, 1, 3]]) > 0
    if kind == "single":
        assert counts[2] == 1
    if kind == "one_class":
        assert counts[1] == Bn
    if R.dacp_id(case) in R.DACP_OVER_512:
        assert counts.max() > 512                   # one class's sorted scores pass index 512
    if kind == "mixed" and Bn >= 5:
        assert calls[0]["mask"].min() == 0 and calls[0]["mask"].max() == 1 and counts.min() > 0
    assert np.array_equal(calls[1]["counts"], 2 * calls[0]["counts"])       # two calls accumulate


@pytest.mark.parametrize("case", [c for c in R.DACP_CASES if c[0] >= 64], ids=R.dacp_id)
def test_dacp_tolerance_rejects_wrong_thresholds(case, monkeypatch):
    calls, _ = R.dacp_reference(case, calls=1)
    want = calls[0]

    def off_by_one(values, q):
        v = np.sort(np.asarray(values, np.float32))
        return v[min(int(np.float32(q) * np.float32(len(v) - 1)) + 1, len(v) - 1)]
    monkeypatch.setattr(dad_oracle, "quantile_linear", off_by_one)
    bad = R.dacp_reference(case, calls=1)[0][0]
    assert _rejects(gh.close, bad["tau"], want["tau"], 1e-6, "quantile one rank up")
    monkeypatch.undo()
    if case[1] == "empty":
        # an empty class must still blend its old threshold (adjusted and floored) into the EMA
        tau0 = R.dacp_case(case)[1]
        kept = want["tau"].copy()
        kept[2] = tau0[2]
        assert _rejects(gh.close, kept, want["tau"], 1e-6, "empty class left unchanged")
    # the last row of the largest class left out of the sums and counts: the sums' tolerance catches it up to 512 rows
    # (past that one score can lie below 1e-6 of a sum), the counts, compared for equality, at every size
    c = int(np.argmax(want["counts"]))
    row = np.nonzero(want["pred"] == c)[0][-1]
    s, n = want["sums"].copy(), want["counts"].copy()
    s[c] -= float(want["score"][row])
    n[c] -= 1
    if case[0] <= 512:
        assert _rejects(gh.close, s, want["sums"], 1e-6, "one score missing from the sums")
    assert _rejects(np.testing.assert_array_equal, n.astype(np.float32), want["counts"].astype(np.float32))


def test_dacp_epoch_end_keeps_an_empty_class():
    case = [c for c in R.DACP_CASES if c[1] == "empty"][0]
    _, st = R.dacp_reference(case)
    Q0 = st.Q.copy()
    st.epoch_end(R.cfg()["DACP_QUALITY_SMOOTHING_BETA"])
    assert abs(st.Q[2] - Q0[2]) < 1e-6 and np.abs(st.Q[[0, 1, 3]] - Q0[[0, 1, 3]]).min() > 1e-3


# ------------------------------------------------------------------------------------------------ ECDA
@pytest.mark.parametrize("name", sorted(R.ECDA_CASES))
def test_ecda_cases_reach_their_branches(name):
    t, k = R.ECDA_CASES[name], R.ecda_case(name)
    assert k["B"] == sum(t["clean"]) and k["Bn"] == sum(t["inn"]) + sum(t["out"])
    assert R.ecda_branches(k) == t["expect"], R.ecda_branches(k)
    assert len(k["w"]) == (4 if t["w"] == "dacp" else k["Bn"])
    m = R.ecda_bool_mask(k)
    assert [int(((k["pred"] == c) & m).sum()) for c in range(4)] == t["inn"]
    if t.get("float_mask"):
        thr = np.float32(R.cfg()["FIXED_CONFIDENCE_THRESHOLD"])
        assert k["mask"].dtype == np.float32 and (k["mask"] == thr).sum() == 1 and not m[k["mask"] == thr].any()
        assert torch.equal(torch.from_numpy(k["mask"]) > R.cfg()["FIXED_CONFIDENCE_THRESHOLD"], torch.from_numpy(m))
    members = max(a + b for a, b in zip(t["clean"], t["inn"]))
    if False in t["aware"]:
        members = max(members, k["B"] + sum(t["inn"]))
    assert members <= 240                                    # the oracle's [n, n, H] float64 temporary
    for aware in t["aware"]:
        loss, gc, gn = R.ecda_reference(name, aware)
        assert np.isfinite(loss) and np.all(np.isfinite(gc)) and np.all(np.isfinite(gn))
        if aware:
            gated, cent = t["expect"]["gated"], t["expect"]["cent"]
            assert (loss != 0.0) == bool(gated)
            # exactly the member rows carry a gradient: clean rows of a gated class; noisy members of a gated class,
            # and of every class with a centroid when a gated class's repulsion term has two centroids to push apart
            touched_c = np.isin(k["yc"], gated)
            rep = bool(gated) and len(cent) > 1
            touched_n = m & np.isin(k["pred"], sorted(set(gated) | (set(cent) if rep else set())))
        else:
            on = k["B"] >= 2 and m.sum() >= 2
            assert (loss != 0.0) == on
            touched_c, touched_n = np.full(k["B"], on), m & on
        assert np.array_equal(np.any(gc != 0, axis=1), touched_c)
        assert np.array_equal(np.any(gn != 0, axis=1), touched_n)


def test_ecda_named_branches():
    assert R.ecda_reference("B1_Bn1", True)[0] == 0.0 and R.ecda_reference("B1_Bn1", False)[0] == 0.0
    loss, gc, gn = R.ecda_reference("ones_Bn2_class3", True)
    assert loss == 0.0 and not gc.any() and not gn.any()
    assert R.ecda_reference("ones_Bn2_class3", False)[0] != 0.0        # (the global MMD has no class loop to cut short)
    # over range(4) the same case is NOT zero: the zero comes from range(len(w)) alone
    k = R.ecda_case("ones_Bn2_class3")
    full = dad_oracle.ecda_loss(k["clean"], k["noisy"], k["yc"], k["pred"], k["mask"], k["scores"].astype(np.float64),
                                np.ones(4, np.float32), R.cfg(), True, False)
    assert full[0] != 0.0
    # ones(4): reading the weights as DACP's [4] or as ones(Bn) is one formula in the reference (unit attention)
    k = R.ecda_case("ones_Bn4")
    w = np.asarray(k["w"], np.float64)
    assert len(w) == 4 and np.all(np.exp(R.cfg()["ECDA_CLASS_ATTENTION_LAMBDA"] * (w.mean() - w)) == 1.0)
    # one valid class: no repulsion, so the other classes' noisy rows stay untouched
    k = R.ecda_case("one_valid_class")
    gn = R.ecda_reference("one_valid_class", True)[2]
    assert not gn[k["pred"] != 0].any()


@pytest.mark.parametrize("name", ["B5_Bn7", "pre_82_members", "ones_Bn9", "float_mask"])
def test_ecda_tolerances_reject_a_skipped_class(name):
    loss, gc, gn = R.ecda_reference(name, True)
    cls = R.ECDA_CASES[name]["expect"]["gated"][-1]
    l2, gc2, gn2 = R.ecda_reference(name, True, drop_class=cls)
    print("%s: class %d skipped moves the loss by %.3g" % (name, cls, l2 - loss))
    assert not R.ecda_loss_ok(l2, loss)
    assert _rejects(gh.close_grad, gc2, gc, "d/d clean") and _rejects(gh.close_grad, gn2, gn, "d/d noisy")


# --------------------------------------------------------------------------------------------- encoder
ALL_GEOMS = R.ENC_GEOMS + [R.limit_geom()]


@pytest.mark.parametrize("geom", ALL_GEOMS, ids=R.enc_id)
def test_encoder_operands_are_exact(geom):
    k = R.encoder_case(geom)
    B, T = k["B"], k["T"]
    assert k["x"].shape == (B, T, R.D) and np.abs(k["x"]).max() < 17
    for what, a, step in (("x", k["x"], 2.0 ** -3), ("W1", k["W1"], 2.0 ** -10), ("de", k["de"], 2.0 ** -6)):
        t = torch.from_numpy(np.ascontiguousarray(a))
        assert t.dtype == torch.float32 and np.array_equal(a / step, np.round(a / step)), what
        if what != "de":
            assert torch.equal(t.half().float(), t) and torch.equal(t.bfloat16().float(), t), what
    assert np.abs(k["de"]).max() <= 4 and np.all(np.abs(k["b1"] * 2.0 ** 14) % 2 == 1)
    if k["pad"].any() and B < 1024:
        assert np.abs(k["x"][k["pad"]]).max() > 0                # padded frames hold values, not zeros
    ref = R.encoder_reference(k)
    x2 = k["x"].reshape(B * T, R.D)
    got = x2 @ k["W1"].T + k["b1"]
    assert got.dtype == np.float32 and np.array_equal(got.astype(np.float64), ref["pre"].reshape(B * T, -1))
    perm = np.random.RandomState(0).permutation(R.D)
    got_p = np.ascontiguousarray(x2[:, perm]) @ np.ascontiguousarray(k["W1"][:, perm]).T + k["b1"]
    assert np.array_equal(got_p.astype(np.float64), ref["pre"].reshape(B * T, -1))
    assert np.all(ref["pre"] != 0)
    mag = np.abs(x2).astype(np.float64) @ np.abs(k["W1"]).astype(np.float64).T + np.abs(k["b1"]).astype(np.float64)
    assert mag.max() < 1024
    # the oracle's own fp32 forward and weight gradient lie inside the bounds
    e32, act32, vlen32 = dad_oracle.encoder_forward(k["x"], k["pad"], k["W1"], k["b1"])
    assert np.array_equal(act32, ref["act"])
    assert R.enc_forward_ratio(e32, ref, T) <= 1.0
    if B < 1024:
        dW32, db32 = dad_oracle.encoder_wgrad(k["x"], act32, vlen32, k["de"])
        rW, rb = R.enc_backward_ratios(dW32, db32, ref, B, T)
        print("%s: oracle fp32 wgrad / bound: dW1 %.3g, db1 %.3g" % (R.enc_id(geom), rW, rb))
        assert rW <= 1.0 and rb <= 1.0


@pytest.mark.parametrize("geom", ALL_GEOMS, ids=R.enc_id)
def test_encoder_geometry_holds_its_edges(geom):
    k = R.encoder_case(geom)
    ref = R.encoder_reference(k)
    lens, T = k["lens"], k["T"]
    for b in np.nonzero(lens == 0)[0]:
        assert not ref["e"][b].any() and not ref["act"][b].any()
    dead = ref["S_W1"].max(1) == 0
    print("%s: %d of 256 rows of dW1 are exactly zero" % (R.enc_id(geom), dead.sum()))
    if lens.sum() <= 2:
        assert dead.sum() > 0
    if max(lens) == 0:
        assert dead.all() and not ref["dW1"].any()
    if 3 <= len(lens) < 1024:
        assert (lens == 0).any() and (lens == T).any() and ((lens % R.SLAB != 0) & (lens < T) & (lens > 0)).any()


@pytest.mark.parametrize("geom", [g for g in R.ENC_GEOMS if len(g[1]) >= 3], ids=R.enc_id)
def test_encoder_bounds_reject_wrong_answers(geom):
    k = R.encoder_case(geom)
    B, T = k["B"], k["T"]
    ref = R.encoder_reference(k)
    r = R.enc_forward_ratio(R.encoder_reference(k, lens_with_padding=True)["e"], ref, T)
    print("%s: pooled length with padding: %.3g x the forward bound" % (R.enc_id(geom), r))
    assert r >= 10.0
    bad = R.encoder_reference(k, act=R.act_whole_last_slab(k))
    rW, rb = R.enc_backward_ratios(bad["dW1"], bad["db1"], ref, B, T)
    print("%s: ReLU' bits to the end of the last slab: %.3g / %.3g x the backward bound" % (R.enc_id(geom), rW, rb))
    assert rW >= 10.0 and rb >= 10.0
    # de rounded to bf16 instead of kept in fp32; one utterance's scale taken with len + 1
    de16 = torch.from_numpy(k["de"] / np.float32(3.0)).bfloat16().float().numpy() * np.float32(3.0)
    r16 = R.enc_backward_ratios(*[X.wgrad64(k["x"], ref["act"], ref["vlen"], de16)[i] for i in (0, 2)], ref, B, T)
    assert min(r16) >= 10.0
    lens1 = ref["vlen"].copy()
    lens1[int(np.argmax(lens1))] += 1
    r1 = R.enc_backward_ratios(*[X.wgrad64(k["x"], ref["act"], ref["vlen"], k["de"], lens=lens1)[i] for i in (0, 2)],
                               ref, B, T)
    assert min(r1) >= 10.0


# -------------------------------------------------------------------------------------------- augment
@pytest.mark.parametrize("shape", R.AUG_SHAPES, ids=str)
def test_augment_cases_draw_valid_starts(shape):
    B, T, Dd = shape
    x, nw, ns, u, start = R.augment_case(shape)
    c = R.cfg()
    mlen = int(T * c["TEMPORAL_MASK_RATIO"])
    assert np.all(start >= 0) and np.all(start + mlen <= T)
    st = dad_oracle.strong_augment(x, ns, u, start, c["STRONG_NOISE_STD"], c["DROPOUT_RATE"], c["TEMPORAL_MASK_RATIO"])
    if mlen > 0:
        for b in range(B):
            assert not st[b, start[b]:start[b] + mlen].any()
    if Dd >= 7 and shape != (3, 5, 7):
        assert 0 < (u > np.float32(c["DROPOUT_RATE"])).sum() < Dd       # the feature mask drops and keeps
    assert (B * T * Dd) % 2 == (1 if shape in ((1, 1, 1), (3, 5, 7)) else 0)
