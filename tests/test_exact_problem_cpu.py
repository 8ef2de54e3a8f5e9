"""The conditions that keep tests/test_gpu_exact_operands.py honest, each checked on the reference alone (no GPU):
the operands of tests/exact_problem.py are exact in fp16 and bf16, the pre-activations are exact in fp32 in any
summation order and never 0, the DACP / ECDA gates are open with the mask decisions far from their thresholds, the
strong branch is visible in the weight gradient, the fp32 references and a simulated 16-bit rounding of the
weight gradient's scales lie inside the derived bound, and wrong weight gradients lie at least 10x outside it.
The long problems (exact_problem.LONG_GEOMS, tests/test_gpu_long_utterances.py) meet the same conditions; their own
controls: every loud slab dropped or counted twice lies 10x outside the fp16 bound through its sentinel column, L3's 22
splits begin and end in loud slabs, and what csrc/pool.h's loops could get wrong past 16 slabs or 512 frames lies 10x
outside the embedding and db1 bounds."""
import numpy as np
import pytest
import torch

import exact_problem as X
from oracle import dad_oracle
from oracle.torch_cpu import TorchCPUStep

GEOMS = pytest.mark.parametrize("geom", X.GEOMS, ids=X.geom_id)
# the conditions every problem must meet: the edge geometries and the long ones (tests/test_gpu_long_utterances.py)
ALL = pytest.mark.parametrize("geom", X.GEOMS + X.LONG_GEOMS + [X.S1_PLUS], ids=X.geom_id)
SENTINEL = pytest.mark.parametrize("geom", [g for g in X.LONG_GEOMS if g.get("sentinel")], ids=X.geom_id)
POOLED = pytest.mark.parametrize("geom", [X.LONG["L1"], X.LONG["L2"]], ids=X.geom_id)
EPOCH = 60


def _encoder_operands(geom):
    """[(name, x [B,T,D], W1, b1)] of the three encoder passes of a post-warm-up step."""
    inp, st, _ = X.case(geom, EPOCH)
    xw, xs = X.augmented(inp, X.cfg())
    return [("clean", inp["xc"], st["student"][0], st["student"][1]),
            ("weak", xw, st["teacher"][0], st["teacher"][1]),
            ("strong", xs, st["student"][0], st["student"][1])]


@ALL
def test_operands_survive_fp16_and_bf16(geom):
    inp = X.case(geom, EPOCH)[0]
    assert np.abs(inp["xc"]).max() < 17 and np.abs(inp["xn"]).max() < 17
    for name, x, W1, _ in _encoder_operands(geom):
        for what, a in ((name + " x", x), (name + " W1", W1)):
            t = torch.from_numpy(np.ascontiguousarray(a))
            assert t.dtype == torch.float32
            assert torch.equal(t.half().float(), t), what + ": fp16"
            assert torch.equal(t.bfloat16().float(), t), what + ": bf16"


@ALL
def test_preactivations_are_exact_in_any_order_and_never_zero(geom):
    perm = np.random.RandomState(0).permutation(768)
    for name, x, W1, b1 in _encoder_operands(geom):
        B, T, D = x.shape
        x2 = x.reshape(B * T, D)
        want = X.preact64(x, W1, b1).reshape(B * T, -1)
        got = x2 @ W1.T + b1
        assert got.dtype == np.float32
        assert np.array_equal(got.astype(np.float64), want), name
        got_p = np.ascontiguousarray(x2[:, perm]) @ np.ascontiguousarray(W1[:, perm]).T + b1
        assert np.array_equal(got_p.astype(np.float64), want), name + " (columns permuted)"
        units = want * 2.0 ** 14
        assert np.array_equal(units, np.round(units)) and np.all(np.abs(units) % 2 == 1), name   # odd multiples of 2^-14
        assert np.all(want != 0), name
        mag = np.abs(x2).astype(np.float64) @ np.abs(W1).astype(np.float64).T + np.abs(b1).astype(np.float64)
        assert mag.max() < 1024, (name, mag.max())


@ALL
def test_gates_are_open_and_mask_decisions_are_robust(geom):
    r = X.case(geom, EPOCH)[2]["oracle"]
    mask = np.asarray(r["mask"])
    assert mask.sum() >= 2 and r["consistency_loss"] != 0.0, (mask.sum(), r["consistency_loss"])
    if geom["B"] >= 12:
        assert r["ecda_loss"] != 0.0
    if geom["Bn"] >= 16:
        assert mask.min() == 0 and mask.max() == 1, mask
    margin = np.abs(np.asarray(r["score"], np.float64) - np.asarray(r["tau_after"], np.float64)[r["pred"]]).min()
    print("%s: mask %d/%d, smallest |score - threshold| %.3g" % (X.geom_id(geom), mask.sum(), mask.size, margin))
    assert margin >= 1e-3, margin


@GEOMS
def test_strong_branch_is_visible_in_the_weight_gradient(geom):
    ref = X.case(geom, EPOCH)[2]
    share = np.linalg.norm(ref["strong"][1]) / np.linalg.norm(ref["S"][0])
    print("%s: strong share of |S_W1| %.3f" % (X.geom_id(geom), share))
    assert share >= 0.10, share


@GEOMS
def test_tail_term_stays_a_small_part_of_the_bound(geom):
    """The worst-case fp32 error of the classifier backward (exact_problem's tail term) matters where dL/de
    cancels; elsewhere the bound is (eps_op + n_rows u + 1e-4) S_W1 as before: at least half of the elements
    keep the fp16 bound within a factor of 20."""
    ref = X.case(geom, EPOCH)[2]
    S = ref["S"][0]
    rel = ref["tail"][S > 0] / S[S > 0]
    print("%s: tail term / S_W1 median %.3g, 90th percentile %.3g, max %.3g" % (
        X.geom_id(geom), np.median(rel), np.percentile(rel, 90), rel.max()))
    assert np.all(ref["tail"][S == 0] == 0)
    assert np.median(rel) <= 19 * X.bound("dW1", "fp16", ref["n_rows"])


def _torch_step(inp, st, epoch):
    """Plain fp32 autograd: (pre-clip gradients, outputs)."""
    c = dict(X.cfg(), GRADIENT_CLIPPING=False)      # (the step would scale .grad in place)
    t = TorchCPUStep(*st["student"], c)
    t.load_state(st)
    out = t.step(inp, epoch, draws=inp)
    grads = [p.grad.detach().numpy().copy() for p in t.student]
    return grads, {k: v.detach().numpy() for k, v in out.items() if torch.is_tensor(v)}


@pytest.mark.parametrize("epoch", [0, EPOCH])
@ALL
def test_fp32_references_lie_inside_the_fp32_bound(geom, epoch):
    inp, st, ref = X.case(geom, epoch)
    r = ref["oracle"]
    tg, tout = _torch_step(inp, st, epoch)
    if epoch >= 30:
        np.testing.assert_array_equal(tout["mask"], r["mask"])
    for who, grads, out in (("oracle", r["grads"], r), ("torch", tg, tout)):
        ratios = X.grad_ratios(grads, ref, "fp32")
        ratios.update(X.forward_ratios(out, {**ref, "e": {k: v for k, v in ref["e"].items() if k in out},
                                             "z": {k: v for k, v in ref["z"].items() if k in out}}))
        print("%s e%d %s: %s" % (X.geom_id(geom), epoch, who, {k: float("%.3g" % v) for k, v in ratios.items()}))
        assert max(ratios.values()) <= 1.0, (who, ratios)


def _scales(ref):
    """Per-(utterance, h) scales dL/de / len of the clean and strong rows, stacked [Bc + Bn, H]."""
    v = [p["g"] / np.maximum(p["vlen"], 1.0)[:, None] for p in (ref["parts"]["clean"], ref["parts"]["strong"])]
    return np.concatenate(v, 0)


def _round16(v, prec):
    """The weight gradient's rounding of the scales (csrc/wgrad_direct.h): bf16 directly; fp16 after the power of
    two that maps hidden unit h's largest |v| into [2^14, 2^15)."""
    if prec == "bf16":
        return torch.from_numpy(v.astype(np.float32)).bfloat16().double().numpy()
    mx = np.abs(v).max(0)
    s = 14 - np.floor(np.log2(np.where(mx > 0, mx, 1.0)))
    return np.float16(v * 2.0 ** s).astype(np.float64) / 2.0 ** s


def _dw1(ref, scale=None, clean=None, strong=None):
    """dW1 in float64 from the reference's parts; `scale`: stacked replacement scales; clean / strong: replacement
    fields of a branch (x, act, vlen)."""
    pc, ps = dict(ref["parts"]["clean"], **(clean or {})), dict(ref["parts"]["strong"], **(strong or {}))
    if scale is None:
        return X.wgrad64(**pc)[0] + X.wgrad64(**ps)[0]
    Bc = pc["x"].shape[0]
    return X.wgrad64_scaled(pc["x"], pc["act"], scale[:Bc])[0] + X.wgrad64_scaled(ps["x"], ps["act"], scale[Bc:])[0]


def _ratio(dw, ref, prec):
    return X.worst(dw - ref["grads"][0], X.grad_limit("dW1", prec, ref))


@ALL
def test_simulated_16bit_scale_rounding_lies_inside_the_bound(geom):
    ref = X.case(geom, EPOCH)[2]
    assert _ratio(_dw1(ref), ref, "fp32") < 1e-6                 # the rebuild itself
    for prec in ("fp16", "bf16"):
        r = _ratio(_dw1(ref, scale=_round16(_scales(ref), prec)), ref, prec)
        print("%s: simulated %s scales, worst err / bound %.3f" % (X.geom_id(geom), prec, r))
        assert r <= 1.0, (prec, r)


def _last_slab_off(part, u):
    """The branch's ReLU' pattern without the last 32-row slab of utterance u's frames."""
    n = int(part["vlen"][u])
    act = part["act"].copy()
    act[u, 32 * ((n - 1) // 32):n] = False
    return act


def _mutants(geom):
    inp, st, ref = X.case(geom, EPOCH)
    pc, ps = ref["parts"]["clean"], ref["parts"]["strong"]
    W1, b1 = st["student"][:2]
    us = int(np.nonzero(np.asarray(ref["oracle"]["mask"]) > 0)[0][-1])      # the last strong utterance in the mask
    yield "last slab of the last masked-in strong utterance dropped", _dw1(ref, strong=dict(act=_last_slab_off(ps, us)))
    uc = pc["x"].shape[0] - 1
    yield "last clean slab dropped", _dw1(ref, clean=dict(act=_last_slab_off(pc, uc)))
    lens = pc["vlen"].copy()
    # the clean utterance whose scales g / len move most under len + 1 (by |g| / (len (len + 1)))
    u = int(np.argmax(np.linalg.norm(pc["g"], axis=1) / (lens * (lens + 1))))
    lens[u] += 1
    yield "clean utterance %d divided by len + 1" % u, _dw1(ref, clean=dict(lens=lens))
    h = int(np.argmax(np.linalg.norm(ref["grads"][0], axis=1)))
    dw = ref["grads"][0].copy()
    dw[h] *= 2.0
    yield "hidden unit %d's row scaled by 2" % h, dw
    xw = ref["parts"]["weak_x"]
    act_w = dad_oracle.encoder_forward(xw, inp["mn"], W1, b1)[1]
    yield "weak-augmented input in place of the strong one", _dw1(ref, strong=dict(x=xw, act=act_w))


@GEOMS
def test_wrong_weight_gradients_exceed_the_fp16_bound_tenfold(geom):
    ref = X.case(geom, EPOCH)[2]
    for what, dw in _mutants(geom):
        r = _ratio(dw, ref, "fp16")
        print("%s: %s: %.1f x the fp16 bound" % (X.geom_id(geom), what, r))
        assert r >= 10.0, (what, r)


# ---------------------------------------------------------------- the long problems' own controls
# (X.LONG_GEOMS: past about 100 slabs one slab carries less of S_W1 than the bound allows, so the mutants above
# would pass there; the sentinel channels give every slab a column it shares with only every 128th slab.)

def _wg_slabs(geom, epoch=EPOCH):
    """Every weight-gradient slab of a long problem in dad_wg_total's order: (s, branch, u, c, frames, loud), frames =
    the slab's valid frames outside the temporal zero; loud = a clean or masked-in slab with at least 16 of them."""
    inp, _, ref = X.case(geom, epoch)
    c = X.cfg()
    mlen = int(geom["Tn"] * c["TEMPORAL_MASK_RATIO"])
    mask = np.asarray(ref["oracle"]["mask"]) > 0
    for noisy, B, T, lens in ((False, geom["B"], geom["T"], geom["lens_c"]), (True, geom["Bn"], geom["Tn"], geom["lens_n"])):
        for u in range(B):
            live = np.arange(T) < lens[u]
            if noisy:
                live[int(inp["start"][u]):int(inp["start"][u]) + mlen] = False
            for k in range((T + 31) // 32):
                frames = int(live[32 * k:32 * k + 32].sum())
                loud = frames >= 16 and (not noisy or bool(mask[u]))
                yield X.wg_slab(geom["B"], geom["T"], geom["Bn"], geom["Tn"], noisy, u, k), "strong" if noisy else "clean", u, k, frames, loud


@SENTINEL
def test_sentinel_channels_hold_one_slab_in_128(geom):
    inp = X.case(geom, EPOCH)[0]
    xw, xs = X.augmented(inp, X.cfg())
    assert np.all(inp["u"][X.SENT0:] == 1.0)
    for s, branch, u, k, frames, _ in _wg_slabs(geom):
        rows = slice(32 * k, 32 * k + 32)
        own = X.SENT0 + s % X.SENT_N
        for a in ((inp["xc"],) if branch == "clean" else (inp["xn"], inp["nw"], inp["ns"], xw, xs)):
            sent = a[u, rows, X.SENT0:].copy()
            sent[:, own - X.SENT0] = 0
            assert not sent.any(), (s, branch)
        x = inp["xc"] if branch == "clean" else inp["xn"]
        pad = (inp["mc"] if branch == "clean" else inp["mn"])[u, rows]
        v = x[u, rows, own]
        assert np.all(v[pad] == 0) and np.all(np.abs(v[~pad]) >= 0.125) and np.all(np.abs(v[~pad]) <= 2.0), (s, branch)


@SENTINEL
def test_every_loud_slab_is_visible_in_the_weight_gradient(geom):
    """Clearing a loud slab's ReLU' bits, and counting the slab twice, each move some dW1 element at least 10x
    outside the fp16 bound."""
    ref = X.case(geom, EPOCH)[2]
    lim = X.grad_limit("dW1", "fp16", ref)
    dw_ref = ref["grads"][0]
    slabs = list(_wg_slabs(geom))
    loud = [t for t in slabs if t[5]]
    worst = {}
    for s, branch, u, k, frames, _ in loud:
        p = ref["parts"][branch]
        rows = slice(32 * k, 32 * k + 32)
        scale = p["g"][u] / max(p["vlen"][u], 1.0)
        own = scale[:, None] * (p["act"][u, rows].astype(np.float64).T @ p["x"][u, rows].astype(np.float64))
        for what, dw in (("dropped", dw_ref - own), ("twice", dw_ref + own)):
            worst[(s, what)] = X.worst(dw - dw_ref, lim)
    low = min(worst, key=worst.get)
    print("%s: %d loud and %d silent slabs; a loud slab dropped or counted twice reads %.1f x to %.1f x the fp16 bound "
          "(least: slab %d %s)" % (X.geom_id(geom), len(loud), len(slabs) - len(loud), worst[low], max(worst.values()),
                                    low[0], low[1]))
    assert loud and worst[low] >= 10.0, (low, worst[low])


def test_l3_splits_begin_and_end_in_loud_slabs_and_its_mask_is_mixed():
    geom = X.LONG["L3"]
    mask = np.asarray(X.case(geom, EPOCH)[2]["oracle"]["mask"])
    assert mask.min() == 0 and mask.max() == 1 and mask.sum() >= 8, mask
    loud = {t[0]: t[5] for t in _wg_slabs(geom)}
    assert len(loud) == 22 * 64
    for split in range(22):
        assert loud[64 * split] and loud[64 * split + 63], split


def _slab_partials(x, pad, W1, b1):
    """The encoder's per-slab pooled sums and active counts [B, ceil(T / 32), H] in float64, and the lengths."""
    pre = X.preact64(x, W1, b1)
    act = (pre > 0) & ~pad[..., None]
    B, T, H = pre.shape
    nc = (T + 31) // 32
    r, a = np.zeros((B, 32 * nc, H)), np.zeros((B, 32 * nc, H))
    r[:, :T], a[:, :T] = np.where(act, pre, 0.0), act
    return r.reshape(B, nc, 32, H).sum(2), a.reshape(B, nc, 32, H).sum(2), (~pad).sum(1).astype(np.float64)


# what csrc/pool.h's loops could get wrong past 16 slabs / 512 frames, as (name, slabs summed of nc, frames counted of T)
_POOL_MUTANTS = (("only the first 16 slabs summed", lambda nc: slice(0, 16), None),
                 ("the last slab left out", lambda nc: slice(0, nc - 1), None),
                 ("the length stops counting at frame 512", lambda nc: slice(0, nc), 512))


@POOLED
def test_pool_mutants_past_16_slabs_exceed_the_bounds_tenfold(geom):
    inp, st, ref = X.case(geom, EPOCH)
    pads = {"clean": inp["mc"], "weak": inp["mn"], "strong": inp["mn"]}
    names = {"clean": "e_clean", "weak": "e_teacher", "strong": "e_strong"}
    parts = {name: _slab_partials(x, pads[name], W1, b1) for name, x, W1, b1 in _encoder_operands(geom)}
    for name, (ps, pc, vlen) in parts.items():        # the rebuild itself
        e = ps.sum(1) / np.maximum(vlen, 1.0)[:, None]
        assert X.worst(e - ref["e"][names[name]], X.bound("e", None, ref["T"][names[name]]) * np.abs(e)) < 1e-6
    for what, take, stop in _POOL_MUTANTS:
        db1 = np.zeros(ref["grads"][1].shape)
        for name, (ps, pc, vlen) in parts.items():
            sel = take(ps.shape[1])
            n = vlen if stop is None else np.minimum(vlen, stop)
            e = ps[:, sel].sum(1) / np.maximum(n, 1.0)[:, None]
            er = ref["e"][names[name]]
            r = X.worst(e - er, X.bound("e", None, ref["T"][names[name]]) * np.abs(er))
            print("%s: %s: %s %.0f x its bound" % (X.geom_id(geom), what, names[name], r))
            assert r >= 10.0, (what, name, r)
            if name != "weak":      # cnt_tot and the length the kernel stores feed db1 = sum_u dL/de_u / len_u * count_u
                p = ref["parts"][name]
                db1 += ((p["g"] / np.maximum(n, 1.0)[:, None]) * pc[:, sel].sum(1)).sum(0)
        r = X.worst(db1 - ref["grads"][1], X.grad_limit("db1", "fp16", ref))
        print("%s: %s: db1 %.0f x its bound" % (X.geom_id(geom), what, r))
        assert r >= 10.0, (what, r)


# ---------------------------------------------------------------- the supervised-contrastive term
# (tests/test_gpu_exact_scl.py's cases: exact_problem's reference with the term, "contrastive term" in its docstring)

def _scl_cases():
    cases = [(g, ecda, None) for g in X.GEOMS for ecda in (True, False)]
    cases += [(X.PAST64, True, None), (X.LONG["L1"], True, None), (X.GEOMS[2], True, 8.0)]
    return cases


def _scl_id(c):
    return X.geom_id(c[0]) + ("" if c[1] else "-noecda") + ("-w%g" % c[2] if c[2] else "")


SCL_CASES = pytest.mark.parametrize("case", _scl_cases(), ids=_scl_id)


def _scl_case(case):
    geom, ecda, weight = case
    return X.case(geom, EPOCH, **X.scl_over(geom, ecda, weight))


LOOSEST = "bf16"       # the loosest bound a case is checked under, ECDA on or off: its eps_op is the largest of the three


def test_scl_weight_rule_and_the_off_path():
    c = dict(X.cfg(), **X.SCL_ON)
    assert [X.scl_weight(c, e) for e in (0, 29, 30, 60)] == [0.0, 0.0, 1.0, 1.0]
    assert X.scl_weight(dict(c, SCL_START_EPOCH=61), 60) == 0.0 and X.scl_weight(X.cfg(), 60) == 0.0
    ref = X.case(X.GEOMS[1], EPOCH)[2]
    assert "scl" not in ref and "tail_b1" not in ref and "total_loss" not in ref
    # the term moves dW1 and db1 only, and the base it is added to is the step's without it
    on = _scl_case((X.GEOMS[1], True, None))[2]
    for i in (2, 3):
        assert np.array_equal(on["grads"][i], ref["grads"][i]) and np.array_equal(on["S"][i], ref["S"][i])
    assert np.array_equal(on["scl"]["base"]["clean"], ref["parts"]["clean"]["g"])
    assert not np.array_equal(on["grads"][0], ref["grads"][0]) and not np.array_equal(on["grads"][1], ref["grads"][1])
    assert on["total_loss"] == ref["oracle"]["total_loss"] + on["scl"]["loss"]


@SCL_CASES
def test_scl_gates_members_and_the_two_restatements_agree(case):
    geom = case[0]
    inp, st, ref = _scl_case(case)
    s, r = ref["scl"], ref["oracle"]
    mask = np.asarray(r["mask"])
    margin = np.abs(np.asarray(r["score"], np.float64) - np.asarray(r["tau_after"], np.float64)[r["pred"]]).min()
    assert mask.sum() >= 2 and r["consistency_loss"] != 0.0
    if geom["Bn"] >= 7:
        assert mask.min() == 0 and mask.max() == 1 and margin >= 0.07, (mask, margin)
    assert s["members"] == len(inp["yc"]) + int(mask.sum()) and s["V"] == int(np.sum(s["anchors"]))
    # the noisy labels handed to the step are wrong in every row the mask lets in
    assert np.all((inp["yn"] != np.asarray(r["pred"]))[mask > 0])
    gmax = np.abs(s["g"]).max()
    agree = np.abs(s["g"] - s["g_closed"]).max() / gmax if gmax > 0 else 0.0
    print("%s: members %d, anchors %s, loss %.6f; autograd against the closed form %.2g of max |g|; the allowance's "
          "sensitivity part is %.2f of its 1e-4 part" % (_scl_id(case), s["members"], [int(a) for a in s["anchors"]], s["loss"], agree,
                                                         s["sensitivity"]))
    assert agree <= 1e-12 and abs(s["loss"] - s["loss_closed"]) <= 1e-12 * max(1.0, abs(s["loss"]))
    if s["V"] == 0:
        assert s["loss"] == 0.0 and not np.any(s["g"]) and geom["B"] == 1
    if geom is X.PAST64:
        assert len(s["member"]) > 128 and s["members"] > 64 and ref["parts"]["clean"]["x"].shape[0] > 64 and len(mask) > 64


@SCL_CASES
def test_scl_term_is_visible_in_the_weight_gradient(case):
    ref = _scl_case(case)[2]
    s = ref["scl"]
    rest = ref["S"][0] - s["S_term"]
    print("%s: the term's share of S_W1 %.4f (median over the elements; %.3g x everything else); |w g| %.3f" % (
        _scl_id(case), s["share"], np.median(s["S_term"][rest > 0] / rest[rest > 0]) if s["V"] else 0.0,
        s["w"] * np.linalg.norm(s["g"])))
    if s["V"]:
        assert s["share"] >= 0.03, s["share"]


def _f32_restatement(inp, st, ref):
    """[dW1, db1] of the step with the term in float32: a float32 pooled encoder, scl_closed_form(dtype=float32) on
    its embeddings and a float32 weight-gradient sum (the base dL/de: the oracle's, rounded to float32)."""
    import scl_ref
    s = ref["scl"]
    W1, b1 = st["student"][:2]
    pc, ps = ref["parts"]["clean"], ref["parts"]["strong"]
    e32 = np.concatenate([X.pool32(pc["x"], inp["mc"], W1, b1), X.pool32(ps["x"], inp["mn"], W1, b1)], 0)
    assert e32.dtype == np.float32
    g32 = scl_ref.scl_closed_form(e32, s["labels"], s["member"], s["tau"], dtype=np.float32)[1].astype(np.float32)
    Bc = pc["x"].shape[0]
    dW, db = np.zeros(ref["grads"][0].shape, np.float32), np.zeros(ref["grads"][1].shape, np.float32)
    for p, base, g in ((pc, s["base"]["clean"], g32[:Bc]), (ps, s["base"]["strong"], g32[Bc:])):
        scale = (base.astype(np.float32) + np.float32(s["w"]) * g) / np.maximum(p["vlen"], 1.0).astype(np.float32)[:, None]
        for u in range(len(scale)):
            a = p["act"][u].astype(np.float32).T
            dW += scale[u][:, None] * (a @ p["x"][u].astype(np.float32))
            db += scale[u] * a.sum(1)
    assert dW.dtype == np.float32 and db.dtype == np.float32
    return dW, db


@SCL_CASES
def test_scl_float32_restatement_lies_inside_every_bound(case):
    inp, st, ref = _scl_case(case)
    dW, db = _f32_restatement(inp, st, ref)
    for prec in ("fp32", "fp16", "bf16"):
        r = {n: X.worst(g - ref["grads"][i], X.grad_limit(n, prec, ref)) for i, (n, g) in enumerate((("dW1", dW), ("db1", db)))}
        print("%s: float32 restatement, %s bound: dW1 %.3f db1 %.3f" % (_scl_id(case), prec, r["dW1"], r["db1"]))
        assert max(r.values()) <= 1.0, (prec, r)


def _scl_of_z(z, y, tau):
    """scl_ref.scl_torch's loss as a function of the unit rows themselves (nothing normalised inside)."""
    y = torch.as_tensor(np.asarray(y))
    m = z.shape[0]
    s = (z @ z.T) / tau
    eye = torch.eye(m, dtype=torch.bool)
    lse = torch.logsumexp(s.masked_fill(eye, -float("inf")), dim=1)
    pos = (y[:, None] == y[None, :]) & ~eye
    npos = pos.sum(1)
    anchor = npos >= 1
    return (-((s - lse[:, None]) * pos).sum(1)[anchor] / npos[anchor]).mean()


def _scl_dw1(ref, g, base=None, strong=None):
    """dW1 in float64: the branches' base dL/de (or `base`) through their own inputs, plus w x the term `g`
    [Bc + Bn, H]; strong: replacement (x, act) for the TERM's strong rows."""
    s = ref["scl"]
    pc, ps = ref["parts"]["clean"], ref["parts"]["strong"]
    base = s["base"] if base is None else base
    Bc = pc["x"].shape[0]
    dw = X.wgrad64(pc["x"], pc["act"], pc["vlen"], base["clean"] + s["w"] * g[:Bc])[0]
    dw += X.wgrad64(ps["x"], ps["act"], ps["vlen"], base["strong"])[0]
    tx, tact = (ps["x"], ps["act"]) if strong is None else strong
    return dw + X.wgrad64(tx, tact, ps["vlen"], s["w"] * g[Bc:])[0]


def _scl_controls(case):
    """(name, wrong dW1) for every way the issue lists of carrying the term wrongly that applies to the case."""
    import scl_ref
    geom, ecda, weight = case
    inp, st, ref = _scl_case(case)
    s, r = ref["scl"], ref["oracle"]
    emb, labels, member, tau = np.concatenate([ref["e"]["e_clean"], ref["e"]["e_strong"]], 0), s["labels"], s["member"], s["tau"]
    Bc = len(inp["yc"])
    yield "the term dropped", _scl_dw1(ref, np.zeros_like(s["g"]))
    if ecda and r["ecda_loss"] != 0.0:
        off = X.case(geom, EPOCH, **X.scl_over(geom, False, weight))[2]["scl"]["base"]
        m = (member != 0)[:, None]
        base = dict(clean=np.where(m[:Bc], off["clean"], s["base"]["clean"]), strong=np.where(m[Bc:], off["strong"], s["base"]["strong"]))
        assert not np.array_equal(base["clean"], s["base"]["clean"])
        yield "the term overwrites the ECDA part of the flagged rows", _scl_dw1(ref, s["g"], base=base)
    if not member.all():
        yield "masked-out strong rows taken as members", _scl_dw1(ref, scl_ref.scl_autograd(emb, labels, np.ones_like(member), tau)[1])
    true = np.concatenate([inp["yc"], inp["yn"]])
    yield "the noisy batch's labels in place of the pseudo-labels", _scl_dw1(ref, scl_ref.scl_autograd(emb, true, member, tau)[1])
    p = X.cfg()["DROPOUT_RATE"]
    post = emb * np.concatenate([inp["keep1"], inp["keep2"]], 0).astype(np.float64) / (1.0 - p)
    yield "post-dropout embeddings", _scl_dw1(ref, scl_ref.scl_autograd(post, labels, member, tau)[1])
    idx = scl_ref.members(emb, labels, member)
    nrm = np.linalg.norm(emb[idx], axis=1)
    z = torch.tensor(emb[idx] / nrm[:, None], dtype=torch.float64, requires_grad=True)
    _scl_of_z(z, labels[idx], tau).backward()
    g = np.zeros_like(s["g"])
    g[idx] = z.grad.numpy() / nrm[:, None]
    yield "the normalisation's backward left out", _scl_dw1(ref, g)
    yield "tau = 0.07", _scl_dw1(ref, scl_ref.scl_autograd(emb, labels, member, 0.07)[1])
    if s["V"] != s["members"]:
        yield "the mean taken over the members", _scl_dw1(ref, s["g"] * s["V"] / s["members"])
    xw = ref["parts"]["weak_x"]
    act_w = dad_oracle.encoder_forward(xw, inp["mn"], *st["student"][:2])[1]
    yield "the strong rows' share sent through the weak input", _scl_dw1(ref, s["g"], strong=(xw, act_w))


@SCL_CASES
def test_scl_wrong_terms_exceed_the_loosest_bound_tenfold(case):
    geom = case[0]
    ref = _scl_case(case)[2]
    assert _ratio(_scl_dw1(ref, ref["scl"]["g"]), ref, "fp32") < 1e-6          # the rebuild itself
    if ref["scl"]["V"] == 0:
        return
    prec = LOOSEST
    seen = {}
    lim = X.grad_limit("dW1", prec, ref)
    for what, dw in _scl_controls(case):
        # (over the elements that have a bound: the weak input also reaches channels the feature mask zeroes, where
        # S_W1 = 0 and any value is infinitely far out)
        seen[what] = X.worst((dw - ref["grads"][0])[lim > 0], lim[lim > 0])
        print("%s: %s: %.1f x the %s bound" % (_scl_id(case), what, seen[what], prec))
    least = min(seen, key=seen.get)
    print("%s: the least factor is %.1f (%s)" % (_scl_id(case), seen[least], least))
    if X.geom_id(geom) == "B5T33_Bn7Tn31":
        assert "the mean taken over the members" in seen
    assert seen[least] >= 10.0, (least, seen[least])


def test_scl_weight_8_makes_the_term_and_ecda_of_one_size_in_the_flagged_rows():
    """Within a factor of 4 of each other, by the norm over the member rows: neither is a rounding of the other in
    the fp16 weight gradient's per-hidden-unit scale."""
    geom = X.GEOMS[2]
    s = _scl_case((geom, True, 8.0))[2]["scl"]
    off = _scl_case((geom, False, 8.0))[2]["scl"]["base"]
    m = s["member"] != 0
    ecda = np.concatenate([s["base"]["clean"] - off["clean"], s["base"]["strong"] - off["strong"]], 0)[m]
    size = np.linalg.norm(s["w"] * s["g"][m]) / np.linalg.norm(ecda)
    print("weight 8: |w g_scl| / |ECDA's dL/de| over the member rows %.3f (weight 1: %.3f)" % (size, size / 8.0))
    assert s["w"] == 8.0 and 0.25 <= size <= 4.0, size
