"""Seeded cases and float64 references for the stand-alone C-ABI operators (TEST INFRASTRUCTURE; imports oracle/ and
tests/exact_problem.py only): csrc/utils_abi.hip (dad_augment, dad_certainty_scores, dad_dacp_mask, dad_ecda_loss),
csrc/encoder_ops.hip (dad_encoder_forward / dad_encoder_backward) and csrc/eval.hip (dad_predict_head).

tests/test_operators_ref_cpu.py asserts, on the reference alone, every condition the GPU modules
(test_gpu_helper_ops.py, test_gpu_encoder_ops.py) rely on, and that each bound rejects a wrong answer.

Bounds (u = 2^-24; none is a measured number):
  prediction head   logits  |z - z_ref| <= (H + 8) u (|e| |W2|^T + |b2|): H products, H - 1 additions in any order
                    and the bias, as exact_problem's logit bound without the T of its pooled embedding.
                    probs   |p - p_ref| <= (2 eps_z + (C + 6) u) p_ref, eps_z = the row's largest logit bound
                    (exact_problem's softmax term: dp_c = p_c (dz_c - sum_j p_j dz_j); exp, C additions, division).
                    score   rtol 1e-5, atol 1e-6 of float64 (test_gpu_eval.py's), pred = the first maximum wherever
                    the reference's top-two logit gap exceeds 2 eps_z.
  certainty, DACP   the project's 1e-6 (gpu_harness.close) against oracle/dad_oracle.py; mask and pred equal.
  ECDA              loss 1e-4 (|loss - ref| <= 1e-4 max(1, |ref|)), gradients gpu_harness.close_grad: test_gpu_utils.py's.
  encoder forward   |e - e_ref| <= (T + 2) u |e_ref| in fp32, fp16 and bf16 (exact_problem's embedding bound: the
                    operands are exact in all three, the pooled terms exact and non-negative).
  encoder backward  |g - g_ref| <= c u S_g elementwise, c = B T + 2, S_g the reference's sum of magnitudes:
                    dW1[h][d] = sum over the active frames (b, t) of s_bh x_btd with s_bh = de_bh / max(len_b, 1).
                    x is exact (the grid).  s_bh is ONE fp32 division: relative error <= u.  Each product s x rounds
                    once (u) unless fused into the sum, and an fp32 sum of N <= B T terms in ANY order (split-K
                    partials included: every summation tree of N leaves has depth <= N - 1) adds (N - 1) u: together
                    (1 + u)^(N + 1) - 1 <= (N + 1) u + ((N + 1) u)^2, and for N <= 1024 the second-order term is
                    below 0.07 u.  So c = N + 2 with N = B T.  db1[h] = sum_b s_bh n_bh (n_bh active frames, an exact
                    integer) is the same sum with the frames of an utterance grouped: the same c covers it.
                    S_g = 0 (only padded frames or a dead ReLU feed the element) demands g = 0 exactly.
"""
import numpy as np

import exact_problem as X
from oracle import dad_oracle, synth

U32 = X.U32
H, D, C = synth.H_DIM, synth.D_IN, synth.N_CLS
F32 = np.float32
SLAB = 32                      # csrc DAD_SLAB: frames per encoder slab
worst = X.worst


def cfg(**over):
    return dad_oracle.make_cfg("iemocap", **over)


# ------------------------------------------------------------------------------------- prediction head
HEAD_SEED = 5
HEAD_B = (1, 3, 4, 5, 37)
HEAD_KINDS = ("plain", "tie", "all_tie", "wide")
SCORE_RTOL, SCORE_ATOL = 1e-5, 1e-6          # tests/test_gpu_eval.py's


def head_case(B, kind="plain", seed=HEAD_SEED):
    """(e [B, H], W2 [C, H], b2 [C]) float32.  e: non-negative multiples of 2^-10 (a pooled ReLU output on the grid);
    W2, b2: synth.init_weights.  kind 'tie': the most often predicted class's row and bias copied to another class
    (tie_pair finds the two); 'all_tie': every row class 0's; 'wide': W2 scaled until the reference logits span about +-80 (fp32 probabilities underflow to 0)."""
    assert kind in HEAD_KINDS
    rs = np.random.RandomState(seed * 1000 + B)
    W2, b2 = [a.copy() for a in synth.init_weights(seed)[2:4]]
    e = X.q(np.abs(rs.standard_normal((B, H))) * 0.5, 2.0 ** -10)
    if kind == "tie":
        k = np.bincount((e.astype(np.float64) @ W2.astype(np.float64).T + b2).argmax(1), minlength=C).argmax()
        j = C - 1 if k < C - 1 else 0
        W2[j], b2[j] = W2[k], b2[k]
    elif kind == "all_tie":
        W2[:], b2[:] = W2[0], b2[0]
    elif kind == "wide":
        z = e.astype(np.float64) @ W2.astype(np.float64).T
        z = z - z.mean(1, keepdims=True)
        W2 = (W2 - W2.mean(0, keepdims=True)) * F32(80.0 / np.abs(z).max())
    return e, W2.astype(F32), b2.astype(F32)


def tie_pair(W2, b2):
    """(lower, higher) index of the two identical classifier rows of a 'tie' case."""
    for i in range(C):
        for j in range(i + 1, C):
            if np.array_equal(W2[i], W2[j]) and b2[i] == b2[j]:
                return i, j
    raise AssertionError("no two identical rows")


def head_reference(e, W2, b2, last_max=False):
    """float64 head of float32 operands: dict(z, z_lim, eps_z, p, p_lim, score {True/False: use_entropy}, pred, gap,
    decided).  last_max: the wrong-answer control (last maximal index)."""
    e64, W64, b64 = (np.asarray(a, np.float64) for a in (e, W2, b2))
    z = e64 @ W64.T + b64
    z_lim = (H + 8) * U32 * (np.abs(e64) @ np.abs(W64).T + np.abs(b64))
    eps_z = z_lim.max(1)
    p = dad_oracle.softmax(z)
    p_lim = (2.0 * eps_z + (C + 6) * U32)[:, None] * p
    ent = -(p * np.log2(p + 1e-8)).sum(1)                  # I/utils.py:417
    mp = p.max(1)
    pred = (C - 1 - z[:, ::-1].argmax(1)) if last_max else z.argmax(1)
    top = np.sort(z, axis=1)
    gap = top[:, -1] - top[:, -2]
    return dict(z=z, z_lim=z_lim, eps_z=eps_z, p=p, p_lim=p_lim, score={True: mp * (1.0 - ent / np.log2(C)), False: mp},
                pred=pred, gap=gap, decided=gap > 2.0 * eps_z)


def score_lim(ref):
    return SCORE_ATOL + SCORE_RTOL * np.abs(ref)


# ------------------------------------------------------------------------------------- certainty scores
CERT_B = (1, 255, 256, 257, 1000)
CERT_TOL = 1e-6
# one-hot (p = 0 entries), uniform, an exact two-way tie at index 0 and one whose first maximum is index 1
SPECIAL_ROWS = np.array([[0, 0, 1, 0], [0.25, 0.25, 0.25, 0.25], [0.4, 0.1, 0.4, 0.1], [0.1, 0.4, 0.4, 0.1]], F32)
SPECIAL_PRED = (2, 0, 0, 1)


def special_slots(B):
    """Rows of a B-row case that hold SPECIAL_ROWS (all four from B = 255 on; B = 1 runs each alone)."""
    return [0, 1, B // 2, B - 1] if B >= 4 else []


def certainty_case(B, seed=21):
    rs = np.random.RandomState(seed + B)
    p = dad_oracle.softmax(3.0 * rs.standard_normal((B, C))).astype(F32)
    for row, slot in zip(SPECIAL_ROWS, special_slots(B)):
        p[slot] = row
    return p


# ------------------------------------------------------------------------------------------------ DACP
DACP_MARGIN = 0.07             # exact_problem.py's: every case below allows it
DACP_TOP2 = 1e-3
DACP_CALLS = 2
# (Bn, kind, seed).  kind: 'mixed' rows over all classes; 'empty' no row predicts class 2; 'single' exactly one row
# predicts class 2; 'one_class' every row predicts class 1.  The seeds are those for which dad_oracle.dacp_mask alone
# meets the conditions of test_operators_ref_cpu.py (margin, top-two gap, both mask values from Bn = 5 on).
DACP_CASES = [(1, "one_class", 101), (2, "mixed", 102), (5, "mixed", 103), (5, "single", 104), (64, "mixed", 105),
              (64, "one_class", 106), (65, "mixed", 107), (65, "empty", 108), (511, "mixed", 109), (513, "mixed", 110),
              (513, "single", 111), (513, "one_class", 114), (1024, "mixed", 112), (1024, "empty", 113),
              (1024, "one_class", 115)]
# the cases whose one class holds more than 512 scores: dacp_thresholds' srt[c][512 ...] and a quantile rank past 512
DACP_OVER_512 = ("Bn513_one_class", "Bn1024_one_class")


def dacp_id(case):
    return "Bn%d_%s" % case[:2]


def _dacp_band(tau0, anchors, c, calls):
    """Where a threshold can lie after 1..calls updates, whatever the batch: tau' = a tau + (1 - a) F with
    F = max(tau_hat + lambda (w - 1/2), anchor), tau_hat in [0, 1] (a score, or the old threshold), w in (0, 1)."""
    a, lam = c["DACP_THRESHOLD_SMOOTHING_ALPHA"], c["DACP_CALIBRATION_STRENGTH_LAMBDA"]
    f_lo, f_hi = np.maximum(-0.5 * lam, anchors), np.maximum(1.0 + 0.5 * lam, anchors)
    lo, hi = tau0.astype(np.float64), tau0.astype(np.float64)
    band_lo, band_hi = np.full(C, np.inf), np.full(C, -np.inf)
    for _ in range(calls):
        lo, hi = a * lo + (1 - a) * f_lo, a * hi + (1 - a) * f_hi
        band_lo, band_hi = np.minimum(band_lo, lo), np.maximum(band_hi, hi)
    return band_lo, band_hi


def dacp_case(case):
    """(probs [Bn, 4] f32, tau [4], Q [4], anchors [4], epoch).  Each row is drawn until its pseudo-label is the
    class the kind assigns it, its top two probabilities differ by 2 DACP_TOP2 and its certainty score keeps
    DACP_MARGIN from the band the class's threshold can reach (_dacp_band); every row drawn this way is compared."""
    Bn, kind, seed = case
    rs = np.random.RandomState(seed)
    c = cfg()
    tau = rs.uniform(0.45, 0.65, C).astype(F32)
    Q = rs.uniform(0.3, 0.7, C).astype(F32)
    anchors = rs.uniform(0.1, 0.3, C).astype(F32)
    epoch = int(rs.randint(30, 400))
    lo, hi = _dacp_band(tau, anchors, c, DACP_CALLS)
    cls = {"mixed": rs.randint(0, C, Bn), "empty": np.array([0, 1, 3])[rs.randint(0, 3, Bn)],
           "single": np.array([0, 1, 3])[rs.randint(0, 3, Bn)], "one_class": np.full(Bn, 1)}[kind]
    if kind == "single":
        cls[rs.randint(0, Bn)] = 2
    probs = np.zeros((Bn, C), F32)
    for b in range(Bn):
        while True:
            z = rs.standard_normal(C)
            z[cls[b]] += rs.uniform(0.5, 9.0)
            p = dad_oracle.softmax(z[None]).astype(F32)
            s, pr = dad_oracle.certainty_scores(p, True)
            top = np.sort(p[0])
            outside = s[0] < lo[cls[b]] - DACP_MARGIN - 0.01 or s[0] > hi[cls[b]] + DACP_MARGIN + 0.01
            if pr[0] == cls[b] and top[-1] - top[-2] > 2 * DACP_TOP2 and outside:
                probs[b] = p[0]
                break
    return probs, tau, Q, anchors, epoch


def dacp_reference(case, calls=DACP_CALLS):
    """dad_oracle.dacp_mask applied `calls` times to the case: [dict(mask, score, pred, w, tau, sums, counts)] per
    call (tau / sums / counts: the state after it), and the DACPState."""
    probs, tau, Q, anchors, epoch = dacp_case(case)
    st = dad_oracle.DACPState(C, tau, Q)
    out = []
    for _ in range(calls):
        mask, s, pred, w, _ = dad_oracle.dacp_mask(st, probs, epoch, anchors, cfg(), True)
        out.append(dict(mask=mask, score=s, pred=pred, w=w, tau=st.tau.copy(), sums=st.score_sum.copy(),
                        counts=st.score_cnt.copy()))
    return out, st


# ------------------------------------------------------------------------------------------------ ECDA
# Member counts per class: clean rows labelled c, noisy rows predicted c and masked in ('inn') or masked out ('out').
# w: 'dacp' = DACP's [4] class weights, 'ones' = ones(Bn) of the fixed-threshold branch (I/train.py:420): the
# reference then loops its classes over range(Bn) (I/utils.py: `for c in range(len(class_weights_wce))`).
# aware: which USE_CLASS_AWARE_MMD settings run the case.  expect: what test_operators_ref_cpu.py asserts of it:
#   gated   classes whose term enters the loss (len(si) >= 2 and len(ti) >= 2)
#   cent    classes with a noisy centroid (repulsion needs two)
#   single  classes skipped for len(si) < 2 although len(ti) >= 2
#   beyond  classes with members that range(len(w)) never reaches
# The kernel takes another path at B or Bn > 64 (ECDA_PRE: rows prefetched into registers) and at more than 80
# members of a class (ECDA_NZ: members staged in LDS); the cases stand on both sides of each.  The oracle's
# [n, n, H] float64 temporary bounds one class block to a few hundred members: 234 at the most here.
ECDA_CASES = {
    "B5_Bn7": dict(clean=[2, 3, 0, 0], inn=[3, 2, 1, 0], out=[0, 1, 0, 0], w="dacp", aware=(True, False),
                   expect=dict(gated=[0, 1], cent=[0, 1, 2], single=[], beyond=[])),
    "B1_Bn1": dict(clean=[1, 0, 0, 0], inn=[1, 0, 0, 0], out=[0, 0, 0, 0], w="dacp", aware=(True, False),
                   expect=dict(gated=[], cent=[0], single=[], beyond=[])),
    "B64_Bn3": dict(clean=[16, 16, 16, 16], inn=[2, 1, 0, 0], out=[0, 0, 0, 0], w="dacp", aware=(True, False),
                    expect=dict(gated=[0], cent=[0, 1], single=[], beyond=[])),
    "all_zero_mask": dict(clean=[2, 2, 2, 2], inn=[0, 0, 0, 0], out=[2, 2, 2, 2], w="dacp", aware=(True, False),
                          expect=dict(gated=[], cent=[], single=[], beyond=[])),
    "single_clean_row": dict(clean=[1, 3, 2, 0], inn=[2, 2, 0, 0], out=[0, 0, 1, 0], w="dacp", aware=(True, False),
                             expect=dict(gated=[1], cent=[0, 1], single=[0], beyond=[])),
    "one_valid_class": dict(clean=[3, 2, 0, 0], inn=[4, 0, 0, 0], out=[0, 2, 0, 0], w="dacp", aware=(True, False),
                            expect=dict(gated=[0], cent=[0], single=[], beyond=[])),
    "pre_82_members": dict(clean=[41, 10, 8, 5], inn=[41, 10, 5, 3], out=[2, 1, 1, 1], w="dacp", aware=(True,),
                           expect=dict(gated=[0, 1, 2, 3], cent=[0, 1, 2, 3], single=[], beyond=[])),
    "B70_Bn66_staged": dict(clean=[20, 20, 15, 15], inn=[18, 16, 14, 10], out=[2, 2, 2, 2], w="dacp", aware=(True,),
                            expect=dict(gated=[0, 1, 2, 3], cent=[0, 1, 2, 3], single=[], beyond=[])),
    "B520_Bn520": dict(clean=[130] * 4, inn=[104] * 4, out=[26] * 4, w="dacp", aware=(True,),
                       expect=dict(gated=[0, 1, 2, 3], cent=[0, 1, 2, 3], single=[], beyond=[])),
    "global_B130_Bn70": dict(clean=[33, 33, 32, 32], inn=[15, 15, 15, 15], out=[3, 3, 2, 2], w="dacp", aware=(False,),
                             expect=dict(gated=[0, 1, 2, 3], cent=[0, 1, 2, 3], single=[], beyond=[])),
    "ones_Bn2_class3": dict(clean=[0, 0, 2, 3], inn=[0, 0, 0, 2], out=[0, 0, 0, 0], w="ones", aware=(True, False),
                            expect=dict(gated=[], cent=[], single=[], beyond=[2, 3])),
    "ones_Bn2_class1": dict(clean=[2, 3, 0, 0], inn=[0, 2, 0, 0], out=[0, 0, 0, 0], w="ones", aware=(True, False),
                            expect=dict(gated=[1], cent=[1], single=[], beyond=[])),
    "ones_Bn3": dict(clean=[2, 0, 2, 2], inn=[1, 0, 2, 0], out=[0, 0, 0, 0], w="ones", aware=(True, False),
                     expect=dict(gated=[2], cent=[0, 2], single=[], beyond=[3])),
    # n_weights == Bn == 4: dad_ecda_loss reads four weights as DACP's.  The reference has ONE formula for both
    # (attention exp(lambda (mean(w) - w)), classes range(len(w))): for ones(4) the attention is exp(0) = 1 and
    # range(4) = every class, which is also what the ones(Bn) branch gives (unit attention, classes < min(Bn, 4)).
    "ones_Bn4": dict(clean=[2, 2, 2, 2], inn=[2, 0, 0, 2], out=[0, 0, 0, 0], w="ones", aware=(True, False),
                     expect=dict(gated=[0, 3], cent=[0, 3], single=[], beyond=[])),
    "ones_Bn9": dict(clean=[3, 3, 3, 3], inn=[3, 2, 1, 2], out=[0, 1, 0, 0], w="ones", aware=(True, False),
                     expect=dict(gated=[0, 1, 3], cent=[0, 1, 2, 3], single=[], beyond=[])),
    # the mask given as confidences, re-cast against FIXED_CONFIDENCE_THRESHOLD (I/utils.py:573-576): 'out' rows lie
    # below it, one of them exactly ON float32(threshold) (`>` leaves it out)
    "float_mask": dict(clean=[3, 3, 0, 0], inn=[3, 2, 0, 0], out=[1, 1, 0, 0], w="ones", aware=(True, False),
                       float_mask=True, expect=dict(gated=[0, 1], cent=[0, 1], single=[], beyond=[])),
}
ECDA_LOSS_TOL = 1e-4
_ECDA = {}


def ecda_case(name):
    """dict(clean [B, H], noisy [Bn, H], yc, pred, mask (bool, or float32 confidences), scores, w) of ECDA_CASES[name],
    rows shuffled; computed once."""
    if name in _ECDA:
        return _ECDA[name]
    t = ECDA_CASES[name]
    rs = np.random.RandomState(sum(map(ord, name)))
    yc = np.repeat(np.arange(C), t["clean"])
    pred = np.concatenate([np.repeat(np.arange(C), t["inn"]), np.repeat(np.arange(C), t["out"])])
    mask = np.concatenate([np.ones(sum(t["inn"]), bool), np.zeros(sum(t["out"]), bool)])
    pc, pn = rs.permutation(len(yc)), rs.permutation(len(pred))
    yc, pred, mask = yc[pc].astype(np.int64), pred[pn].astype(np.int64), mask[pn]
    B, Bn = len(yc), len(pred)
    proto = rs.standard_normal((C, H))
    clean = (proto[yc] + 0.7 * rs.standard_normal((B, H))).astype(F32)
    noisy = (proto[pred] + 0.3 + rs.standard_normal((Bn, H))).astype(F32)
    scores = rs.uniform(0.3, 1.0, Bn).astype(F32)
    w = rs.uniform(0.2, 0.8, C).astype(F32) if t["w"] == "dacp" else np.ones(Bn, F32)
    if t.get("float_mask"):
        thr = F32(cfg()["FIXED_CONFIDENCE_THRESHOLD"])
        conf = np.where(mask, rs.uniform(0.91, 0.99, Bn), rs.uniform(0.5, 0.89, Bn)).astype(F32)
        conf[np.nonzero(~mask)[0][0]] = thr
        mask = conf
    _ECDA[name] = dict(clean=clean, noisy=noisy, yc=yc, pred=pred, mask=mask, scores=scores, w=w, B=B, Bn=Bn)
    return _ECDA[name]


def ecda_bool_mask(k):
    m = np.asarray(k["mask"])
    return m if m.dtype == bool else m > cfg()["FIXED_CONFIDENCE_THRESHOLD"]


def ecda_branches(k):
    """Which branch of the reference's class loop each class of a case takes (see ECDA_CASES' `expect`)."""
    m, n = ecda_bool_mask(k), len(k["w"])
    ns = [int((k["yc"] == c).sum()) for c in range(C)]
    nt = [int(((k["pred"] == c) & m).sum()) for c in range(C)]
    return dict(gated=[c for c in range(min(n, C)) if ns[c] >= 2 and nt[c] >= 2],
                cent=[c for c in range(min(n, C)) if nt[c] > 0],
                single=[c for c in range(min(n, C)) if ns[c] < 2 and nt[c] >= 2],
                beyond=[c for c in range(min(n, C), C) if ns[c] + nt[c] > 0])


_ECDA_REF = {}


def ecda_reference(name, class_aware, drop_class=None):
    """(loss, d/d clean, d/d noisy) by dad_oracle.ecda_loss as it is; computed once.  drop_class: the wrong-answer
    control (that class's noisy members masked out)."""
    key = (name, class_aware, drop_class)
    if key not in _ECDA_REF:
        k = ecda_case(name)
        mask = k["mask"]
        if drop_class is not None:
            mask = ecda_bool_mask(k) & (k["pred"] != drop_class)
        _ECDA_REF[key] = dad_oracle.ecda_loss(k["clean"], k["noisy"], k["yc"], k["pred"], mask,
                                              k["scores"].astype(np.float64), k["w"], cfg(), class_aware,
                                              len(k["w"]) != C)
    return _ECDA_REF[key]


def ecda_loss_ok(got, want):
    return abs(float(got) - want) <= ECDA_LOSS_TOL * max(1.0, abs(want))


# --------------------------------------------------------------------------------------------- encoder
# (B, T) -> valid lengths.  Where B allows: one utterance fully padded (len 0 -> / max(len, 1)), one whose padding
# ends inside a 32-frame slab, one unpadded; T = 1, T on the slab, T one past it.  The padded frames hold grid
# values, not zeros: include/dad.h states no precondition on them.
ENC_GEOMS = [
    ((1, 1), [1]),
    ((1, 32), [32]),
    ((1, 32), [0]),
    ((2, 33), [0, 33]),
    ((5, 64), [0, 64, 40, 32, 1]),
    ((3, 65), [0, 65, 47]),
    ((7, 31), [0, 31, 17, 1, 30, 16, 31]),
]
ENC_LIMIT = (1024, 1)          # DAD_MAX_BATCH utterances of one frame (every 8th fully padded)
ENC_SEED = X.SEED


def enc_id(g):
    (B, T), lens = g
    return "B%dT%d%s" % (B, T, "_allpad" if max(lens) == 0 else "")


def enc_c(B, T):
    """The factor c of the backward bound c u S_g (module docstring)."""
    return B * T + 2


_ENC = {}


def encoder_case(geom):
    """dict(x [B, T, D], pad [B, T] bool, W1, b1, de [B, H], lens) on exact_problem's grid (its generators: problem()
    for x, state() for W1 / b1); de: multiples of 2^-6, |de| <= 4.  Computed once."""
    key = enc_id(geom)
    if key in _ENC:
        return _ENC[key]
    (B, T), lens = geom
    x = X.problem(B, T, Bn=1, Tn=1, seed=ENC_SEED, ragged=False)["xc"]
    W1, b1 = X.state(seed=ENC_SEED)["student"][:2]
    lens = np.asarray(lens)
    pad = np.arange(T)[None, :] >= lens[:, None]
    rs = np.random.RandomState(7 * B + T)
    de = (rs.randint(-256, 257, size=(B, H)) / 64.0).astype(F32)
    _ENC[key] = dict(x=x, pad=pad, W1=W1, b1=b1, de=de, lens=lens, B=B, T=T)
    return _ENC[key]


def limit_geom():
    B, T = ENC_LIMIT
    return (ENC_LIMIT, [0 if b % 8 == 3 else 1 for b in range(B)])


def encoder_reference(k, lens_with_padding=False, act=None):
    """float64 forward and weight gradient of a case: dict(pre, act, vlen, e, dW1, S_W1, db1, S_b1).  The two
    wrong-answer controls: lens_with_padding pools over T frames; `act` replaces the ReLU' pattern."""
    pre = X.preact64(k["x"], k["W1"], k["b1"])
    valid = ~k["pad"]
    a = ((pre > 0) & valid[..., None]) if act is None else act
    vlen = valid.sum(1).astype(np.float64)
    if lens_with_padding:
        vlen = np.full(len(vlen), float(k["T"]))
    e = np.where(a, pre, 0.0).sum(1) / np.maximum(vlen, 1.0)[:, None]
    dW, S, db, Sb = X.wgrad64(k["x"], a, vlen, k["de"])
    return dict(pre=pre, act=a, vlen=vlen, e=e, dW1=dW, S_W1=S, db1=db, S_b1=Sb)


def act_whole_last_slab(k):
    """The ReLU' pattern of a backward that keeps every frame of an utterance's last slab (padding that ends inside
    a slab ignored)."""
    pre = X.preact64(k["x"], k["W1"], k["b1"])
    upto = np.minimum((k["lens"] + SLAB - 1) // SLAB * SLAB, k["T"])
    return (pre > 0) & (np.arange(k["T"])[None, :] < upto[:, None])[..., None]


def enc_forward_ratio(e, ref, T):
    return worst(np.asarray(e, np.float64) - ref["e"], X.bound("e", None, T) * np.abs(ref["e"]))


def enc_backward_ratios(dW1, db1, ref, B, T):
    lim = enc_c(B, T) * U32
    return (worst(np.asarray(dW1, np.float64) - ref["dW1"], lim * ref["S_W1"]),
            worst(np.asarray(db1, np.float64) - ref["db1"], lim * ref["S_b1"]))


# -------------------------------------------------------------------------------------------- augment
AUG_SHAPES = [(1, 1, 1), (3, 5, 7), (2, 33, 768), (1, 40, 768), (4, 1, 768)]     # (1, 40, 768) is given as [40, 768]
AUG_2D = (1, 40, 768)


def augment_case(shape, seed=31):
    """(x, nw, ns, u, start) of one [B, T, D] shape, start drawn as the reference draws it (I/utils.py:370)."""
    B, T, Dd = shape
    rs = np.random.RandomState(seed + B * T * Dd)
    x = rs.standard_normal(shape).astype(F32)
    nw = rs.standard_normal(shape).astype(F32)
    ns = rs.standard_normal(shape).astype(F32)
    u = rs.uniform(size=Dd).astype(F32)
    mlen = synth.temporal_mask_len(T, cfg()["TEMPORAL_MASK_RATIO"])
    start = rs.randint(0, max(1, T - mlen + 1), size=B).astype(np.int64)
    return x, nw, ns, u, start
