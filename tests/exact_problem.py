"""Synthetic DAD steps whose encoder operands are exactly representable in fp16 AND bf16, with a float64
reference and an error bound derived from the reference alone (TEST INFRASTRUCTURE; imports oracle/ only, and
tests/scl_ref.py when a case switches the supervised-contrastive term on).

Why: on random inputs a 16-bit forward flips ReLU' decisions of pre-activations near 0 and each flip moves a
whole row of dW1 (gpu_harness.close_grad), so no tolerance separates "rounding" from "wrong".  Here the
discrete decisions cannot differ between the modes, and the only rounding a 16-bit step adds is known.

The grid (every value a dyadic rational):
  features xc, xn     multiples of 2^-3, |x| < 17
  draws               nw = clip(round(nw), -3, 3), ns = clip(round(2 ns), -6, 6), with
                      WEAK_NOISE_STD = STRONG_NOISE_STD = 2^-3: the noise and x + noise stay on the 2^-3 grid
                      below 32 in magnitude, i.e. 8 significant bits (the bf16 significand)
  feature / temporal masks multiply by 0 or 1
  W1 (student, teacher)  multiples of 2^-10, |w| < 0.05: 6 bits
  b1 (student, teacher)  ODD multiples of 2^-14
  W2, b2, Adam moments, tau, Q: as oracle/synth.make_state gives them
Every product is a multiple of 2^-13 and every pre-activation an odd multiple of 2^-14: never 0, and with
sum|x||w| + |b| < 2^24 * 2^-14 = 1024 every partial sum is exact in fp32 in any order.  So the pre-activations,
and with them the ReLU' pattern, are the same numbers in float64, in fp32 with any summation order and on fp16 /
bf16 operands with fp32 accumulation (tests/test_exact_problem_cpu.py checks each of these conditions).

Bounds (u = 2^-24, the fp32 unit roundoff; S_x = the reference's sum with every term replaced by its magnitude):
  gradients   |g - g_ref| <= (eps_op + n_rows u + 1e-4) S_g elementwise, n_rows = Bc Tc + Bn Tn.
              eps_op: the weight gradient rounds the per-(utterance, h) scale dL/de / len once to the operand
              type (fp16: after an exact power-of-two scale, csrc/wgrad_direct.h; x is exact): 0 for fp32, 2^-11
              for fp16, 2^-8 for bf16, and 0 for db1, dW2, db2, which are fp32 sums in every mode.  n_rows u is
              the worst-case fp32 accumulation error.  1e-4 is the project's fp32 gradient bound
              (gpu_harness.close_grad's tol_norm) standing in for the fp32 tail's error in dL/de: plain fp32
              autograd (oracle/torch_cpu.TorchCPUStep) against this reference measures err / S_W1 of at most
              4.5e-5 on these problems (test_exact_problem_cpu.py prints its own figure).
  tail term   dW1 only, added to the bound above.  S_W1 weighs |dL/de|, but the classifier backward cancels twice
              on the way to dL/de_u[h] = k_uh sum_c gz_uc W2[c][h] (k = keep / (1 - p)): in gz_uc = coef_u (p_uc -
              q_uc) (student and teacher softmax nearly agree once the consistency loss is small; clean: p - the
              smoothed target) and in the sum over the classes.  Where both cancel (B1T1/Bn2Tn3, h = 154: sum_c
              (p + q)|W2| k coef = 2300 |dL/de|) the fp32 roundings of p and q alone reach 1e-4 |dL/de|, in ANY
              fp32 evaluation: plain fp32 autograd sits at 0.45 of the bound without this term there, the fused
              step's fp32 mode measured 1.26 on MI355X (an element no clean row reaches).  Derived: logits within the
              logit bound below, |dz| <= eps_z = (T + H + 8) u max_c zS, move a softmax probability by at most
              2 eps_z p (dp_c = p_c (dz_c - sum_j p_j dz_j)), and exp (its argument's rounding is below eps_z),
              the sum over C classes and the division add (C + 6) u p; the product with coef, the C-term sum with
              W2 and the factor k add (C + 4) u |gz| |W2|.  So
                |d(dL/de_u[h])| <= k_uh sum_c [coef_u (p_uc r_s + q_uc r_t) + (C + 4) u |gz_uc|] |W2[c][h]|,
                r = 2 eps_z + (C + 6) u   (clean: coef = 1 / Bc, q's term absent: the target is exact)
              and the tail term is this in place of |dL/de| in S_W1.  (The ECDA part of dL/de stays under the
              1e-4.)  It is a worst case (eps_z allows the logits H roundings): median 0.5 - 1 % of S_W1 at the two
              small geometries, 5e-5 S_W1 at the three larger ones, and every wrong gradient of
              test_exact_problem_cpu.py still lies 10x outside.  db1, dW2, db2 keep the bound without it.
  embeddings |e - e_ref| <= (T + 2) u |e_ref|: the pooled terms are exact and non-negative, so only the fp32
              sum and one division round.
  logits      |z - z_ref| <= (T + H + 8) u (|d_ref| |W2|^T + |b2|), d = the dropout-scaled embedding.
  contrastive term   (cases with TARGET_SCL_WEIGHT > 0 past max(WARMUP_EPOCHS, SCL_START_EPOCH), ConfigView.scl_weight's
              rule; tests/test_gpu_exact_scl.py.)  The oracle has no such term.  The reference adds the float64
              definition (scl_ref.scl_autograd, cross-checked against scl_ref.scl_closed_form) on its OWN pre-dropout
              float64 embeddings: clean rows with yc, strong rows with the oracle's pred, members = every clean row and
              the strong rows with mask != 0.  w_scl g_u joins each branch's dL/de before the weight-gradient sum, so dW1
              and db1 move and dW2, db2 do not; S_W1 and S_b1 add |base| and w_scl |g| WITHOUT cancellation between
              them; the expected total loss is the oracle's plus w_scl x loss.  dad_scl evaluates the term in fp32, and
              its error is no fraction of S (the term's own gradient cancels), so dW1 and db1 gain an allowance that
              enters the way the tail term does: through wgrad64_scaled's magnitude sum with, in place of |dL/de|, per
              element of a member row
                w_scl (1e-4 max |g| + 4 d),
              1e-4 max |g| being the project's own bound on dad_scl's gradient (tests/test_gpu_scl.py's TOL in
              gpu_harness.close's measure) and d its sensitivity to the embeddings it is fed, which are fp32 and may
              differ from the float64 ones by (T + 2) u |e|.  d is measured on the reference, never on a kernel: the
              largest change of any element of the float64 g under three seeded sign patterns of e (1 +- (T + 2) u) and
              under the embeddings of a float32 restatement of the pooling (pool32); 4x is the factor
              tests/test_gpu_domain_gap.py puts on a measured sensitivity.  Measured 4 d / (1e-4 max |g|): 0.40 at
              B5T33/Bn7Tn31, 0.50 at B16T64/Bn16Tn64, 0.51 at B12T45/Bn20Tn70, 0.39 at B64T40/Bn64Tn40, 0.26 at
              B65T33/Bn66Tn31 and 4.2 at L1 (T = 544 / 577: the rows are nearly parallel, 1 / tau = 10 and (T + 2) u =
              3.4e-5): never below a tenth of the first part, so it stays in.  With no anchor (B1T1/Bn2Tn3: three
              members of three classes) g = 0, the allowance is 0 and the bounds are the weight-0 step's.  The float32
              restatement of the whole route sits at most 0.02 of the fp32 bound, and the term dropped, overwriting the
              ECDA part, or with wrong members, labels, embeddings, normalisation backward, temperature, mean or input
              lies at least 22x outside the bf16 bound (test_exact_problem_cpu.py asserts 10x and prints each factor).
              The term's median share of S_W1 is 0.036 - 0.038 with ECDA on at weight 1 (0.027 at B64T40/Bn64Tn40,
              hence weight 2 there: SCL_WEIGHT) and 0.78 - 0.88 where ECDA is off.
The forward bounds hold for ALL three precisions: the 16-bit conversion is lossless on these inputs, so a 16-bit
forward that differs from the fp32 one beyond summation order is a bug.

Long problems (LONG_GEOMS, long_problem; tests/test_gpu_long_utterances.py).  GEOMS stops at T = 70; the step's pooling
sums slab partials in batches of 16 (csrc/pool.h) and its 16-bit weight gradient takes 21 splits until the slab list
passes 21 x 64 (csrc/dad_common.h), so utterances past 512 frames and lists past 1344 slabs run code no GEOMS entry
reaches.  The same grid, bounds and reference serve there (sum|x||w| + |b| stays far below 1024); three things are added:
  lengths     given per utterance, not drawn (which frame an utterance ends on is what the cases are about)
  sentinels   The bound is a fraction of S, the magnitude sum over ALL rows: n_rows u alone is 2.7e-3 S at 16 x 1400
              frames per side, while one slab of 1408 carries 7e-4 S.  Past about 100 slabs a dropped or doubled slab
              therefore passes.  So channels 640 .. 767 hold values only in the frames of the weight-gradient slabs s
              (dad_wg_total's order: clean slabs, then strong ones, padded slabs counted) with s mod 128 == channel -
              640: xc and xn non-zero multiples of 2^-3 in +-[1/8, 2] with one sign per slab, the draws nw and ns
              as drawn, all four 0 there in every other slab, and u = 1 there, so the feature mask keeps the channels.
              S of a sentinel column then covers 1 slab in 128, and a lost slab lies at least 10x outside the fp16
              bound (test_exact_problem_cpu.py asserts it for every loud slab and prints the least factor).
  mislabel    A clean utterance the student classifies confidently has dL/de near 0, and the tail term then dominates
              its slabs' S.  Shifting every clean label by one makes dL/de of order 1 (L3).
L3's mask has to hold both values while the noisy utterances in which a 64-slab split begins or ends are masked in:
its noisy utterances' noise levels and classes are given too (_L3_NOISE, _L3_LABELS).
"""
import numpy as np

from oracle import dad_oracle, synth

SEED = 3                       # problem seed = weight seed
# DACP thresholds of the seeded state (synth.make_state's tau_range).  TAU_RANGE: the gates open (mask sum >= 2)
# and the mask holds zeros and ones at every geometry with Bn >= 7, every certainty score at least 0.07 away
# from its threshold.  A batch of two noisy utterances cannot do both, so it takes the low thresholds, under which
# every utterance is masked in (test_exact_problem_cpu.py checks all of this).
TAU_RANGE = (0.6, 0.94)
TAU_RANGE_OPEN = (0.05, 0.3)
U32 = 2.0 ** -24
EPS_OP = {"fp32": 0.0, "fp16": 2.0 ** -11, "bf16": 2.0 ** -8}
TAIL_TOL = 1e-4                # gpu_harness.close_grad's tol_norm
SCL_TOL = 1e-4                 # tests/test_gpu_scl.py's TOL for dad_scl's gradient, in gpu_harness.close's measure
SCL_SENS_FACTOR = 4.0          # on a measured sensitivity, as tests/test_gpu_domain_gap.py takes it
SCL_ON = dict(TARGET_SCL_WEIGHT=1.0, SCL_START_EPOCH=0, SCL_TEMPERATURE=0.1)
# ... but for B64T40/Bn64Tn40, where weight 1 gives the term a median 0.027 of S_W1 with ECDA on: below the 0.03 the
# CPU module asks for, so the weight is raised there (0.052)
SCL_WEIGHT = {"B64T40_Bn64Tn40": 2.0}
# tests/test_gpu_parity.EDGE (the GPU module asserts they are the same)
GEOMS = [
    dict(B=1, T=1, Bn=2, Tn=3),
    dict(B=5, T=33, Bn=7, Tn=31),
    dict(B=16, T=64, Bn=16, Tn=64),
    dict(B=12, T=45, Bn=20, Tn=70, ragged=False),
    dict(B=64, T=40, Bn=64, Tn=40),
]
# Past 64 utterances a side (the general tail, dad_tail_ecda; 131 candidate rows for dad_scl: a third row tile and a
# second column chunk).  Not one of test_gpu_parity's; tests/test_gpu_exact_scl.py runs it.
PAST64 = dict(B=65, T=33, Bn=66, Tn=31)


SENT0, SENT_N = 640, 128       # the sentinel channels 640 .. 767 of the long problems (long_problem)


def _ragged_lengths(seed, n, lo=700, hi=1400, pins=()):
    """n seeded lengths in [lo, hi], each = 16 .. 31 mod 32 (so every last slab holds at least 16 frames);
    `pins`: (utterance, smallest length) pairs, for the utterances a split boundary of L3 falls in."""
    rs = np.random.RandomState(seed)
    lens = 32 * rs.randint((lo + 31) // 32, hi // 32, size=n) + rs.randint(16, 32, size=n)
    for u, least in pins:
        while lens[u] < least:
            lens[u] += 32
        lens[u] = min(lens[u], hi)
    assert lens.min() >= lo and lens.max() <= hi and np.all(lens % 32 >= 16)
    return tuple(int(v) for v in lens)


# L3's 64-slab splits start and end in utterances 0, 1, 2, 4, 5, 7, 8, 10, 11, 13, 14, 15 of either list (44 slabs
# per utterance): these lengths keep the boundary slabs live, and utterance 15 has every frame.
_L3_PINS = ((2, 1304), (5, 1176), (8, 1048), (11, 920), (14, 792), (15, 1400))
# ... and those twelve noisy utterances must be masked in for their strong slabs to carry a gradient, while the mask
# is to hold both values: noisy utterances 3, 6, 9 and 12 are loud (noise level 2.5) members of class 2, whose seeded
# threshold (0.90) none of them reaches; the twelve are quiet (0.5) members of the classes 0, 1 and 3.
_L3_OUT = (3, 6, 9, 12)
_L3_NOISE = tuple(2.5 if u in _L3_OUT else 0.5 for u in range(16))
_L3_LABELS = (0, 1, 3, 2, 0, 1, 2, 3, 0, 2, 1, 3, 2, 0, 1, 3)
# The long problems (explicit lengths; module docstring "Long problems").
LONG_GEOMS = [
    dict(id="L1", B=2, T=544, Bn=3, Tn=577, lens_c=(544, 200), lens_n=(577, 512, 31), sentinel=True, tau="open"),
    dict(id="L2", B=2, T=1056, Bn=2, Tn=1025, lens_c=(1056, 513), lens_n=(1025, 1000), sentinel=True, tau="open"),
    dict(id="L3", B=16, T=1400, Bn=16, Tn=1400, lens_c=_ragged_lengths(41, 16, pins=_L3_PINS),
         lens_n=_ragged_lengths(42, 16, pins=_L3_PINS), sentinel=True, mislabel=True, noise_n=_L3_NOISE,
         labels_n=_L3_LABELS),
    dict(id="S1", B=32, T=32, Bn=32, Tn=32, lens_c=tuple(int(v) for v in np.random.RandomState(43).permutation(32) + 1),
         lens_n=tuple(int(v) for v in np.random.RandomState(44).permutation(32) + 1)),
]
LONG = {g["id"]: g for g in LONG_GEOMS}
S1_PLUS = dict(LONG["S1"], id="S1plus", B=33, lens_c=LONG["S1"]["lens_c"] + (17,))


def geom_id(g):
    return g["id"] if "id" in g else "B%dT%d_Bn%dTn%d" % (g["B"], g["T"], g["Bn"], g["Tn"])


def scl_over(geom, ecda=True, weight=None):
    """The settings of a case with the contrastive term on, beside cfg(): SCL_ON with the geometry's weight (or
    `weight`), and USE_ECDA=False where asked.  Both the reference (case) and the step under test take them."""
    over = dict(SCL_ON, TARGET_SCL_WEIGHT=SCL_WEIGHT.get(geom_id(geom), 1.0) if weight is None else float(weight))
    if not ecda:
        over["USE_ECDA"] = False
    return over


def q(a, step):
    """Round to the nearest multiple of `step` (a power of two), as float32."""
    return (np.round(np.asarray(a, np.float64) / step) * step).astype(np.float32)


def cfg():
    return dad_oracle.make_cfg("iemocap", WEAK_NOISE_STD=2.0 ** -3, STRONG_NOISE_STD=2.0 ** -3)


def problem(B, T, Bn=None, Tn=None, seed=SEED, ragged=True):
    """test_gpu_parity._problem's inputs (independent clean / noisy geometry) on the dyadic grid."""
    Bn = B if Bn is None else Bn
    Tn = T if Tn is None else Tn
    P = synth.init_weights(seed)[4]
    xc, mc, yc = synth.make_batch(P, seed * 11 + 1, B, T, ragged=ragged)
    xn, mn, yn = synth.make_batch(P, seed * 11 + 2, Bn, Tn, snr_db=5.0, noisy=True, ragged=ragged, label_shift=1)
    dr = synth.make_draws(seed * 11 + 3, Bn, Tn)
    dr["keep1"] = synth.make_draws(seed * 11 + 4, B, 1)["keep1"]
    dr["nw"] = np.clip(np.round(dr["nw"]), -3, 3).astype(np.float32)
    dr["ns"] = np.clip(np.round(2.0 * dr["ns"]), -6, 6).astype(np.float32)
    return dict(xc=q(xc, 2.0 ** -3), mc=mc, yc=yc, xn=q(xn, 2.0 ** -3), mn=mn, yn=yn, **dr)


def _batch_of(P, seed, lens, T, noisy, label_shift, noise=None, classes=None):
    """synth.make_batch with the lengths given, not drawn: features on the 2^-3 grid with |x| < 17, pads 0.
    `noise`, `classes`: the noisy utterances' noise levels and classes, where given (make_batch draws the levels
    from U(0.5, 2.5) and shuffles the classes; the draws are made either way, so the stream stays the same)."""
    rs = np.random.RandomState(seed)
    B = len(lens)
    labels = (np.arange(B) + label_shift) % P.shape[0]
    rs.shuffle(labels)
    if classes is not None:
        labels = np.asarray(classes, np.int64)
    level = rs.uniform(0.5, 2.5, size=(B, 1, 1))
    if noise is not None:
        level = np.asarray(noise, np.float64).reshape(B, 1, 1)
    sigma = 0.5 + (10.0 ** (-5.0 / 20.0) * level if noisy else 0.0)
    x = P[labels][:, None, :] + (sigma * rs.standard_normal(size=(B, T, P.shape[1]))).astype(np.float32)
    x = np.clip(q(x, 2.0 ** -3), -16.875, 16.875)
    pad = np.arange(T)[None, :] >= np.asarray(lens)[:, None]
    x[pad] = 0.0
    return x, pad, labels.astype(np.int64)


def wg_slab(B, T, Bn, Tn, noisy, b, c):
    """Weight-gradient slab number of 32-frame slab c of utterance b (csrc/dad_common.h dad_wg_total's order:
    the clean slabs, then the strong ones; padded slabs count)."""
    ncc, ncn = (T + 31) // 32, (Tn + 31) // 32
    return B * ncc + b * ncn + c if noisy else b * ncc + c


def _sentinels(a, first_slab, rs=None):
    """Apply the sentinel rule to [B, T, D] array `a` in place: channel SENT0 + s mod SENT_N is zero outside the
    frames of the slabs numbered s (utterance b's slab c is first_slab + b * ceil(T / 32) + c).  With `rs`,
    the slab's own channel is redrawn as non-zero multiples of 2^-3 in +-[1/8, 2], one sign per slab; without,
    it is kept."""
    B, T, _ = a.shape
    nc = (T + 31) // 32
    own = SENT0 + (first_slab + np.arange(B)[:, None] * nc + np.arange(T)[None, :] // 32) % SENT_N      # [B, T]
    bi, ti = np.arange(B)[:, None], np.arange(T)[None, :]
    if rs is None:
        keep = a[bi, ti, own]
    else:
        sign = np.repeat(rs.choice([-1.0, 1.0], size=(B, nc)), 32, axis=1)[:, :T]      # (one per slab: no cancelling)
        keep = (rs.randint(1, 17, size=(B, T)) * sign * 2.0 ** -3).astype(a.dtype)
    a[:, :, SENT0:SENT0 + SENT_N] = 0
    a[bi, ti, own] = keep


def long_problem(B, T, Bn, Tn, lens_c, lens_n, seed=SEED, sentinel=False, mislabel=False, noise_n=None, labels_n=None):
    """problem() with explicit lengths per utterance (one of them the padded length), and optionally
      sentinel   channels 640 .. 767 hold values only in the frames of the weight-gradient slabs s with
                 s mod 128 == channel - 640 (xc, xn: non-zero multiples of 2^-3 in +-[1/8, 2]; nw, ns: their
                 draws); xc, xn, nw and ns are 0 there in every other slab, and u = 1 keeps the channels
      mislabel   every clean label shifted by one, so that dL/de of the clean rows is of order 1"""
    assert len(lens_c) == B and max(lens_c) == T and len(lens_n) == Bn and max(lens_n) == Tn and min(lens_c + lens_n) >= 1
    P = synth.init_weights(seed)[4]
    xc, mc, yc = _batch_of(P, seed * 11 + 1, lens_c, T, False, 0)
    xn, mn, yn = _batch_of(P, seed * 11 + 2, lens_n, Tn, True, 1, noise_n, labels_n)
    dr = synth.make_draws(seed * 11 + 3, Bn, Tn)
    dr["keep1"] = synth.make_draws(seed * 11 + 4, B, 1)["keep1"]
    dr["nw"] = np.clip(np.round(dr["nw"]), -3, 3).astype(np.float32)
    dr["ns"] = np.clip(np.round(2.0 * dr["ns"]), -6, 6).astype(np.float32)
    if sentinel:
        rs = np.random.RandomState(seed * 11 + 5)
        _sentinels(xc, 0, rs)
        _sentinels(xn, wg_slab(B, T, Bn, Tn, True, 0, 0), rs)
        xc[mc] = 0.0
        xn[mn] = 0.0
        for k in ("nw", "ns"):
            _sentinels(dr[k], wg_slab(B, T, Bn, Tn, True, 0, 0))
        dr["u"][SENT0:SENT0 + SENT_N] = 1.0
    if mislabel:
        yc = (yc + 1) % synth.N_CLS
    return dict(xc=xc, mc=mc, yc=yc, xn=xn, mn=mn, yn=yn, **dr)


def tau_range(Bn):
    return TAU_RANGE if Bn > 2 else TAU_RANGE_OPEN


def state(seed=SEED, step=1, tau_range=TAU_RANGE):
    st = synth.make_state(seed, step, tau_range=tau_range)
    for net in ("student", "teacher"):
        W1, b1, W2, b2 = st[net]
        st[net] = [q(W1, 2.0 ** -10), (q(b1, 2.0 ** -13) + np.float32(2.0 ** -14)).astype(np.float32), W2, b2]
    return st


def augmented(inp, c):
    """(weak, strong) inputs of the noisy batch, as the oracle's step builds them."""
    xw = dad_oracle.weak_augment(inp["xn"], inp["nw"], c["WEAK_NOISE_STD"])
    xs = dad_oracle.strong_augment(inp["xn"], inp["ns"], inp["u"], inp["start"], c["STRONG_NOISE_STD"],
                                   c["DROPOUT_RATE"], c["TEMPORAL_MASK_RATIO"])
    return xw, xs


def preact64(x, W1, b1):
    """Pre-activations [B, T, H] in float64 (exact on the grid)."""
    B, T, D = x.shape
    return (x.reshape(B * T, D).astype(np.float64) @ np.asarray(W1, np.float64).T).reshape(B, T, -1) \
        + np.asarray(b1, np.float64)


def wgrad64(x, act, vlen, g, lens=None):
    """float64 dW1[h][d] = sum_u g_u[h] / max(1, len_u) * sum_{rows of u active at h} x[row][d], db1 likewise,
    and their abs-sums (|g|, |x|): (dW1, S_W1, db1, S_b1).  `lens` overrides vlen (the len + 1 mutant)."""
    scale = np.asarray(g, np.float64) / np.maximum(np.asarray(vlen if lens is None else lens, np.float64), 1.0)[:, None]
    return wgrad64_scaled(x, act, scale)


def wgrad64_scaled(x, act, scale, abs_scale=None):
    """wgrad64 from the per-(utterance, h) scales themselves (the simulated 16-bit rounding feeds these)."""
    B, T, D = x.shape
    H = act.shape[2]
    abs_scale = np.abs(scale) if abs_scale is None else abs_scale
    dW, S = np.zeros((H, D)), np.zeros((H, D))
    db, Sb = np.zeros(H), np.zeros(H)
    for u in range(B):
        a = act[u].astype(np.float64).T                    # [H, T]
        xu = x[u].astype(np.float64)
        dW += scale[u][:, None] * (a @ xu)
        S += abs_scale[u][:, None] * (a @ np.abs(xu))
        n = a.sum(1)
        db += scale[u] * n
        Sb += abs_scale[u] * n
    return dW, S, db, Sb


def _pool64(x, pad, W1, b1):
    pre = preact64(x, W1, b1)
    valid = ~pad
    act = (pre > 0) & valid[..., None]
    vlen = valid.sum(1).astype(np.float64)
    e = np.where(act, pre, 0.0).sum(1) / np.maximum(vlen, 1.0)[:, None]
    return e, act, vlen


def _softmax_err(zS, T):
    """Relative error [B] of an fp32 softmax probability of logits that meet the logit bound (tail term)."""
    return 2.0 * bound("z", None, T) * zS.max(1) + (synth.N_CLS + 6) * U32


def _logits64(e, W2, b2, keep, p):
    d = e if keep is None else e * (keep.astype(np.float64) / (1.0 - p))
    W2, b2 = np.asarray(W2, np.float64), np.asarray(b2, np.float64)
    return d @ W2.T + b2, d, np.abs(d) @ np.abs(W2).T + np.abs(b2)


def scl_weight(c, epoch):
    """The supervised-contrastive term's weight at `epoch` (ConfigView.scl_weight's rule; the oracle's settings have
    no such keys unless a case adds them)."""
    if epoch < max(c["WARMUP_EPOCHS"], c.get("SCL_START_EPOCH", 0)):
        return 0.0
    return float(c.get("TARGET_SCL_WEIGHT", 0.0))


def scl_inputs(inp, r, e_clean, e_strong):
    """(embeddings [Bc + Bn, H], classes, member flags) of the term: every clean row with its label, then the strong
    rows with the oracle's pseudo-labels, flagged where the DACP mask lets them in."""
    emb = np.concatenate([e_clean, e_strong], 0)
    labels = np.concatenate([np.asarray(inp["yc"], np.int64), np.asarray(r["pred"], np.int64)])
    member = np.concatenate([np.ones(len(inp["yc"]), np.uint8), (np.asarray(r["mask"]) != 0).astype(np.uint8)])
    return emb, labels, member


def scl_perturbed(emb, T_rows, seed):
    """`emb` with every element moved to the embedding bound, e (1 +- (T + 2) u), the signs seeded."""
    sign = np.random.RandomState(seed).choice([-1.0, 1.0], size=emb.shape)
    return emb * (1.0 + sign * ((np.asarray(T_rows, np.float64) + 2.0) * U32)[:, None])


def pool32(x, pad, W1, b1):
    """The pooled encoder restated in float32: exact pre-activations, a float32 sum over the frames in order and one
    division."""
    pre = preact64(x, W1, b1).astype(np.float32)
    act = (pre > 0) & ~pad[..., None]
    vlen = np.maximum((~pad).sum(1), 1).astype(np.float32)
    return np.cumsum(np.where(act, pre, np.float32(0)), axis=1, dtype=np.float32)[:, -1] / vlen[:, None]


def _add_scl(ref, inp, st, c, w):
    """The supervised-contrastive term on top of the rebuilt step `ref` (module docstring, "contrastive term"): the
    float64 definition on the reference's own pre-dropout embeddings, w dL_scl/de added to each branch's dL/de
    before the weight-gradient sums, the magnitude sums and the allowance added beside the base's."""
    import scl_ref
    W1, b1 = st["student"][:2]
    tau = c.get("SCL_TEMPERATURE", 0.1)
    pc, ps = ref["parts"]["clean"], ref["parts"]["strong"]
    Bc = pc["x"].shape[0]
    emb, labels, member = scl_inputs(inp, ref["oracle"], ref["e"]["e_clean"], ref["e"]["e_strong"])
    loss, g = scl_ref.scl_autograd(emb, labels, member, tau)
    loss_cf, g_cf = scl_ref.scl_closed_form(emb, labels, member, tau)
    stats = scl_ref.stats(emb, labels, member)
    gmax = float(np.abs(g).max())
    # sensitivity to the embeddings' own fp32 error, measured on the reference: the float64 term on embeddings moved
    # to the embedding bound and on the float32 restatement's
    T_rows = np.concatenate([np.full(Bc, ref["T"]["e_clean"]), np.full(len(emb) - Bc, ref["T"]["e_strong"])])
    others = [scl_perturbed(emb, T_rows, s) for s in (0, 1, 2)]
    others.append(np.concatenate([pool32(pc["x"], inp["mc"], W1, b1), pool32(ps["x"], inp["mn"], W1, b1)], 0).astype(np.float64))
    moved = max(float(np.abs(scl_ref.scl_autograd(e2, labels, member, tau)[1] - g).max()) for e2 in others)
    allow = np.zeros(len(emb))
    allow[scl_ref.members(emb, labels, member)] = w * (SCL_TOL * gmax + SCL_SENS_FACTOR * moved)
    dW1, db1 = ref["grads"][0].copy(), ref["grads"][1].copy()
    S1, Sb1 = ref["S"][0].copy(), ref["S"][1].copy()
    S_term, tail, tail_b1 = np.zeros_like(S1), ref["tail"].copy(), np.zeros_like(Sb1)
    for p, rows in ((pc, slice(0, Bc)), (ps, slice(Bc, None))):
        n = np.maximum(p["vlen"], 1.0)[:, None]
        tW, tS, tb, tSb = wgrad64_scaled(p["x"], p["act"], w * g[rows] / n)
        aS, aSb = wgrad64_scaled(p["x"], p["act"], allow[rows, None] / n * np.ones((1, g.shape[1])))[1::2]
        dW1, db1, S1, Sb1, S_term = dW1 + tW, db1 + tb, S1 + tS, Sb1 + tSb, S_term + tS
        tail, tail_b1 = tail + aS, tail_b1 + aSb
    with np.errstate(divide="ignore", invalid="ignore"):
        share = float(np.median((S_term / S1)[S1 > 0])) if stats["V"] else 0.0
    ref["scl"] = dict(w=w, tau=tau, loss=loss, g=g, loss_closed=loss_cf, g_closed=g_cf, V=stats["V"],
                      members=stats["members"], anchors=stats["anchors"], allow=allow,
                      sensitivity=SCL_SENS_FACTOR * moved / (SCL_TOL * gmax) if gmax > 0 else 0.0,
                      base=dict(clean=pc["g"], strong=ps["g"]), labels=labels, member=member, S_term=S_term, share=share)
    ref["parts"] = dict(ref["parts"], clean=dict(pc, g=pc["g"] + w * g[:Bc]), strong=dict(ps, g=ps["g"] + w * g[Bc:]))
    ref["grads"] = [dW1, db1] + ref["grads"][2:]
    ref["S"] = [S1, Sb1] + ref["S"][2:]
    ref["tail"], ref["tail_b1"] = tail, tail_b1
    ref["total_loss"] = ref["oracle"]["total_loss"] + w * loss
    return ref


def reference(inp, st, c, epoch):
    """One DADOracle.step from state `st`, then the float64 rebuild.  Returns a dict:
      oracle   the oracle's own output (losses, mask, fp32 grads, ...)
      grads    [dW1, db1, dW2, db2] float64;  S: their abs-sums;  tail: dW1's tail term [H, D]
      strong   the strong branch's share (dW1, S_W1) (zeros in the warm-up)
      e, z     float64 embeddings / logits by name (e_clean, ...);  zS: the logit bound's magnitude sum
      T        the padded length behind each e_* / z_* name;  n_rows = Bc Tc + Bn Tn
      parts    what the gradient was built from (x, act, vlen, g per branch), for the CPU module's mutants
    With the supervised-contrastive term on (scl_weight(c, epoch) > 0) the gradients, S, tail and parts include it,
    and the dict also holds
      scl      loss, g [Bc + Bn, H] (dL_scl/de, unweighted), w, tau, V, members, anchors [4], loss_closed / g_closed
               (scl_ref.scl_closed_form beside the autograd), allow [Bc + Bn] (the per-row allowance, weighted),
               sensitivity (the allowance's second part over its first), base (the branches'
               dL/de without the term), S_term (the term's part of S_W1) and share (its median share of S_W1)
      tail_b1  db1's allowance for the term [H];  total_loss: the oracle's plus w x loss"""
    W1, b1, W2, b2 = st["student"]
    orc = dad_oracle.DADOracle(W1, b1, W2, b2, c)
    orc.load_state(st)
    r = orc.step(inp, epoch)
    p = c["DROPOUT_RATE"]
    warm = dad_oracle.loss_weights(c, epoch)[2]
    w_kl = dad_oracle.loss_weights(c, epoch)[0]
    C = len(b2)
    Bc, Tc = inp["mc"].shape
    Bn, Tn = inp["mn"].shape
    e, z, zS, T = {}, {}, {}, {}
    ec, act_c, vlen_c = _pool64(inp["xc"], inp["mc"], W1, b1)
    zc, dc, zSc = _logits64(ec, W2, b2, inp["keep1"], p)
    e["e_clean"], z["z_clean"], zS["z_clean"] = ec, zc, zSc
    T["e_clean"] = T["z_clean"] = Tc
    eps = c["LABEL_SMOOTHING_FACTOR"] if c["USE_LABEL_SMOOTHING"] else 0.0
    pc = dad_oracle.softmax(zc)
    gzc = (pc - (1 - eps) * np.eye(C)[inp["yc"]] - eps / C) / Bc
    parts = {"clean": dict(x=inp["xc"], act=act_c, vlen=vlen_c, g=np.asarray(r["e_clean_grad"], np.float64))}
    dW1, S1, db1, Sb1 = wgrad64(**parts["clean"])
    kc = inp["keep1"].astype(np.float64) / (1.0 - p)
    aW2 = np.abs(np.asarray(W2, np.float64))
    # fp32 error of the classifier backward's dL/de (module docstring, "tail term")
    tail_c = ((pc * _softmax_err(zSc, Tc)[:, None] / Bc + (C + 4) * U32 * np.abs(gzc)) @ aW2) * kc
    tail = wgrad64_scaled(inp["xc"], act_c, tail_c / np.maximum(vlen_c, 1.0)[:, None])[1]
    dW2, S2 = gzc.T @ dc, np.abs(gzc).T @ np.abs(dc)
    db2, Sb2 = gzc.sum(0), np.abs(gzc).sum(0)
    strong = (np.zeros_like(dW1), np.zeros_like(S1))
    if not warm:
        xw, xs = augmented(inp, c)
        Wt1, bt1, Wt2, bt2 = st["teacher"]
        et = _pool64(xw, inp["mn"], Wt1, bt1)[0]
        zt, _, zSt = _logits64(et, Wt2, bt2, None, p)
        es, act_s, vlen_s = _pool64(xs, inp["mn"], W1, b1)
        zs, ds, zSs = _logits64(es, W2, b2, inp["keep2"], p)
        e.update(e_teacher=et, e_strong=es)
        z.update(z_teacher=zt, z_strong=zs)
        zS.update(z_teacher=zSt, z_strong=zSs)
        for k in ("e_teacher", "e_strong", "z_teacher", "z_strong"):
            T[k] = Tn
        maskf = np.asarray(r["mask"], np.float64)
        msum = maskf.sum()
        gzs = np.zeros((Bn, C))
        tail_s = np.zeros((Bn, len(b1)))
        if msum > 1:
            coef = w_kl * maskf / (msum + 1e-8)
            ps, qt = dad_oracle.softmax(zs), dad_oracle.softmax(zt)
            gzs = coef[:, None] * (ps - qt)
            dgz = coef[:, None] * (ps * _softmax_err(zSs, Tn)[:, None] + qt * _softmax_err(zSt, Tn)[:, None])
            tail_s = ((dgz + (C + 4) * U32 * np.abs(gzs)) @ aW2) * (inp["keep2"].astype(np.float64) / (1.0 - p))
        parts["strong"] = dict(x=xs, act=act_s, vlen=vlen_s, g=np.asarray(r["e_strong_grad"], np.float64))
        parts["weak_x"] = xw
        strong = wgrad64(**parts["strong"])
        tail = tail + wgrad64_scaled(xs, act_s, tail_s / np.maximum(vlen_s, 1.0)[:, None])[1]
        dW1, S1, db1, Sb1 = dW1 + strong[0], S1 + strong[1], db1 + strong[2], Sb1 + strong[3]
        dW2, S2 = dW2 + gzs.T @ ds, S2 + np.abs(gzs).T @ np.abs(ds)
        db2, Sb2 = db2 + gzs.sum(0), Sb2 + np.abs(gzs).sum(0)
    ref = dict(oracle=r, grads=[dW1, db1, dW2, db2], S=[S1, Sb1, S2, Sb2], tail=tail, strong=strong[:2], e=e, z=z,
               zS=zS, T=T, n_rows=Bc * Tc + Bn * Tn, parts=parts)
    w_scl = scl_weight(c, epoch)
    return _add_scl(ref, inp, st, c, w_scl) if w_scl > 0 else ref


_CASES = {}


def case(geom, epoch, **cfg_over):
    """(inputs, state, reference) of one geometry (a GEOMS or LONG_GEOMS entry, or S1_PLUS) at `epoch`: computed
    once, never changed.  `cfg_over`: settings that differ from cfg() (the step under test must get them too)."""
    key = (geom_id(geom), epoch) + tuple(sorted(cfg_over.items()))
    if key not in _CASES:
        g = dict(geom)
        if "id" in g:
            del g["id"]
            st = state(tau_range=TAU_RANGE_OPEN if g.pop("tau", None) == "open" else TAU_RANGE)
            inp = long_problem(**g)
        else:
            ragged = g.pop("ragged", True)
            inp = problem(ragged=ragged, **g)
            st = state(tau_range=tau_range(g["Bn"]))
        c = dict(cfg(), **cfg_over)
        if scl_weight(c, epoch) > 0:
            # No step reads the noisy batch's labels.  On these problems the teacher's pseudo-label of every
            # masked-in row IS the true label, so a term fed the labels would pass; the cases with the term on hand
            # the step labels that differ from the pseudo-label in every such row (test_exact_problem_cpu.py checks
            # it; the reference does not depend on them).
            inp = dict(inp, yn=(inp["yn"] + 1) % synth.N_CLS)
        _CASES[key] = (inp, st, reference(inp, st, c, epoch))
    return _CASES[key]


GRAD_NAMES = ("dW1", "db1", "dW2", "db2")


def bound(name, precision, n_rows):
    """The factor on S_<name> (gradients), on |e_ref| (name 'e', n_rows = the padded length T) or on the logits'
    magnitude sum (name 'z', n_rows = T), as derived in the module docstring."""
    if name == "e":
        return (n_rows + 2) * U32
    if name == "z":
        return (n_rows + synth.H_DIM + 8) * U32
    assert name in GRAD_NAMES and precision in EPS_OP
    return (EPS_OP[precision] if name == "dW1" else 0.0) + n_rows * U32 + TAIL_TOL


def worst(err, lim):
    """max err / lim; an element with lim == 0 must have err == 0 (else inf)."""
    err, lim = np.abs(np.asarray(err, np.float64)).ravel(), np.asarray(lim, np.float64).ravel()
    if err.size == 0:
        return 0.0
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(lim > 0, err / lim, np.where(err > 0, np.inf, 0.0))
    return float(r.max())


def grad_ratios(grads, ref, precision):
    """{name: worst |g - g_ref| / bound} over the four gradient tensors."""
    return {n: worst(np.asarray(g, np.float64).reshape(gr.shape) - gr, grad_limit(n, precision, ref))
            for n, g, gr in zip(GRAD_NAMES, grads, ref["grads"])}


def grad_limit(name, precision, ref):
    """The elementwise bound of gradient tensor `name`: bound() x S, for dW1 the tail term, and with the contrastive
    term on its allowance in dW1 (inside ref["tail"]) and db1."""
    lim = bound(name, precision, ref["n_rows"]) * ref["S"][GRAD_NAMES.index(name)]
    if name == "db1" and "tail_b1" in ref:
        return lim + ref["tail_b1"]
    return lim + ref["tail"] if name == "dW1" else lim


def forward_ratios(out, ref):
    """{name: worst error / bound} over the embeddings and logits the reference holds."""
    res = {}
    for k, er in ref["e"].items():
        res[k] = worst(np.asarray(out[k], np.float64) - er, bound("e", None, ref["T"][k]) * np.abs(er))
    for k, zr in ref["z"].items():
        res[k] = worst(np.asarray(out[k], np.float64) - zr, bound("z", None, ref["T"][k]) * ref["zS"][k])
    return res
