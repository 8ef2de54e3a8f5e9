"""Synthetic DAD steps whose encoder operands are exactly representable in fp16 AND bf16, with a float64
reference and an error bound derived from the reference alone (TEST INFRASTRUCTURE; imports oracle/ only).

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
The forward bounds hold for ALL three precisions: the 16-bit conversion is lossless on these inputs, so a 16-bit
forward that differs from the fp32 one beyond summation order is a bug.
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
# tests/test_gpu_parity.EDGE (the GPU module asserts they are the same)
GEOMS = [
    dict(B=1, T=1, Bn=2, Tn=3),
    dict(B=5, T=33, Bn=7, Tn=31),
    dict(B=16, T=64, Bn=16, Tn=64),
    dict(B=12, T=45, Bn=20, Tn=70, ragged=False),
    dict(B=64, T=40, Bn=64, Tn=40),
]


def geom_id(g):
    return "B%dT%d_Bn%dTn%d" % (g["B"], g["T"], g["Bn"], g["Tn"])


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


def reference(inp, st, c, epoch):
    """One DADOracle.step from state `st`, then the float64 rebuild.  Returns a dict:
      oracle   the oracle's own output (losses, mask, fp32 grads, ...)
      grads    [dW1, db1, dW2, db2] float64;  S: their abs-sums;  tail: dW1's tail term [H, D]
      strong   the strong branch's share (dW1, S_W1) (zeros in the warm-up)
      e, z     float64 embeddings / logits by name (e_clean, ...);  zS: the logit bound's magnitude sum
      T        the padded length behind each e_* / z_* name;  n_rows = Bc Tc + Bn Tn
      parts    what the gradient was built from (x, act, vlen, g per branch), for the CPU module's mutants"""
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
    return dict(oracle=r, grads=[dW1, db1, dW2, db2], S=[S1, Sb1, S2, Sb2], tail=tail, strong=strong[:2], e=e, z=z,
                zS=zS, T=T, n_rows=Bc * Tc + Bn * Tn, parts=parts)


_CASES = {}


def case(geom, epoch):
    """(inputs, state, reference) of one geometry (a GEOMS entry) at `epoch`: computed once, never changed."""
    key = (geom_id(geom), epoch)
    if key not in _CASES:
        g = dict(geom)
        ragged = g.pop("ragged", True)
        inp = problem(ragged=ragged, **g)
        st = state(tau_range=tau_range(g["Bn"]))
        _CASES[key] = (inp, st, reference(inp, st, cfg(), epoch))
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
    """The elementwise bound of gradient tensor `name`: bound() x S, and for dW1 the tail term."""
    lim = bound(name, precision, ref["n_rows"]) * ref["S"][GRAD_NAMES.index(name)]
    return lim + ref["tail"] if name == "dW1" else lim


def forward_ratios(out, ref):
    """{name: worst error / bound} over the embeddings and logits the reference holds."""
    res = {}
    for k, er in ref["e"].items():
        res[k] = worst(np.asarray(out[k], np.float64) - er, bound("e", None, ref["T"][k]) * np.abs(er))
    for k, zr in ref["z"].items():
        res[k] = worst(np.asarray(out[k], np.float64) - zr, bound("z", None, ref["T"][k]) * ref["zS"][k])
    return res
