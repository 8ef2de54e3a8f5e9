"""float64 reference of dad_attribution (include/dad.h, "attributions of a split"): the closed form of integrated
gradients along the straight path x' -> x_t, its bounds, its restatements in the kernel's own number formats, and
the wrong answers the tests must tell from it.

Definition, per utterance u of len frames x_t, baseline row x' and logit cotangent dz_u held fixed along the path:
    p0_j = W1[j] . x' + b1[j],   a_tj = W1[j] . (x_t - x'),   p1_tj = p0_j + a_tj
    l_tj = |{alpha in [0, 1] : p0_j + alpha a_tj > 0}|   (1; 0; p1 / (p1 - p0); p0 / (p0 - p1))
    g_u  = W2^T dz_u / max(len, 1)
    attr_t[d] = (x_t[d] - x'[d]) sum_j l_tj g_u[j] W1[j][d],   frame_attr_t = sum_j g_u[j] (ReLU p1_tj - ReLU p0_j)
    chan_attr_u = sum_t attr_t,   utt_total_u = sum_t frame_attr_t
Per-frame quantities live in the kernel's explicit layout [32 * slabs, ...]: frame t of utterance i in row
32 * slab_off[i] + t, zeros elsewhere.

Bounds.  u = 2^-24, H = 256, D = 768, S_t[d] = |x_t[d] - x'[d]| sum_j l_tj |g_u[j]| |W1[j][d]|.  k roundings compound
to gamma(k) = k u / (1 - k u).
  * Exact grid (operands exact in the format, exact_problem below): every product and partial sum of both forward
    GEMVs is exact in fp32, so p0, p1 and the case decisions are the reference's.  What rounds: g_u (one product,
    three fmas, the division: 5; its cancellation is charged to |g_u| as input_grad_ref.py does), l (the difference
    and the quotient: 2), l g (1), H products in the GEMM (1 each) and their H - 1 additions, the factor's
    difference (1) and the final product (1): H + C_OPS roundings with C_OPS = 10, so |attr - ref| <=
    gamma(H + 10) S.  fp16 operands: the coefficient l (c_u s_u[j]) is rounded to fp16, 2^-11 relative, or 2^-25
    absolute in the scaled unit where it is an fp16 subnormal: + 2^-11 S + SUB with SUB_t[d] = |x_t[d] - x'[d]|
    sum_j [l_tj > 0] 2^-25 / (c_u len) |W1[j][d]|; everything else it does (products of halves, fp32 accumulation,
    1 / c_u exact, the division by len) is inside the same count.
  * Random operands.  The forward errs by at most lim_tj = (D + 2) u (|x_t - x'| . |W1[j]| + |p0_j| + |W1[j]| . |x'|)
    on p1.  l moves by at most dl = min(1, 2 lim / |p0|) on a unit with |p1| <= lim (its case may change), by
    min(1, lim |p0| / (|p1 - p0| - lim)^2) on any other crossing unit (|d l / d p1| = |p0| / (p1 - p0)^2, taken at
    the nearest admissible p1; 1 when the denominator is not positive), and not at all otherwise.  SENS_t[d] =
    |x_t[d] - x'[d]| sum_j dl_tj |g_u[j] W1[j][d]| is added; no element is left out.
  * frame_attr: gamma(H + 10) sum_j |g_j| (|ReLU p1| + |ReLU p0|) + sum_j |g_j| lim_tj (ReLU is 1-Lipschitz, so a
    changed decision costs no more than the forward error).  On the exact grid lim = 0.
  * chan_attr, utt_total: the sums of the element bounds over an utterance's frames, plus gamma(len) of the sum of the
    magnitudes (the fp32 additions, whatever their order).
  * Completeness against fp32 logits z: the utt_total bound + sum_c |dz_c| zlim_c with zlim = gamma(len + H + 8)
    (|e| |W2|^T + |b2|) (exact_problem.py's logit bound) + |W2| mean_t lim0_t, lim0 the forward error at x' = 0.
  * The golden's midpoint rule of m = 256 points counts the midpoints inside a unit's active interval: it errs in l
    by at most 1 / (2 m) on a crossing unit and by nothing elsewhere: MID_t[d] = |x_t[d] - x'[d]| sum_{j crossing}
    |g_j W1[j][d]| / (2 m).
"""
import numpy as np

from input_grad_ref import (D, H, C, U, f16, q, slab_prefix, to_explicit, valid_rows, worst, forward64,  # noqa: F401
                            EXACT_POW2, EXACT_ODD)

C_OPS = 10
VARIANTS = ("gradient_x_input", "lambda_at_baseline", "cross_as_half", "lambda_complement",
            "factor_x_not_x_minus_baseline", "no_len_division", "rows_past_len", "w1_tile_transposed")
GOLDEN_POINTS = 256


def gamma(k):
    return k * U / (1.0 - k * U)


def lam_of(p0, p1):
    """The four-case closed form, elementwise (the kernel's expressions)."""
    pos0, pos1 = p0 > 0, p1 > 0
    with np.errstate(divide="ignore", invalid="ignore"):
        qd = np.where(pos1, p1, p0) / np.where(pos1, p1 - p0, p0 - p1)
    return np.where(pos0 != pos1, qd, np.where(pos0, 1.0, 0.0)).astype(p1.dtype)


def reference(feats, sizes, offsets, params, dz, baseline=None, variant=None, dtype=np.float64, fp16_operands=False):
    """The closed form.  feats [frames, 768] (the store's values, widened), baseline None or [768].  dtype float32
    restates it in the kernel's accumulation format (NumPy's summation order); fp16_operands rounds the rows, W1, the
    baseline behind p0 and the scaled coefficient to fp16 as DAD_PREC_FP16 does (accumulation in float64).  Returns
    explicit-layout float64 'attr', 'S', 'sens', 'sub', 'mid' [32 * slabs, 768]; 'frame_attr', 'frame_mag',
    'frame_lim' [32 * slabs]; 'chan_attr' [n, 768], 'utt_total' [n]; 'counts' (frames, non-finite, crossing pairs,
    l = 1 pairs); 'switch_share' (hidden units whose sign differs between baseline and input); 'z0' [n, 4] = W2
    ReLU(p0) + b2 and 'z1' [n, 4] the logits at x, both float64; 'n_near' the (t, j) pairs with |p1| <= lim, the only
    ones whose case an fp32 forward may decide otherwise."""
    W1, b1, W2, b2 = [np.asarray(p, np.float64) for p in params]
    xb = np.zeros(D) if baseline is None else np.asarray(baseline, np.float64)
    if variant == "w1_tile_transposed":
        Wb = W1.copy()
        Wb[:32, :32] = W1[:32, :32].T
    else:
        Wb = W1
    Wf, xbf = (f16(W1), f16(xb)) if fp16_operands else (W1, xb)
    soff = slab_prefix(sizes)
    n, R = len(sizes), 32 * int(soff[-1])
    out = {k: np.zeros((R, D)) for k in ("attr", "S", "sens", "sub", "mid")}
    for k in ("frame_attr", "frame_mag", "frame_lim"):
        out[k] = np.zeros(R)
    out["chan_attr"], out["utt_total"] = np.zeros((n, D)), np.zeros(n)
    aW1 = np.abs(W1)
    wb = (Wf.astype(dtype) @ xbf.astype(dtype)).astype(dtype)
    p0 = (wb + b1.astype(dtype)).astype(dtype)
    p0_64 = p0.astype(np.float64)
    out["z0"] = np.tile(W2 @ np.maximum(W1 @ xb + b1, 0) + b2, (n, 1))
    out["z1"] = forward64(feats, sizes, offsets, params)
    frames = cross = ones = n_near = 0
    for i, (o, L) in enumerate(zip(offsets, sizes)):
        if L == 0:
            continue
        r0 = 32 * int(soff[i])
        rows = L if variant != "rows_past_len" else 32 * int(soff[i + 1] - soff[i])
        x = np.zeros((rows, D))
        x[:L] = feats[o:o + L]
        if rows > L:
            x[L:] = x[L - 1]
        xf = f16(x) if fp16_operands else x
        acc = (xf.astype(dtype) @ Wf.astype(dtype).T).astype(dtype)
        p1 = (p0[None, :] + (acc - wb[None, :]).astype(dtype)).astype(dtype)
        lam = lam_of(np.broadcast_to(p0, p1.shape), p1).astype(np.float64)
        p1_64 = p1.astype(np.float64)
        pos0, pos1 = np.broadcast_to(p0_64 > 0, p1.shape), p1_64 > 0
        crossing = pos0 != pos1
        if variant == "gradient_x_input":
            lam = pos1.astype(np.float64)
        elif variant == "lambda_at_baseline":
            lam = pos0.astype(np.float64)
        elif variant == "cross_as_half":
            lam = np.where(crossing, 0.5, lam)
        elif variant == "lambda_complement":
            lam = np.where(crossing, 1.0 - lam, lam)
        s = (W2.astype(dtype).T @ np.asarray(dz[i], dtype)).astype(dtype)
        den = dtype(1.0) if variant == "no_len_division" else dtype(max(L, 1))
        g = (s / den).astype(np.float64)
        if fp16_operands:
            mx = np.abs(s).max()
            c = 2.0 ** (14 - int(np.floor(np.log2(mx)))) if mx > 0 else 1.0
            A = f16(lam * (s.astype(np.float64) * c)[None, :])
            G = (A @ f16(Wb)) / c / float(den)
            out["sub"][r0:r0 + rows] = ((lam > 0) @ aW1) * (2.0 ** -25 / c / float(den))
        else:
            G = ((lam * g[None, :]).astype(dtype) @ Wb.astype(dtype)).astype(np.float64)
        fac = x if variant == "factor_x_not_x_minus_baseline" else x - xb[None, :]
        attr = fac * G
        afac = np.abs(x - xb[None, :])
        ag = np.abs(g)
        out["S"][r0:r0 + rows] = afac * ((lam * ag[None, :]) @ aW1)
        lim = (D + 2) * U * (afac @ aW1.T + np.abs(p0_64)[None, :] + (aW1 @ np.abs(xb))[None, :])
        with np.errstate(divide="ignore", invalid="ignore"):
            near = np.abs(p1_64) <= lim
            dnear = np.minimum(1.0, 2.0 * lim / np.abs(p0_64)[None, :])
            dnear = np.where(np.isnan(dnear), 1.0, dnear)
            room = np.abs(p1_64 - p0_64[None, :]) - lim
            dcross = np.where(room > 0, np.minimum(1.0, lim * np.abs(p0_64)[None, :] / room ** 2), 1.0)
        dl = np.where(near, dnear, np.where(crossing, dcross, 0.0))
        out["sens"][r0:r0 + rows] = afac * ((dl * ag[None, :]) @ aW1)
        out["sub"][r0:r0 + rows] *= afac
        out["mid"][r0:r0 + rows] = afac * ((crossing * ag[None, :]) @ aW1) / (2.0 * GOLDEN_POINTS)
        r1, rr0 = np.maximum(p1_64, 0), np.maximum(p0_64, 0)
        fa = ((r1 - rr0[None, :]).astype(dtype) @ g.astype(dtype)).astype(np.float64)
        out["frame_mag"][r0:r0 + rows] = (r1 + rr0[None, :]) @ ag
        out["frame_lim"][r0:r0 + rows] = lim @ ag
        out["attr"][r0:r0 + rows], out["frame_attr"][r0:r0 + rows] = attr, fa
        out["chan_attr"][i], out["utt_total"][i] = attr.sum(0), fa.sum()
        frames += L
        cross += int(crossing[:L].sum())
        ones += int((pos0 & pos1)[:L].sum())
        n_near += int(near[:L].sum())
    v = valid_rows(sizes)
    out["counts"] = np.array([frames, int((~np.isfinite(out["attr"][v])).sum()), cross, ones])
    out["switch_share"] = cross / max(frames * H, 1)
    out["n_near"] = n_near
    return out


def attr_bound(ref, fp16=False, sens=False):
    """Elementwise bound on |attr - attr_ref| (module docstring)."""
    lim = gamma(H + C_OPS) * ref["S"]
    if fp16:
        lim = lim + 2.0 ** -11 * ref["S"] + ref["sub"]
    if sens:
        lim = lim + ref["sens"]
    return lim


def frame_bound(ref, sens=False):
    lim = gamma(H + C_OPS) * ref["frame_mag"]
    if sens:
        lim = lim + ref["frame_lim"]
    return lim


def _per_utt(rows, sizes):
    soff = slab_prefix(sizes)
    return np.stack([rows[32 * int(soff[i]):32 * int(soff[i + 1])].sum(0) for i in range(len(sizes))])


def chan_bound(ref, sizes, fp16=False, sens=False):
    """[n, 768]: the element bounds summed over an utterance's frames + the fp32 additions."""
    L = np.maximum(np.asarray(sizes, np.float64), 1)[:, None]
    return _per_utt(attr_bound(ref, fp16, sens), sizes) + gamma(L) * _per_utt(np.abs(ref["attr"]), sizes)


def total_bound(ref, sizes, sens=False):
    L = np.maximum(np.asarray(sizes, np.float64), 1)
    return _per_utt(frame_bound(ref, sens), sizes) + gamma(L) * _per_utt(np.abs(ref["frame_attr"]), sizes)


def logit_bound(feats, sizes, offsets, params):
    """[n, 4] bound on an fp32 logit of the eval-mode forward at x (module docstring)."""
    W1, b1, W2, b2 = [np.asarray(p, np.float64) for p in params]
    out = np.zeros((len(sizes), C))
    for i, (o, L) in enumerate(zip(offsets, sizes)):
        if L == 0:
            continue
        x = np.asarray(feats[o:o + L], np.float64)
        e = np.maximum(x @ W1.T + b1, 0).mean(0)
        lim0 = ((D + 2) * U * (np.abs(x) @ np.abs(W1).T + np.abs(b1))).mean(0)
        out[i] = gamma(L + H + 8) * (np.abs(W2) @ e + np.abs(b2)) + np.abs(W2) @ lim0
    return out


def completeness_bound(ref, feats, sizes, offsets, params, dz, sens=True):
    return total_bound(ref, sizes, sens) + (np.abs(np.asarray(dz, np.float64))
                                            * logit_bound(feats, sizes, offsets, params)).sum(1)


def check(got, ref, sizes, fp16=False, sens=False, counts=True):
    """What the GPU tests assert of one call: {name: worst error / bound} for the outputs present in `got`, and a
    list of failures (empty: passes): a ratio above 1, a non-zero row past a length, differing counts."""
    v = valid_rows(sizes)
    ratios, fails = {}, []
    lims = {"attr": lambda: attr_bound(ref, fp16, sens), "frame_attr": lambda: frame_bound(ref, sens),
            "chan_attr": lambda: chan_bound(ref, sizes, fp16, sens), "utt_total": lambda: total_bound(ref, sizes, sens)}
    for name, lim in lims.items():
        if name not in got:
            continue
        g = np.asarray(got[name], np.float64)
        if name in ("attr", "frame_attr"):
            if g[~v].any():
                fails.append("%s: rows past a length are not 0" % name)
            ratios[name] = worst(g[v] - ref[name][v], lim()[v])
        else:
            ratios[name] = worst(g - ref[name], lim())
        if not ratios[name] <= 1.0:
            fails.append("%s: worst error / bound %.3g" % (name, ratios[name]))
    if counts and "counts" in got and not np.array_equal(np.asarray(got["counts"]), ref["counts"]):
        fails.append("counts %r, reference %r" % (list(got["counts"]), list(ref["counts"])))
    return ratios, fails


# ---- the exact grid ----------------------------------------------------------------------------------------------
def exact_problem(sizes, seed=13):
    """Operands on which both forward GEMVs, p0 and p1 are exact in fp32 and in fp16 operands: features multiples of
    2^-3 with |x| <= 16, the baseline multiples of 2^-3 with |x'| <= 1, W1 multiples of 2^-10 with |w| < 0.05 (every
    product a multiple of 2^-13, every partial sum below 2^10: 23 bits), b1 odd multiples of 2^-14 (no pre-activation
    is 0, and p0, p1 stay within 24 bits), W2 multiples of 2^-4 with |w| <= 0.5, dz multiples of 2^-2 (s_u exact).
    Returns (feats, sizes, offsets, params, dz, baseline)."""
    rs = np.random.RandomState(seed)
    sizes = np.asarray(sizes, np.int64)
    offsets = np.concatenate([[0], np.cumsum(sizes)[:-1]])
    feats = q(np.clip(4.0 * rs.standard_normal((int(sizes.sum()), D)), -16, 16), 2.0 ** -3)
    W1 = q(np.clip(0.02 * rs.standard_normal((H, D)), -0.049, 0.049), 2.0 ** -10)
    b1 = (q(0.02 * rs.standard_normal(H), 2.0 ** -13) + np.float32(2.0 ** -14)).astype(np.float32)
    W2 = q(np.clip(0.25 * rs.standard_normal((C, H)), -0.5, 0.5), 2.0 ** -4)
    b2 = q(0.1 * rs.standard_normal(C), 2.0 ** -4)
    dz = q(rs.uniform(-1, 1, (len(sizes), C)), 2.0 ** -2)
    baseline = q(rs.uniform(-1, 1, D), 2.0 ** -3)
    return feats, sizes, offsets, (W1, b1, W2, b2), dz, baseline


def onehot_dz(target):
    return np.eye(C, dtype=np.float32)[np.asarray(target)]


def margin_dz(z, target):
    """e_c - e_c' with c' the runner-up: the largest logit other than the target's (first on a tie)"""
    z = np.asarray(z, np.float64).copy()
    t = np.asarray(target)
    z[np.arange(len(t)), t] = -np.inf
    return (np.eye(C)[t] - np.eye(C)[z.argmax(1)]).astype(np.float32)
