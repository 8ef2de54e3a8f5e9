"""float64 reference of dad_input_grad (include/dad.h, "input gradients of a split"), its bounds, its restatements in
the kernel's own number formats, and the wrong answers the tests must tell from it.

Definition, per utterance u of len frames x_t with perturbation delta_t and logit cotangent dz_u:
    pre_tj = W1[j] . (x_t + delta_t) + b1[j],  m_tj = pre_tj > 0,  s_u = W2^T dz_u,  g_u = s_u / max(len, 1)
    G_t[d] = sum_j m_tj g_u[j] W1[j][d],  step = clamp(delta + alpha sgn(G), -r, r), sgn(0) = 0
Everything per frame lives in the kernel's explicit layout [32 * slabs, 768]: frame t of utterance i in row
32 * slab_off[i] + t, zeros elsewhere.

Bounds (u = 2^-24, H = 256, D = 768, S_t[d] = sum_j m_tj |g_u[j]| |W1[j][d]|):
  * An fp32 sum of H products in any order errs by at most (H - 1) u of its magnitude sum, each product by u, and g_u
    carries 4 roundings of s (one product, three fmas) and one of the division: (H + 4) u S bounds |G - G_ref| when
    the ReLU' pattern is the reference's.  (The cancellation inside s_u is charged to |g_u|, as exact_problem.py
    charges a logit's to its magnitude sum; the tests print error / bound.)
  * fp16 operands add one rounding of 2^-11 relative on each A element when W1 and x + delta are exact in fp16 (the
    exact grid): 2^-11 S.
  * An fp32 forward errs by at most (D + 2) u (|x_t| . |W1[j]| + |b1[j]|) on pre_tj, so only the units J_t whose
    reference |pre| lies within that may legitimately take the other ReLU' decision; each moves G_t[d] by
    |g_u[j] W1[j][d]|.  flip_term sums those.
  * frame_l1 sums D non-negative fp32 terms: D u relative.
"""
import numpy as np

U = 2.0 ** -24
H, D, C = 256, 768, 4
GOLDEN_EPS = (0.01, 0.05, 0.25)

VARIANTS = ("relu_ignored", "no_len_division", "rows_past_len", "mask_at_x", "sgn0_plus", "no_clamp",
            "w1_tile_transposed")


def q(a, step):
    return (np.round(np.asarray(a, np.float64) / step) * step).astype(np.float32)


def slab_prefix(sizes):
    return np.concatenate([[0], np.cumsum((np.asarray(sizes, np.int64) + 31) // 32)])


def to_explicit(rows, sizes, offsets):
    """per-frame rows [frames, ...] -> the explicit layout [32 * slabs, ...] (zeros in the unused rows)"""
    soff = slab_prefix(sizes)
    out = np.zeros((32 * int(soff[-1]),) + rows.shape[1:], rows.dtype)
    for i, (o, L) in enumerate(zip(offsets, sizes)):
        out[32 * soff[i]:32 * soff[i] + L] = rows[o:o + L]
    return out


def valid_rows(sizes):
    soff = slab_prefix(sizes)
    v = np.zeros(32 * int(soff[-1]), bool)
    for i, L in enumerate(sizes):
        v[32 * soff[i]:32 * soff[i] + L] = True
    return v


def f16(a):
    return np.asarray(a, np.float32).astype(np.float16).astype(np.float64)


def reference(feats, sizes, offsets, params, dz, delta=None, alpha=0.0, radius=np.inf, variant=None, dtype=np.float64,
              fp16_operands=False):
    """The closed form.  feats [frames, 768] (the store's values, widened), delta None or explicit-layout
    [32 * slabs, 768].  dtype float32 restates it in the kernel's accumulation format (NumPy's summation order);
    fp16_operands rounds x + delta, W1 and the scaled backward A operand to fp16 as DAD_PREC_FP16 does (accumulation
    in float64).  Returns explicit-layout float64 'grad', 'step', 'S', 'flip_term' and 'frame_l1' [32 * slabs],
    'counts' (frames, non-finite, zeros), 'n_flip_units', 'flip_frames'."""
    W1, b1, W2, b2 = [np.asarray(p, np.float64) for p in params]
    if variant == "w1_tile_transposed":        # W1[j][d] taken as W1[32 (j / 32) + d % 32][32 (d / 32) + j % 32] within a tile
        Wb = W1.copy()
        Wb[:32, :32] = W1[:32, :32].T
    else:
        Wb = W1
    soff = slab_prefix(sizes)
    R = 32 * int(soff[-1])
    out = {k: np.zeros((R, D)) for k in ("grad", "step", "S", "flip_term")}
    out["frame_l1"] = np.zeros(R)
    n_flip, flip_frames, frames = 0, 0, 0
    aW1 = np.abs(W1)
    for i, (o, L) in enumerate(zip(offsets, sizes)):
        if L == 0:
            continue
        r0 = 32 * int(soff[i])
        rows = L if variant != "rows_past_len" else 32 * int(soff[i + 1] - soff[i])
        x = np.zeros((rows, D))
        x[:L] = feats[o:o + L]
        if rows > L:
            x[L:] = x[L - 1]
        dl = np.zeros((rows, D)) if delta is None else np.asarray(delta[r0:r0 + rows], np.float64)
        xf = x if variant == "mask_at_x" else x + dl
        Wf = W1
        if fp16_operands:
            xf, Wf = f16(xf), f16(W1)
        xf = xf.astype(dtype)
        pre = (xf @ Wf.astype(dtype).T + b1.astype(dtype)).astype(np.float64)
        m = np.ones_like(pre, bool) if variant == "relu_ignored" else pre > 0
        s = (W2.astype(dtype).T @ np.asarray(dz[i], dtype)).astype(dtype)
        den = dtype(1.0) if variant == "no_len_division" else dtype(max(L, 1))
        g = (s / den).astype(np.float64)
        if fp16_operands:
            mx = np.abs(s).max()
            c = 2.0 ** (14 - int(np.floor(np.log2(mx)))) if mx > 0 else 1.0
            A = m * f16(s.astype(np.float64) * c)[None, :]
            G = (A @ f16(Wb)) / c / float(den)
        else:
            G = ((m * g[None, :]).astype(dtype) @ Wb.astype(dtype)).astype(np.float64)
        S = (m * np.abs(g)[None, :]) @ aW1
        lim = (D + 2) * U * (np.abs(xf.astype(np.float64)) @ aW1.T + np.abs(b1))
        J = np.abs(pre) <= lim
        n_flip += int(J[:L].sum())
        flip_frames += int(J[:L].any(1).sum())
        ft = (J * np.abs(g)[None, :]) @ aW1
        sg = np.sign(G)
        if variant == "sgn0_plus":
            sg = np.where(G == 0, 1.0, sg)
        st = dl + alpha * sg
        if variant != "no_clamp":
            st = np.clip(st, -radius, radius)
        k = rows
        out["grad"][r0:r0 + k], out["step"][r0:r0 + k] = G, st
        out["S"][r0:r0 + k], out["flip_term"][r0:r0 + k] = S, ft
        out["frame_l1"][r0:r0 + k] = np.abs(G).sum(1)
        frames += L
    v = valid_rows(sizes)
    out["counts"] = np.array([frames, int((~np.isfinite(out["grad"][v])).sum()), int((out["grad"][v] == 0).sum()), 0])
    out["n_flip_units"], out["flip_frames"] = n_flip, flip_frames
    return out


def grad_bound(ref, fp16=False, flips=False):
    """Elementwise bound on |G - G_ref| (module docstring)."""
    lim = (H + 4) * U * ref["S"]
    if fp16:
        lim = lim + 2.0 ** -11 * ref["S"]
    if flips:
        lim = lim + ref["flip_term"]
    return lim


def worst(err, lim):
    """max err / lim; an element with lim == 0 must have err == 0 (else inf)."""
    err, lim = np.abs(np.asarray(err, np.float64)).ravel(), np.asarray(lim, np.float64).ravel()
    if err.size == 0:
        return 0.0
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(lim > 0, err / lim, np.where(err > 0, np.inf, 0.0))
    return float(r.max())


def check_grad(G, ref, sizes, fp16=False, flips=False):
    """What the GPU test asserts of a gradient: the elementwise bound, equal signs wherever |G_ref| exceeds it.
    Returns (worst error / bound, number of sign mismatches among the checked elements, share left unchecked)."""
    v = valid_rows(sizes)
    G, Gr, lim = np.asarray(G, np.float64)[v], ref["grad"][v], grad_bound(ref, fp16, flips)[v]
    ratio = worst(G - Gr, lim)
    checked = np.abs(Gr) > lim
    bad = int((np.sign(G)[checked] != np.sign(Gr)[checked]).sum())
    return ratio, bad, 1.0 - checked.mean()


def exact_failures(got, ref, sizes, fp16=False):
    """What the GPU test asserts on the exact grid, as a list of failures (empty: passes).  got / ref: dicts with
    explicit-layout 'grad', 'step', 'frame_l1'.  Power-of-two lengths: grad and step bit-equal, frame_l1 within
    D u relative.  Other lengths: the derived bound, equal signs and equal steps wherever |G_ref| exceeds it.  Rows
    past each length are 0."""
    fails = []
    v = valid_rows(sizes)
    soff = slab_prefix(sizes)
    G, st, l1 = (np.asarray(got[k], np.float64) for k in ("grad", "step", "frame_l1"))
    if G[~v].any() or st[~v].any() or l1[~v].any():
        fails.append("rows past a length are not 0")
    lim = grad_bound(ref, fp16)
    for i, L in enumerate(sizes):
        if L == 0:
            continue
        r = slice(32 * int(soff[i]), 32 * int(soff[i]) + int(L))
        if L & (L - 1) == 0:
            if not np.array_equal(G[r], ref["grad"][r]):
                fails.append("grad bits, length %d" % L)
            if not np.array_equal(st[r], ref["step"][r]):
                fails.append("step bits, length %d" % L)
        else:
            if worst(G[r] - ref["grad"][r], lim[r]) > 1.0:
                fails.append("grad bound, length %d" % L)
            sure = np.abs(ref["grad"][r]) > lim[r]
            if (np.sign(G[r])[sure] != np.sign(ref["grad"][r])[sure]).any():
                fails.append("signs, length %d" % L)
            if not np.array_equal(st[r][sure], ref["step"][r][sure]):
                fails.append("steps, length %d" % L)
        if worst(l1[r] - ref["frame_l1"][r], D * U * ref["frame_l1"][r]) > 1.0:
            fails.append("frame_l1, length %d" % L)
    return fails


def sign_disagreement(G, ref, sizes):
    v = valid_rows(sizes)
    return float((np.sign(np.asarray(G, np.float64)[v]) != np.sign(ref["grad"][v])).mean())


def forward64(feats, sizes, offsets, params, delta=None):
    """float64 logits [n, 4] of the eval-mode forward at x + delta (delta in the explicit layout); an utterance
    without frames has logits b2."""
    W1, b1, W2, b2 = [np.asarray(p, np.float64) for p in params]
    soff = slab_prefix(sizes)
    z = np.tile(b2, (len(sizes), 1))
    for i, (o, L) in enumerate(zip(offsets, sizes)):
        if L == 0:
            continue
        x = np.asarray(feats[o:o + L], np.float64)
        if delta is not None:
            x = x + np.asarray(delta[32 * soff[i]:32 * soff[i] + L], np.float64)
        z[i] = W2 @ (np.maximum(x @ W1.T + b1, 0).sum(0) / L) + b2
    return z


def softmax64(z):
    e = np.exp(z - z.max(-1, keepdims=True))
    return e / e.sum(-1, keepdims=True)


def ce_dz(z, target):
    return softmax64(np.asarray(z, np.float64)) - np.eye(C)[np.asarray(target)]


def ce_loss(z, target):
    p = softmax64(np.asarray(z, np.float64))
    return -np.log(p[np.arange(len(target)), np.asarray(target)])


# ---- the exact grid ----------------------------------------------------------------------------------------------
EXACT_POW2 = (1, 32, 64)
EXACT_ODD = (31, 33, 65)


def exact_problem(sizes, seed=11):
    """Operands on which G is exact in fp32 for power-of-two lengths (module docstring of the tests): features
    multiples of 2^-3 with |x| < 17, W1 multiples of 2^-10 with |w| < 0.05, b1 odd multiples of 2^-14, W2 multiples
    of 2^-4 with |w| <= 0.5, dz multiples of 2^-2, delta multiples of 2^-3 with |delta| <= 1.
    Returns (feats, sizes, offsets, params, dz, delta explicit)."""
    rs = np.random.RandomState(seed)
    sizes = np.asarray(sizes, np.int64)
    offsets = np.concatenate([[0], np.cumsum(sizes)[:-1]])
    feats = q(np.clip(4.0 * rs.standard_normal((int(sizes.sum()), D)), -16, 16), 2.0 ** -3)
    W1 = q(np.clip(0.02 * rs.standard_normal((H, D)), -0.049, 0.049), 2.0 ** -10)
    b1 = (q(0.02 * rs.standard_normal(H), 2.0 ** -13) + np.float32(2.0 ** -14)).astype(np.float32)
    W2 = q(np.clip(0.25 * rs.standard_normal((C, H)), -0.5, 0.5), 2.0 ** -4)
    b2 = q(0.1 * rs.standard_normal(C), 2.0 ** -4)
    dz = q(rs.uniform(-1, 1, (len(sizes), C)), 2.0 ** -2)
    delta = to_explicit(q(rs.uniform(-1, 1, (int(sizes.sum()), D)), 2.0 ** -3), sizes, offsets)
    return feats, sizes, offsets, (W1, b1, W2, b2), dz, delta
