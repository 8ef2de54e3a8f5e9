"""Reference for dad_eval_noise (TEST INFRASTRUCTURE): the definition in include/dad.h ("noise response of a split")
restated in float64 NumPy, the per-utterance comparisons against level 0, and the DAD_EN_* block.

Definition.  Level k of utterance i (L frames x_t, noise rows n_t) is the eval-mode forward on x_t + sigma_k n_t:
  e_k = (1 / max(L, 1)) sum_t relu(W1 (x_t + sigma_k n_t) + b1),  z_k = W2 e_k + b2,  p_k = softmax(z_k),
  pred_k = first maximum of z_k;  drift_k = |e_k - e_0|_2;  kl_k = sum_c p_0c (log p_0c - log p_kc) (0 log 0 = 0);
  break_level = the smallest k >= 1 with pred_k != pred_0, or K.
Explicit noise is slab-aligned: frame t of utterance i of the call is row 32 * slab_off[i] + t of noise
[32 * slabs][768].

Bounds the GPU module holds the device to (u = 2^-24); none is a measured number:
  emb, logits     rtol 1e-5, atol 1e-4: the project's tolerance for this forward in fp32 (test_gpu_windows._check_values,
                  test_gpu_eval_split); the same for 16-bit stores on the widened values and for fp16 operands against
                  float64 on the fp16-rounded rows, noise and W1 (only the accumulation differs).
  probs, score    rtol 1e-5, atol 1e-6 (the same source).
  pred            the first maximum of the device's own logits, and equal to the reference wherever the reference's
                  top-two gap exceeds GAP = windows_ref.GAP (2e-4 = twice the logit atol); at most 5 % of a case's
                  (utterance, level) cells may fall under it (asserted on the reference alone).
  drift           | |a| - |b| | <= |a - b| and each embedding component is within EMB_TOL = atol + rtol max|e|, so
                  |drift - ref| <= |de_k - de_0|_2 <= 2 sqrt(256) EMB_TOL  (DRIFT_LIM).
  kl              kl_lim() below, from the logit bound in the manner of operators_ref.head_reference's eps_z: with
                  eps the largest logit tolerance of the two rows (atol + rtol max|z|), a log-softmax entry moves by
                  at most 2 eps (its logit and the log-sum-exp, each by at most eps) and p_0c by the relative
                  2 eps + (C + 6) u (exact_problem's softmax term), so
                    |kl - ref| <= (2 eps + (C + 6) u) sum_c p_0c |lp_0c - lp_kc| + 4 eps + 32 u (1 + R + ln C),
                  R = the larger logit range of the two rows; the last term covers the fp32 evaluation of
                  (z - m) - log(sum exp) and the products (a few roundings of numbers of size R + ln C).
  break_level, block   equal to this module's restatement from the device's own pred / score / drift / kl; the float64
                  sums within n 2^-53 relative of NumPy's sum of the device's float32 values (a float64 sum of n
                  non-negative terms in any order; kl and drift are >= 0 up to rounding, so the bound is taken on
                  sum |v|).
  exact operands  on tests/exact_problem.py's dyadic grid (features multiples of 2^-3, integer noise in [-3, 3],
                  sigma in {0, 1/8, 1/4, 1/2, 1}, W1 multiples of 2^-10, b1 odd multiples of 2^-14) every
                  pre-activation is an exact odd multiple of 2^-14 at every level in fp32 and fp16, so
                  |e - e_ref| <= (T + 2) u |e_ref| and the logits (T + H + 8) u times their magnitude sum (X.bound).
"""
import functools

import numpy as np

GAP = 2e-4
EMB_RTOL, EMB_ATOL = 1e-5, 1e-4
U32 = 2.0 ** -24
C = 4
LEVELS4 = (0.0, 0.01, 0.05, 0.25)
LEVELS8 = (0.0, 0.01, 0.05, 0.25, 0.25, 1.0, 0.0, 4.0)      # a duplicate, a zero that is not first, a large level
NOISE_SEED = 31
VARIANTS = ("level_shift", "noise_by_store_row", "sigma_after_relu", "padded_mean", "kl_swapped")


def slab_prefix(lens):
    lens = np.asarray(lens, np.int64)
    return np.concatenate([[0], np.cumsum((lens + 31) // 32)])


def log_softmax64(z):
    zs = z - z.max(-1, keepdims=True)
    return zs - np.log(np.exp(zs).sum(-1, keepdims=True))


def forward64(x, noise, sizes, offsets, order, sigmas, params, fp16_operands=False, variant=None):
    """float64 outputs of every level for the subset `order` of a store with rows x [frames, 768] (already widened
    to float32 values) under explicit noise [32 * slabs, 768] in the subset's slab-aligned layout.  params =
    (W1, b1, W2, b2).  With fp16_operands the rows, the noise and W1 are rounded to fp16 first.  variant builds one
    of the WRONG references of the controls (VARIANTS).  Returns [K, n, ...] arrays: emb, logits, logit_mag, probs,
    score_entropy, score_max, pred, gap, drift, kl, kl_lim, and break_level [n]."""
    W1, b1, W2, b2 = (np.asarray(a, np.float32) for a in params)
    x, noise = np.asarray(x, np.float32), np.asarray(noise, np.float32)
    if fp16_operands:
        x, noise, W1 = x.astype(np.float16), noise.astype(np.float16), W1.astype(np.float16)
    W1, b1, W2, b2 = (a.astype(np.float64) for a in (W1, b1, W2, b2))
    hx = x.astype(np.float64) @ W1.T
    hn = noise.astype(np.float64) @ W1.T
    return _levels(hx, hn, sizes, offsets, order, sigmas, b1, W2, b2, variant)


def _levels(hx, hn, sizes, offsets, order, sigmas, b1, W2, b2, variant=None):
    sub = np.asarray(sizes)[order]
    soff = slab_prefix(sub)
    sig = list(sigmas)
    if variant == "level_shift":
        sig = sig[1:] + sig[:1]
    K, n = len(sig), len(order)
    emb = np.zeros((K, n, hx.shape[1]))
    for j, i in enumerate(order):
        L = int(sizes[i])
        if L == 0:
            continue
        a = hx[offsets[i]:offsets[i] + L]
        if variant == "noise_by_store_row":
            b = hn[(offsets[i] + np.arange(L)) % len(hn)]
        else:
            b = hn[32 * soff[j]:32 * soff[j] + L]
        den = 32 * -(-L // 32) if variant == "padded_mean" else L
        for k, s in enumerate(sig):
            if variant == "sigma_after_relu":
                rows = np.maximum(a + b1, 0.0) + s * b
            else:
                rows = np.maximum(a + s * b + b1, 0.0)
            emb[k, j] = rows.sum(0) / den
    return heads(emb, W2, b2, variant)


def heads(emb, W2, b2, variant=None):
    z = emb @ W2.T + b2
    lp = log_softmax64(z)
    p = np.exp(lp)
    top = np.sort(z, -1)
    ent = -(p * np.log2(p + 1e-8)).sum(-1)
    pmax = p.max(-1)
    pred = z.argmax(-1)
    with np.errstate(invalid="ignore"):
        if variant == "kl_swapped":
            kl = np.where(p > 0, p * (lp - lp[0:1]), 0.0).sum(-1)
        else:
            kl = np.where(p[0:1] > 0, p[0:1] * (lp[0:1] - lp), 0.0).sum(-1)
    out = {"emb": emb, "logits": z, "logit_mag": np.abs(emb) @ np.abs(W2).T + np.abs(b2), "probs": p,
           "score_entropy": pmax * (1 - ent / 2.0), "score_max": pmax, "pred": pred, "gap": top[..., -1] - top[..., -2],
           "drift": np.sqrt(((emb - emb[0:1]) ** 2).sum(-1)), "kl": kl, "break_level": break_level(pred)}
    out["kl_lim"] = kl_lim(z, p, lp)
    return out


def emb_tol(ref_emb):
    return EMB_ATOL + EMB_RTOL * float(np.abs(ref_emb).max())


def drift_lim(ref_emb):
    return 2.0 * np.sqrt(ref_emb.shape[-1]) * emb_tol(ref_emb)


def kl_lim(z, p, lp):
    """The bound on |kl - ref| [K, n] derived in the module docstring."""
    eps_row = EMB_ATOL + EMB_RTOL * np.abs(z).max(-1)                     # [K, n]
    eps = np.maximum(eps_row, eps_row[0:1])
    rng = z.max(-1) - z.min(-1)
    R = np.maximum(rng, rng[0:1])
    A = (p[0:1] * np.abs(lp[0:1] - lp)).sum(-1)
    return (2.0 * eps + (C + 6) * U32) * A + 4.0 * eps + 32.0 * U32 * (1.0 + R + np.log(C))


def break_level(pred):
    """[n] from pred [K, n]: the smallest k >= 1 with pred_k != pred_0, or K."""
    pred = np.asarray(pred)
    K = pred.shape[0]
    moved = pred != pred[0:1]
    moved[0] = False
    return np.where(moved.any(0), moved.argmax(0), K).astype(np.int64)


def decided(ref, min_gap=GAP):
    """(utterance, level) cells whose reference prediction a logit error below min_gap / 2 cannot change; the filter
    may drop at most 5 % of a case's cells (asserted on the reference alone)."""
    ok = ref["gap"] > min_gap
    assert (~ok).mean() <= 0.05, "the reference itself has %d of %d near-ties" % ((~ok).sum(), ok.size)
    return ok


def block(L, pred, score, drift, kl, labels, n_nonfinite=0):
    """(counts int64 [EN_COUNTS], sums float64 [EN_SUMS]) from the per-utterance [K, n] values (float32 for the three
    summed ones) and the labels (None: no utterance is labelled).  L = the package's _lib (slot numbers)."""
    pred = np.asarray(pred, np.int64)
    K, n = pred.shape
    labels = np.full(n, -1, np.int64) if labels is None else np.asarray(labels, np.int64)
    lab = (labels >= 0) & (labels < 4)
    brk = break_level(pred)
    counts = np.zeros(L.EN_COUNTS, np.int64)
    sums = np.zeros(L.EN_SUMS, np.float64)
    for k in range(K):
        cm = np.zeros((4, 4), np.int64)
        np.add.at(cm, (labels[lab], pred[k][lab]), 1)
        counts[L.EN_CONF + 16 * k:L.EN_CONF + 16 * (k + 1)] = cm.ravel()
        counts[L.EN_FLIPS + k] = (pred[k] != pred[0]).sum()
        counts[L.EN_SURVIVE + k] = (brk > k).sum()
        for slot, v in ((L.EN_SUM_SCORE, score), (L.EN_SUM_DRIFT, drift), (L.EN_SUM_KL, kl)):
            sums[slot + k] = np.asarray(v[k], np.float64).sum()
    counts[L.EN_N], counts[L.EN_N_LABELLED], counts[L.EN_N_SKIPPED] = n, lab.sum(), (~lab).sum()
    counts[L.EN_N_NONFINITE], counts[L.EN_LEVELS] = n_nonfinite, K
    return counts, sums


# ---- the shared inputs of the CPU and GPU modules ------------------------------------------------------------
@functools.lru_cache(None)
def main_inputs():
    """test_gpu_eval_split._inputs('main') (37 utterances read through a shuffled subset of 39 with two repeats) and
    the explicit noise of the subset: standard_normal(RandomState(NOISE_SEED)) float32 [32 * slabs, 768]."""
    from test_gpu_eval_split import _inputs
    feats, sizes, offsets, labels, order = _inputs("main")
    slabs = int(slab_prefix(sizes[order])[-1])
    noise = np.random.RandomState(NOISE_SEED).standard_normal((32 * slabs, 768)).astype(np.float32)
    return feats, sizes, offsets, labels, order, noise


def widen(feats, dt):
    from windows_ref import widen as w
    return w(feats, dt)


@functools.lru_cache(None)
def _main_products(dt, net, fp16_operands):
    from oracle import data_oracle as do
    feats, _, _, _, _, noise = main_inputs()
    W1 = np.asarray(do.eval_weights(11)["st".index(net)][0], np.float32)
    x = widen(feats, dt)
    if fp16_operands:
        x, noise, W1 = x.astype(np.float16), noise.astype(np.float16), W1.astype(np.float16)
    W1 = W1.astype(np.float64)
    return x.astype(np.float64) @ W1.T, noise.astype(np.float64) @ W1.T


@functools.lru_cache(None)
def main_reference(dt, net, sigmas, fp16_operands=False, variant=None):
    """forward64 of the main inputs for one store type, network ('s' / 't') and tuple of levels; computed once per
    case, never modified."""
    from oracle import data_oracle as do
    _, sizes, offsets, _, order, _ = main_inputs()
    _, b1, W2, b2 = (np.asarray(a, np.float64) for a in do.eval_weights(11)["st".index(net)])
    hx, hn = _main_products(dt, net, fp16_operands)
    return _levels(hx, hn, sizes, offsets, order, sigmas, b1, W2, b2, variant)
