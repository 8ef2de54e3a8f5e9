"""A reference for the optimizer kernel (csrc/optim.hip: global-norm clip + Adam with L2 decay + teacher
EMA), independent of the step around it; no GPU needed.

reference_update   float64, from first principles.  It takes the hyper-parameters themselves (lr, the
                   Adam count t AFTER this step, ...), never the host-derived dad_config fields
                   (lr_step_size, bc2_sqrt, one_m_beta*): those are part of what is under test.
f32_restatement    the kernel's arithmetic (adam_ema_apply) in np.float32, in its operation order and
                   with the host's c_float constants; MUTATIONS are selectable by name.
frag_index         dad_w1frag_index restated from its formula (csrc/dad_common.h).
bounds             per-element error bounds of a float32 evaluation against reference_update.

Error model.  u = 2^-24 is the unit roundoff of float32 round-to-nearest: every operation and every
host constant rounded to c_float contributes a relative error <= u (sqrtf and the division are
correctly rounded; the library is built with -ffp-contract=off, so nothing is fused).  First order in
u; the K values below are counts of such roundings, written out where they are defined.
"""
import math

import numpy as np

from oracle import synth

U = 2.0 ** -24
TINY = 2.0 ** -149          # float32 subnormal spacing: the absolute floor of every bound
H, D, C = 256, 768, 4
NW1 = H * D
NPARAM = NW1 + H + C * H + C
OFFSETS = (0, NW1, NW1 + H, NW1 + H + C * H, NPARAM)
BETA1, BETA2, EPS = 0.9, 0.999, 1e-8
F = np.float32

# ---- the counts ------------------------------------------------------------------------------
# clip norm: the squared-norm partials are double sums rounded to float (1; the square root halves
#   it) and the double sqrt of their double sum is rounded to float (1).  0.5 + 1 -> K_N = 2.
K_N = 2
# coef = max_norm / (norm + 1e-6f): norm (K_N = 2), the constant 1e-6f (1), the add (1), the constant
#   max_norm (1), the division (1) = 6; coef == 1 exactly when the clip is inactive.
K_COEF = 6
# g = G coef + wd p: on the G coef term coef (6), the multiply (1) and the add (1) = 8; on the wd p term
#   the constant (1), the multiply (1) and the add (1) = 3.  K_G = 8 covers both terms.
K_G = 8
# m' = m + c1 (g - m): g (8), the subtraction (1), the constant c1 = float(1 - beta1) (1), the multiply
#   (1), the add (1) = 12, each on a quantity <= |m| + |g|: absolute K_M u (|m| + |g|).
K_M = 12
# v' = v beta2 + c2 g g: the g g term carries g twice (2 x 8 = 16), the constant c2 (1), two multiplies
#   (2) and the add (1) = 20; the v beta2 term the constant (1), the multiply (1), the add (1) = 3.  Both
#   terms are >= 0, so the larger count bounds v' relatively: K_V = 20.  (g enters squared, which is why
#   this exceeds the 16 a plain count of distinct roundings gives.)
K_V = 20
# update = step (m' / denom), denom = sqrt(v') / bc2_sqrt + eps: sqrt halves v' (10) and rounds (1), the
#   constant bc2_sqrt (1), the division (1), the constant eps (1), the add (1) = 15 on denom; then the
#   division m' / denom (1), the constant step = float(lr / (1 - beta1^t)) (1), the multiply (1) = 18,
#   relative to the update.  m' itself is NOT bounded relatively (m and c1 (g - m) may cancel), so its
#   absolute bound E_m is carried through: E_p = u |p'| (the final add) + K_P u |p' - p| + step E_m / denom.
K_P = 18
# t' = t ema + p' (1 - ema): per term the constant (1), the multiply (1) and the add (1) = 3, relative to
#   |t ema| + |p' (1 - ema)| (the constant's rounding multiplies t itself, not the change of t), plus
#   (1 - ema) E_p:  E_t = K_T u (ema |t| + (1 - ema) |p'|) + (1 - ema) E_p.
K_T = 3

MUTATIONS = ("t_minus_1", "t_plus_1", "no_weight_decay", "ema_pre_update", "eps_in_sqrt", "no_coef",
             "bc2_no_sqrt", "ema_in_warmup")


def frag_index(h, k):
    """Position of W1[h][k] in the 16-bit shadow: fragment ((w 4 + t) 24 + ks) is 64 lanes x 8 values,
    lane l holding h = 64 w + 16 t + (l & 15), k = 32 ks + 8 (l >> 4) + j."""
    h, k = np.asarray(h, np.int64), np.asarray(k, np.int64)
    w, t, n = h // 64, (h // 16) % 4, h % 16
    ks, q, j = k // 32, (k // 8) % 4, k % 8
    return ((((w * 4 + t) * 24 + ks) * 64) + n + 16 * q) * 8 + j


def param_of_frag(f):
    """The inverse, as optim.hip's w1_param_of_frag comment states it: f = ((((h>>4) 24 + ks) 64) +
    (h & 15) + 16 q) 8 + j, k = 32 ks + 8 q + j; returns the flat W1 index h 768 + k."""
    f = np.asarray(f, np.int64)
    j, lane, r2 = f % 8, (f // 8) % 64, f // 512
    n, q, ks, ht = lane % 16, lane // 16, r2 % 24, r2 // 24
    return (16 * ht + n) * D + 32 * ks + 8 * q + j


def reference_update(G, p, m, v, teacher, lr, t, weight_decay, max_norm, ema_momentum, warmup, clip=True,
                     beta1=BETA1, beta2=BETA2, eps=EPS):
    """One update in float64.  t: the Adam count after this step."""
    G, p, m, v, teacher = (np.asarray(a, np.float64) for a in (G, p, m, v, teacher))
    norm = math.sqrt(float(np.dot(G, G)))
    coef = min(1.0, max_norm / (norm + 1e-6)) if clip else 1.0
    g = coef * G + weight_decay * p
    m2 = m + (1.0 - beta1) * (g - m)
    v2 = beta2 * v + (1.0 - beta2) * g * g
    step = lr / (1.0 - beta1 ** t)
    denom = np.sqrt(v2) / math.sqrt(1.0 - beta2 ** t) + eps
    p2 = p - step * m2 / denom
    t2 = teacher.copy() if warmup else ema_momentum * teacher + (1.0 - ema_momentum) * p2
    return dict(norm=norm, coef=coef, clip_active=bool(clip and coef < 1.0), G=G, g=g, p0=p, m0=m, t0=teacher,
                m=m2, v=v2, p=p2, teacher=t2, step=step, denom=denom, ema=ema_momentum, wd=weight_decay,
                warmup=bool(warmup))


def f32_norm(G):
    """The clip norm as the kernels form it: double sums of the squares over 1024-element blocks, each
    rounded to float; their double sum; the square root rounded to float."""
    G = np.asarray(G, F)
    sq = G.astype(np.float64) ** 2
    pad = (-sq.size) % 1024
    parts = np.concatenate([sq, np.zeros(pad)]).reshape(-1, 1024).sum(axis=1).astype(F)
    return F(math.sqrt(float(parts.astype(np.float64).sum())))


def f32_restatement(G, p, m, v, teacher, lr, t, weight_decay, max_norm, ema_momentum, warmup, clip=True,
                    mutation=None):
    """adam_ema_apply in np.float32, operation by operation, with the constants as dad_config_for
    rounds them to c_float.  mutation: None or one of MUTATIONS."""
    assert mutation is None or mutation in MUTATIONS, mutation
    G, p, m, v, teacher = (np.asarray(a, F) for a in (G, p, m, v, teacher))
    tt = t - 1 if mutation == "t_minus_1" else t + 1 if mutation == "t_plus_1" else t
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        step = F(lr / (1 - BETA1 ** tt)) if tt > 0 else F(np.inf)
        bc2 = 1 - BETA2 ** tt
        bc2s = F(bc2) if mutation == "bc2_no_sqrt" else F(math.sqrt(bc2))
        c1, b2, c2, eps = F(1 - BETA1), F(BETA2), F(1 - BETA2), F(EPS)
        wd = F(0.0) if mutation == "no_weight_decay" else F(weight_decay)
        ema, ema1 = F(ema_momentum), F(1.0 - ema_momentum)
        norm = f32_norm(G)
        coef = F(1.0)
        if clip and mutation != "no_coef":
            coef = min(F(max_norm) / (norm + F(1e-6)), F(1.0))
        g = G * coef
        g = g + wd * p
        m2 = m + c1 * (g - m)
        v2 = v * b2 + c2 * g * g
        if mutation == "eps_in_sqrt":
            denom = np.sqrt(v2 + eps) / bc2s
        else:
            denom = np.sqrt(v2) / bc2s + eps
        p2 = p + (-step) * (m2 / denom)
        src = p if mutation == "ema_pre_update" else p2
        t2 = teacher.copy() if (warmup and mutation != "ema_in_warmup") else teacher * ema + src * ema1
    for a in (g, m2, v2, denom, p2, t2):
        assert a.dtype == F
    return dict(norm=float(norm), coef=float(coef), m=m2, v=v2, p=p2, teacher=t2)


def bounds(ref):
    """Error bounds of a float32 evaluation against `ref` (reference_update's dict): absolute, per
    element, for m, v, p and teacher; `norm_rel` relative for the clip norm."""
    kc = K_COEF if ref["clip_active"] else 0
    kg = kc + 2
    assert kg <= K_G
    aG, ap = np.abs(ref["coef"] * ref["G"]), np.abs(ref["wd"] * ref["p0"])
    e_m = K_M * U * (np.abs(ref["m0"]) + aG + ap) + TINY
    e_v = K_V * U * ref["v"] + TINY
    upd = np.abs(ref["p"] - ref["p0"])
    e_p = U * np.abs(ref["p"]) + K_P * U * upd + ref["step"] * e_m / ref["denom"] + TINY
    if ref["warmup"]:
        e_t = np.zeros_like(e_p)
    else:
        ema = ref["ema"]
        e_t = K_T * U * (ema * np.abs(ref["t0"]) + (1.0 - ema) * np.abs(ref["p"])) + (1.0 - ema) * e_p + TINY
    return dict(m=e_m, v=e_v, p=e_p, teacher=e_t, norm_rel=K_N * U)


def worst(got, ref, bnd):
    """Per quantity: (elements out of bounds, the worst error as a multiple of its bound)."""
    out = {}
    for k in ("m", "v", "p", "teacher"):
        err = np.abs(np.asarray(got[k], np.float64) - ref[k])
        with np.errstate(invalid="ignore", divide="ignore"):
            ratio = np.where(bnd[k] > 0, err / np.where(bnd[k] > 0, bnd[k], 1.0), np.where(err > 0, np.inf, 0.0))
        ratio = np.where(np.isfinite(err), ratio, np.inf)
        out[k] = (int((ratio > 1.0).sum()), float(ratio.max()))
    return out


def worst_u(got, ref):
    """The worst error of each quantity in units of u times its natural scale (for reporting): m against
    |m| + |g|, v against v', p against |p'| + |p' - p|, teacher against ema |t| + (1 - ema) |p'|, norm
    against the norm."""
    scale = dict(m=np.abs(ref["m0"]) + np.abs(ref["g"]), v=ref["v"],
                 p=np.abs(ref["p"]) + np.abs(ref["p"] - ref["p0"]),
                 teacher=ref["ema"] * np.abs(ref["t0"]) + (1.0 - ref["ema"]) * np.abs(ref["p"]))
    out = {}
    for k, s in scale.items():
        err = np.abs(np.asarray(got[k], np.float64) - ref[k])
        ok = s > 0
        out[k] = float((err[ok] / s[ok]).max() / U)
    out["norm"] = abs(got["norm"] - ref["norm"]) / ref["norm"] / U
    return out


# ---- the cases (shared by the CPU test and the GPU tests) -----------------------------------------
HYPER = dict(lr=5e-4, weight_decay=1e-5, max_norm=1.0, ema_momentum=0.995)
#            gradient norm, Adam count after the step, warm-up, fresh moments
CASES = {"clip_inactive": (0.5, 9, False, False), "clip_active": (7.0, 9, False, False),
         "fresh": (0.5, 1, False, True), "late": (7.0, 20000, False, False), "warmup": (7.0, 9, True, False)}
_CASES = {}


def flat(parts):
    return np.concatenate([np.asarray(a, F).reshape(-1) for a in parts])


def gradient(seed, norm):
    """Seeded normal gradient of the given 2-norm; about 10 % of W1's rows (dead hidden units) are
    exactly zero, and so are those units' bias gradients."""
    rs = np.random.RandomState(seed)
    G = rs.standard_normal(NPARAM)
    dead = rs.rand(H) < 0.1
    G[:NW1].reshape(H, D)[dead] = 0.0
    G[NW1:NW1 + H][dead] = 0.0
    G *= norm / np.linalg.norm(G)
    G = G.astype(F)
    assert (G[:NW1].reshape(H, D)[dead] == 0).all() and dead.sum() > 10
    return G


def make_case(name):
    """(inputs, keyword arguments) of a case: inputs = dict(G, p, m, v, teacher) as float32 flat vectors
    over [W1 | b1 | W2 | b2], from oracle.synth's seeded training state; computed once, never changed."""
    if name not in _CASES:
        norm, t, warmup, fresh = CASES[name]
        st = synth.make_state(40, 1)
        inp = dict(G=gradient(1000 + sorted(CASES).index(name), norm), p=flat(st["student"]),
                   teacher=flat(st["teacher"]), m=flat(st["exp_avg"]), v=flat(st["exp_avg_sq"]))
        if fresh:
            inp["m"], inp["v"] = np.zeros(NPARAM, F), np.zeros(NPARAM, F)
        for a in inp.values():
            a.setflags(write=False)
        _CASES[name] = (inp, dict(HYPER, t=t, warmup=warmup))
    return _CASES[name]


_REFS = {}


def case_reference(name):
    """(reference_update's result, its bounds) of a case, computed once."""
    if name not in _REFS:
        inp, kw = make_case(name)
        ref = reference_update(inp["G"], inp["p"], inp["m"], inp["v"], inp["teacher"], **kw)
        _REFS[name] = (ref, bounds(ref))
    return _REFS[name]
