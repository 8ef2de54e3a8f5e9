"""One split of 513 utterances on tests/exact_problem.py's dyadic grid, for the four store-fed evaluators that share
csrc/eval_rows.h (dad_eval_split, dad_eval_noise, dad_eval_windows, dad_eval_models), with float64 references and
the NumPy restatements the wrong-answer controls mutate (TEST INFRASTRUCTURE; tests/test_split_scale_cpu.py asserts
every condition on the reference alone, tests/test_gpu_split_scale.py holds the device to it).

Why: the evaluators' other tests use splits of 37 - 41 utterances of at most 96 frames.  There the split-wide result
kernels (one workgroup of 256 threads walking u = tid; u < n; u += 256) never take a second trip, only wave 0 of
dad_models_result's ballot loop runs, dad_window_utt's second block never starts, slab_owner searches a table of
about 80 entries, and no head sums more than three slab partials.

The split (store order; the sub-cases are the prefixes order[:n], n in NS, and one seeded permutation of all 513):
  lengths   0 at 0 - 2 (a run of three equal slab-table entries); 31, 32, 33, 63, 64, 65, 96, 97, 128, 129 at
            8, 19, 30, ... 107; around the first result-pass boundary 0, 0, 331, 1, 0, 0, 1025 at 253 - 259 (331 frames
            = 11 slabs at 255, one frame at 256, 33 slabs at 259); 300 at 300; 0, 0, 2 at 510 - 512; every other
            length seeded in 1 .. 5.  n = 257 gives a slab table of odd length, n = 513 an even one.
  features  multiples of 2^-3 in [-16, 16] (as test_gpu_noise._exact draws them)
  networks  exact_problem.state()'s student and teacher, then exact_problem.state(seed)'s students for further
            seeds: W1 multiples of 2^-10 below 0.05, b1 odd multiples of 2^-14
  noise     integers in [-3, 3], levels SIGMAS = (0, 2^-3, 2^-1)
  labels    seeded in 0 .. 3, -1 at UNLABELLED
Every pre-activation is then an exact odd multiple of 2^-14 in float64, in fp32 in any order and on fp16 / bf16
operands, at every noise level (sigma n W1 is a multiple of 2^-13 and the fused multiply-add behind it exact), so one
bound serves every precision and store type.

Bounds (u = 2^-24; none is a measured number):
  emb      |e - e_ref| <= (len + 2) u |e_ref|                    exact_problem.bound("e"): an empty utterance must be 0
  logits   |z - z_ref| <= (len + H + 8) u (|e_ref| |W2|^T + |b2|)  exact_problem.bound("z")
  probs    |p - p_ref| <= (2 eps_z + (C + 6) u) p_ref, eps_z the row's largest logit bound (operators_ref's head bound)
  score    rtol 1e-5, atol 1e-6 (operators_ref.SCORE_*)
  pred     equal to the float64 argmax wherever the top-two gap exceeds 2 eps_z (at most 5 % of the non-empty
           utterances may fall under it: test_gpu_eval_split._decided's rule; here none does)
  windows  the same with the window's frame count in place of len (test_gpu_windows' exact-operand test)
  sums     (n + 8) 2^-53 sum |terms| (test_gpu_models' bound)
"""
import functools

import numpy as np

import exact_problem as X
import noise_ref as nr
import windows_ref as wr
from oracle import synth

SEED = 77
N = 513
NS = (255, 256, 257, 513)
H, C = synth.H_DIM, synth.N_CLS
FIXED = {0: 0, 1: 0, 2: 0, 253: 0, 254: 0, 255: 331, 256: 1, 257: 0, 258: 0, 259: 1025, 300: 300, 510: 0, 511: 0, 512: 2}
FIXED.update({8 + 11 * k: L for k, L in enumerate((31, 32, 33, 63, 64, 65, 96, 97, 128, 129))})
LONG = (255, 259, 300)                       # the utterances of more than three slabs
UNLABELLED = (5, 100, 260, 301, 509)
SIGMAS = (0.0, 2.0 ** -3, 2.0 ** -1)
# exact_problem.state(seed)'s students are networks 2 .. 7.  Seed 6 comes first: on utterance 256 (all that n = 257
# adds to the first result pass) student and teacher agree on a wrong class and seed 6's network is right, so K = 3
# already moves a pair count there (tests/test_split_scale_cpu.py asserts it).
NET_SEEDS = (6, 4, 5, 7, 8, 9)
SCORE_RTOL, SCORE_ATOL = 1e-5, 1e-6          # operators_ref.SCORE_RTOL / SCORE_ATOL
WINDOW_CASES = ((1, 1, "sliding"), (25, 2, "sliding"), (32, 1, "prefix"), (33, 1, "prefix"))


def block_from_outputs(res, labels, with_teacher):
    """dad_eval_split's result block restated in NumPy from the kernel's own per-utterance outputs."""
    pred = res["pred"].cpu().numpy()
    score = res["score"].cpu().numpy()
    valid = (labels >= 0) & (labels < 4)
    cs = np.zeros((4, 4), np.int64)
    np.add.at(cs, (labels[valid], pred[valid]), 1)
    ct = np.zeros((4, 4), np.int64)
    dis = 0
    if with_teacher:
        tp = res["t_pred"].cpu().numpy()
        np.add.at(ct, (labels[valid], tp[valid]), 1)
        dis = int((pred != tp).sum())
    mom = np.zeros((4, 3))
    for c in range(4):
        v = score[labels == c].astype(np.float64)
        if len(v):
            mom[c] = [len(v), np.mean(v), np.std(v) ** 2]
    return cs, ct, dis, int(valid.sum()), int((~valid).sum()), mom


@functools.lru_cache(None)
def split():
    """(feats f32 [frames, 768], sizes, offsets, labels, noise f32 [32 * slabs, 768] for the store order)."""
    rs = np.random.RandomState(SEED)
    sizes = rs.randint(1, 6, N)
    for i, L in FIXED.items():
        sizes[i] = L
    offsets = np.concatenate([[0], np.cumsum(sizes)[:-1]])
    feats = X.q(np.clip(4.0 * rs.standard_normal((int(sizes.sum()), 768)), -16, 16), 2.0 ** -3)
    labels = rs.randint(0, 4, N).astype(np.int64)
    labels[list(UNLABELLED)] = -1
    noise = rs.randint(-3, 4, (32 * int(nr.slab_prefix(sizes)[-1]), 768)).astype(np.float32)
    return feats, sizes, offsets, labels, noise


def order(case):
    """The subset of a sub-case: a prefix length, or 'perm' (all 513 through a seeded permutation)."""
    return np.random.RandomState(SEED + 1).permutation(N) if case == "perm" else np.arange(int(case))


@functools.lru_cache(None)
def networks():
    """Eight networks (W1, b1, W2, b2) float32: student, teacher, then the further seeds' students."""
    st = X.state()
    return tuple([tuple(st["student"]), tuple(st["teacher"])] + [tuple(X.state(seed=s)["student"]) for s in NET_SEEDS])


@functools.lru_cache(None)
def hidden(k):
    """relu(W1 x_t + b1) of every frame under network k, float64 [frames, 256] (exact on the grid)."""
    W1, b1 = networks()[k][:2]
    hid = wr.hidden64(split()[0], W1, b1)
    hid.setflags(write=False)
    return hid


POOL_VARIANTS = ("owner_run_first", "first16", "first32", "drop_last", "pair_second_lost")


def pooled(hid, sizes, offsets, variant=None):
    """Embeddings [n, 256] the way the kernels build them: one partial sum per 32-frame slab job, job j owned by the
    largest u with slab_off[u] <= j, the owner's partials summed and divided by max(len, 1).  `variant` builds a
    WRONG answer of the controls:
      owner_run_first   the owner search stops at the FIRST entry of a run of equal ones: the empty utterances in
                        front of a non-empty one take its first slab
      first16 / first32 the head sums only an utterance's first 16 / 32 slabs
      drop_last         the head drops the last slab
      pair_second_lost  of the job pairs (2p, 2p + 1) the second is lost when the first is its utterance's last slab"""
    sizes = np.asarray(sizes, np.int64)
    soff = nr.slab_prefix(sizes)
    n, slabs = len(sizes), int(soff[-1])
    owner = np.searchsorted(soff[:-1], np.arange(slabs), side="right") - 1
    emb = np.zeros((n, hid.shape[1]))
    for j in range(slabs):
        u = int(owner[j])
        c = j - int(soff[u])
        part = hid[offsets[u] + 32 * c:offsets[u] + min(32 * c + 32, int(sizes[u]))].sum(0)
        nsl = int(soff[u + 1] - soff[u])
        to = u
        if variant == "owner_run_first" and c == 0:
            to = int(np.searchsorted(soff[:-1], soff[u], side="left"))
        if variant in ("first16", "first32") and c >= int(variant[5:]):
            continue
        if variant == "drop_last" and c == nsl - 1:
            continue
        if variant == "pair_second_lost" and j % 2 == 1 and owner[j - 1] != u:
            continue
        emb[to] += part
    return emb / np.maximum(sizes, 1)[:, None]


def heads(emb, params):
    """noise_ref.heads of embeddings [n, 256] (or [K, n, 256]) under one network's classifier, without the level
    axis where none was given."""
    W2, b2 = (np.asarray(a, np.float64) for a in params[2:])
    one = emb.ndim == 2
    out = nr.heads(emb[None] if one else emb, W2, b2)
    return {k: (v[0] if one and k != "break_level" else v) for k, v in out.items()}


@functools.lru_cache(None)
def reference(k):
    """float64 outputs of network k on all 513 utterances in store order (noise_ref.heads' keys; row i of a sub-case
    is row order(case)[i] of these).  Computed once, never modified."""
    _, sizes, offsets, _, _ = split()
    return heads(pooled(hidden(k), sizes, offsets), networks()[k])


@functools.lru_cache(None)
def noise_reference(k):
    """noise_ref.forward64 of network k on the whole split at SIGMAS: [3, 513, ...] arrays."""
    feats, sizes, offsets, _, noise = split()
    return nr.forward64(feats, noise, sizes, offsets, np.arange(N), SIGMAS, networks()[k])


@functools.lru_cache(None)
def windows_reference(hop, span, mode):
    """windows_ref.forward64 of the student on the whole split (the windows of a prefix are its first win_off[n])."""
    _, sizes, offsets, _, _ = split()
    W2, b2 = networks()[0][2:]
    return wr.forward64(hidden(0), sizes, offsets, np.arange(N), W2, b2, hop, span, mode)


def limits(ref, frames):
    """(emb, logits, probs, score) elementwise bounds and the decided mask of reference rows `ref` whose embeddings
    pool `frames` frames each (module docstring)."""
    T = np.asarray(frames, np.float64)[..., None]
    e_lim = X.bound("e", None, T) * np.abs(ref["emb"])
    z_lim = X.bound("z", None, T) * ref["logit_mag"]
    eps_z = z_lim.max(-1)
    p_lim = (2.0 * eps_z + (C + 6) * X.U32)[..., None] * ref["probs"]
    s_lim = SCORE_ATOL + SCORE_RTOL * np.abs(ref["score_entropy"])
    return dict(emb=e_lim, logits=z_lim, probs=p_lim, score=s_lim, eps_z=eps_z, decided=ref["gap"] > 2.0 * eps_z)


def decided(ref, frames):
    """Rows whose float64 prediction an error within the logit bound cannot change; at most 5 % of the non-empty
    ones may be left out (test_gpu_eval_split._decided's cap, asserted on the reference alone)."""
    ok = limits(ref, frames)["decided"]
    live = np.broadcast_to(np.asarray(frames) > 0, ok.shape)
    assert (~ok & live).sum() <= 0.05 * live.sum(), "the reference itself has %d near-ties" % (~ok & live).sum()
    return ok | ~live          # an empty utterance's logits are b2 itself in float32 and in float64


def rows(ref, idx, axis=0):
    """The utterances `idx` of a reference (axis 1 for the per-level arrays of noise_reference)."""
    return {k: np.take(v, idx, axis=axis) for k, v in ref.items() if k != "break_level"}


def confusion(labels, pred):
    lab = (labels >= 0) & (labels < 4)
    cm = np.zeros((4, 4), np.int64)
    np.add.at(cm, (labels[lab], pred[lab]), 1)
    return cm


def sum_limit(values, n):
    """(n + 8) 2^-53 sum |terms|: the bound on a float64 sum of n float32 terms in any order (test_gpu_models)."""
    return (n + 8) * 2.0 ** -53 * np.abs(np.asarray(values, np.float64)).sum(-1)
