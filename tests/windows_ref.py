"""Reference for dad_eval_windows (TEST INFRASTRUCTURE): window and piece enumeration straight from the
definitions in include/dad.h ("windows of a split"), a float64 forward per window, and the per-utterance
summaries and the DAD_EW_* block restated in NumPy.

Definitions: utterance of L frames, hop h, span m; S = ceil(L / h) hop-segments.
  sliding  J = 0 if L = 0 else max(1, S - m + 1); window j = [j h, min((j + m) h, L))
  prefix   J = S;                                  window j = [0, min((j + 1) h, L))
  pieces   maximal runs of frames inside one 32-frame slab and one hop-segment
"""
import functools

import numpy as np

# the cases of tests/test_gpu_windows.py: (hop, span), in both modes where the span allows
CASES = [(1, 1), (5, 2), (7, 3), (8, 4), (25, 2), (32, 1), (32, 2), (33, 1), (128, 1)]
MODE_CASES = [(h, m, mode) for h, m in CASES for mode in ("sliding", "prefix") if mode == "sliding" or m == 1]
MODE_CASES += [(h, 1, "prefix") for h, m in CASES if m != 1 and (h, 1) not in CASES]
GAP = 2e-4          # a logit error below GAP / 2 cannot change a prediction whose top-two gap exceeds GAP


def windows_brute(L, hop, span, mode):
    """[(start, end)] of one utterance's windows, by walking its hop-segments."""
    segs = []                                   # the hop-segments
    s = 0
    while s * hop < L:
        segs.append((s * hop, min((s + 1) * hop, L)))
        s += 1
    if not segs:
        return []
    if mode == "prefix":
        assert span == 1
        return [(0, e) for _, e in segs]
    if len(segs) < span:
        return [(0, L)]
    return [(segs[j][0], segs[j + span - 1][1]) for j in range(len(segs) - span + 1)]


def pieces_brute(L, hop):
    """[(start, end)] of one utterance's pieces, by walking its frames."""
    out = []
    for t in range(L):
        key = (t // 32, t // hop)
        if out and out[-1][2] == key:
            out[-1][1] = t + 1
        else:
            out.append([t, t + 1, key])
    return [(a, b) for a, b, _ in out]


def layout_brute(sizes, hop, span, mode):
    """(win_off, utt, start, end) of a split's windows by windows_brute."""
    off, utt, st, en = [0], [], [], []
    for i, L in enumerate(sizes):
        w = windows_brute(int(L), hop, span, mode)
        off.append(off[-1] + len(w))
        utt += [i] * len(w)
        st += [a for a, _ in w]
        en += [b for _, b in w]
    return np.array(off, np.int64), np.array(utt, np.int64), np.array(st, np.int64), np.array(en, np.int64)


def hidden64(x, W1, b1):
    """Per-frame rows relu(W1 x_t + b1) in float64, [frames, 256]."""
    return np.maximum(np.asarray(x, np.float64) @ np.asarray(W1, np.float64).T + np.asarray(b1, np.float64), 0.0)


def forward64(hid, sizes, offsets, order, W2, b2, hop, span, mode, end_shift=0, divide_by_span=False):
    """float64 outputs of every window of the subset `order` of a store (hid = hidden64 of the store's rows):
    {'win_off', 'utt', 'start', 'end', 'frames', 'emb', 'esum_abs', 'logits', 'logit_mag', 'probs', 'pred', 'gap',
    'score_entropy', 'score_max'}.  end_shift / divide_by_span build the WRONG references of the controls: a window
    that ends end_shift frames later (where the utterance has them), and a mean over span * hop frames instead of
    the window's own count."""
    sub = np.asarray(sizes)[order]
    win_off, utt, st, en = layout_brute(sub, hop, span, mode)
    W2, b2 = np.asarray(W2, np.float64), np.asarray(b2, np.float64)
    emb = np.zeros((len(utt), hid.shape[1]))
    for w in range(len(utt)):
        i = order[utt[w]]
        e = min(en[w] + end_shift, int(sizes[i])) if end_shift else en[w]
        rows = hid[offsets[i] + st[w]:offsets[i] + e]
        emb[w] = rows.sum(0) / (span * hop if divide_by_span else max(e - st[w], 1))
    z = emb @ W2.T + b2
    zs = z - z.max(1, keepdims=True) if len(z) else z
    p = np.exp(zs)
    p = p / p.sum(1, keepdims=True) if len(z) else p
    top = np.sort(z, 1)[:, ::-1] if len(z) else np.zeros((0, 4))
    ent = -(p * np.log2(p + 1e-8)).sum(1)
    pmax = p.max(1) if len(z) else np.zeros(0)
    return {"win_off": win_off, "utt": utt, "start": st, "end": en, "frames": en - st, "emb": emb, "logits": z,
            "logit_mag": np.abs(emb) @ np.abs(W2).T + np.abs(b2), "probs": p,
            "pred": z.argmax(1) if len(z) else np.zeros(0, np.int64), "gap": top[:, 0] - top[:, 1],
            "score_entropy": pmax * (1 - ent / 2.0), "score_max": pmax}


def decided(ref, min_gap=GAP):
    """Windows whose reference prediction a logit error below min_gap / 2 cannot change; the filter may drop at
    most 5 % of them (asserted on the reference alone)."""
    ok = ref["gap"] > min_gap
    assert (~ok).mean() <= 0.05, "the reference itself has %d of %d near-ties" % ((~ok).sum(), len(ok))
    return ok


def summaries(w_pred, w_probs, win_off, sizes, hop, span, mode):
    """The per-utterance outputs from the per-window predictions and float32 probabilities: {'J', 'mean_probs'
    (float32, summed in window order, / J), 'mean_pred', 'vote_pred', 'last_pred', 'settle', 'switches',
    'settle_frames'}; -1 (mean_probs 0) for an utterance without a window."""
    n = len(sizes)
    w_pred = np.asarray(w_pred, np.int64)
    w_probs = np.asarray(w_probs, np.float32)
    out = {"J": np.diff(win_off).astype(np.int64), "mean_probs": np.zeros((n, 4), np.float32),
           "settle_frames": np.zeros(n, np.int64)}
    for k in ("mean_pred", "vote_pred", "last_pred", "settle", "switches"):
        out[k] = np.full(n, -1, np.int64)
    for u in range(n):
        a, b = int(win_off[u]), int(win_off[u + 1])
        if a == b:
            continue
        pr = w_pred[a:b]
        acc = np.zeros(4, np.float32)
        for row in w_probs[a:b]:
            acc = (acc + row).astype(np.float32)
        out["mean_probs"][u] = acc / np.float32(b - a)
        out["mean_pred"][u] = int(np.argmax(out["mean_probs"][u]))
        out["vote_pred"][u] = int(np.argmax(np.bincount(pr, minlength=4)))
        out["last_pred"][u] = pr[-1]
        differs = np.nonzero(pr != pr[-1])[0]
        out["settle"][u] = differs[-1] + 1 if len(differs) else 0
        out["switches"][u] = int((pr[1:] != pr[:-1]).sum())
        j = int(out["settle"][u])
        out["settle_frames"][u] = min((j + (1 if mode == "prefix" else span)) * hop, int(sizes[u]))
    return out


def block(L, w_pred, summ, win_off, labels, n_nonfinite=0):
    """The DAD_EW_* block (int64 [EW_SLOTS]) from the per-window predictions, summaries() and the labels (None: no
    utterance is labelled).  L = the package's _lib (slot numbers)."""
    n = len(summ["J"])
    out = np.zeros(L.EW_SLOTS, np.int64)
    labels = np.full(n, -1, np.int64) if labels is None else np.asarray(labels, np.int64)
    lab = (labels >= 0) & (labels < 4)
    live = summ["J"] > 0
    for slot, key in ((L.EW_CONF_MEAN, "mean_pred"), (L.EW_CONF_VOTE, "vote_pred"), (L.EW_CONF_LAST, "last_pred")):
        cm = np.zeros((4, 4), np.int64)
        np.add.at(cm, (labels[lab & live], summ[key][lab & live]), 1)
        out[slot:slot + 16] = cm.ravel()
    out[L.EW_N], out[L.EW_N_LABELLED], out[L.EW_N_EMPTY] = n, lab.sum(), (~live).sum()
    out[L.EW_N_WINDOWS], out[L.EW_N_NONFINITE] = win_off[-1], n_nonfinite
    out[L.EW_SETTLE_SUM] = summ["settle"][live].sum()
    out[L.EW_SWITCHES_SUM] = summ["switches"][live].sum()
    out[L.EW_SETTLE_FRAMES_SUM] = summ["settle_frames"][live].sum()
    for u in np.nonzero(lab & live)[0]:
        a, J = int(win_off[u]), int(summ["J"][u])
        for j in range(L.EW_CURVE):
            hit = int(w_pred[a + min(j, J - 1)] == labels[u])
            out[L.EW_CARRIED + j] += hit
            if J > j:
                out[L.EW_REACHED + j] += 1
                out[L.EW_CORRECT + j] += hit
    return out


# ---- the shared inputs of the CPU and GPU modules ------------------------------------------------------------
@functools.lru_cache(None)
def main_inputs():
    """test_gpu_eval_split._inputs('main'): 37 utterances read through a shuffled subset with two repeats."""
    from test_gpu_eval_split import _inputs
    return _inputs("main")


def widen(feats, dt):
    """The store's values as float32: dt 'f32', 'f16' or 'bf16'."""
    import torch
    t = torch.from_numpy(np.ascontiguousarray(feats))
    return t.to({"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}[dt]).float().numpy()


@functools.lru_cache(None)
def main_hidden(dt, net, fp16_operands=False):
    """hidden64 of the main inputs' store of type dt under eval_weights(11)'s student ('s') or teacher ('t');
    with fp16_operands, rows and W1 rounded to fp16 first (the FP16 operand mode).  Computed once."""
    from oracle import data_oracle as do
    feats = main_inputs()[0]
    W1, b1, _, _ = do.eval_weights(11)["st".index(net)]
    x = widen(feats, dt)
    if fp16_operands:
        x, W1 = x.astype(np.float16), np.asarray(W1, np.float32).astype(np.float16)
    return hidden64(x, W1, b1)


@functools.lru_cache(None)
def main_reference(dt, net, hop, span, mode, fp16_operands=False):
    """forward64 of the main inputs; computed once per case, never modified."""
    from oracle import data_oracle as do
    _, sizes, offsets, _, order = main_inputs()
    _, _, W2, b2 = do.eval_weights(11)["st".index(net)]
    return forward64(main_hidden(dt, net, fp16_operands), sizes, offsets, order, W2, b2, hop, span, mode)
