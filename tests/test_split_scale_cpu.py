"""The conditions tests/test_gpu_split_scale.py relies on, asserted on tests/split_scale.py's case and references
alone (no device), and the wrong-answer controls: each mutant of a NumPy restatement moves a compared integer or lies
at least 10x outside the bound the GPU module applies (the factor is printed)."""
import numpy as np
import pytest
import torch

import dadpkg
import exact_problem as X
import models_ref as mr
import noise_ref as nr
import split_scale as S
import windows_ref as wr

PKG = dadpkg.pkg()
L_ = PKG._lib
E = PKG.evaluate
FACTOR = 10.0


def _sizes():
    return S.split()[1]


def _labels():
    return S.split()[3]


# ---- the case -----------------------------------------------------------------------------------------------------
def test_lengths_and_slab_tables_are_the_ones_the_case_is_about():
    sizes, soff = _sizes(), nr.slab_prefix(_sizes())
    assert len(sizes) == S.N == 513 and not sizes[[0, 1, 2, 253, 254, 257, 258, 510, 511]].any()
    assert list(sizes[[255, 256, 259, 300, 512]]) == [331, 1, 1025, 300, 2]
    below = set(int(v) for v in sizes[:128])
    assert {31, 32, 33, 63, 64, 65, 96, 97, 128, 129} <= below
    free = np.array([i for i in range(S.N) if i not in S.FIXED])
    assert sizes[free].min() >= 1 and sizes[free].max() <= 5
    assert soff[257] % 2 == 1 and soff[513] % 2 == 0 and soff[513] > 500          # both parities of the pair kernel
    assert soff[260] - soff[259] == 33 and soff[256] - soff[255] == 11 and soff[301] - soff[300] == 10
    rows, lens, slab_off = E.plan_host(sizes, S.split()[2])
    np.testing.assert_array_equal(slab_off, soff)
    # the longest run of equal slab-table entries: the three empty utterances 0 - 2 and their successor, the owner
    runs = np.diff(np.flatnonzero(np.diff(np.concatenate([[-1], soff[:-1], [-2]])) != 0))
    assert runs.max() == 4 and runs[0] == 4 and (runs == 3).sum() == 3
    utt, c = E.slab_jobs(slab_off)                        # the kernel's owner rule gives the restatement's owners
    assert (sizes[utt] > 0).all() and c.max() == 32
    labels = _labels()
    assert sorted(np.flatnonzero(labels < 0)) == sorted(S.UNLABELLED) and (np.array(S.UNLABELLED) >= 256).sum() >= 2
    assert set(labels[256:]) >= {0, 1, 2, 3} and labels[256] >= 0 and labels[512] >= 0
    perm = S.order("perm")
    assert sorted(perm) == list(range(S.N)) and (np.diff(perm) < 0).any()


def test_every_operand_is_on_the_grid_and_every_preactivation_exact():
    feats, sizes, offsets, labels, noise = S.split()
    assert np.array_equal(feats * 8, np.round(feats * 8)) and np.abs(feats).max() <= 16
    assert np.array_equal(noise, np.round(noise)) and np.abs(noise).max() == 3
    for s in S.SIGMAS:                                     # sigma * integer noise stays on the 2^-3 grid
        assert s * 8 == round(s * 8)
    ax = np.abs(feats).astype(np.float64) + max(S.SIGMAS) * 3.0
    nets = S.networks()
    assert len(nets) == 8
    for W1, b1, W2, b2 in nets:
        W1, b1 = np.asarray(W1, np.float64), np.asarray(b1, np.float64)
        assert np.array_equal(W1 * 1024, np.round(W1 * 1024)) and np.abs(W1).max() < 2.0 ** -4      # 6 bits
        assert np.array_equal(np.abs(b1 * 2 ** 14) % 2, np.ones(len(b1)))                          # odd multiples
        assert (ax @ np.abs(W1).T).max() + np.abs(b1).max() < 1024.0
        assert np.array_equal(W1.astype(np.float16).astype(np.float64), W1)
    for a in (feats, noise):                               # lossless in both 16-bit store types
        assert np.array_equal(a.astype(np.float16).astype(np.float32), a)
        assert torch.equal(torch.from_numpy(a).to(torch.bfloat16).float(), torch.from_numpy(a))
    # float32 pre-activations in a scrambled order equal the float64 ones
    W1, b1 = nets[0][:2]
    col = np.random.RandomState(1).permutation(768)
    pre32 = np.zeros((64, 256), np.float32)
    for d in col:
        pre32 += feats[:64, d:d + 1] * W1[:, d][None, :]
    pre64 = feats[:64].astype(np.float64) @ np.asarray(W1, np.float64).T
    assert np.array_equal(pre32.astype(np.float64), pre64)


def test_the_networks_predict_several_classes_on_both_sides_of_256():
    sizes = _sizes()
    for k in (0, 1):
        ref = S.reference(k)
        counts = np.bincount(ref["pred"], minlength=4)
        print("network %d predicts %s (%s at index >= 256)" % (k, counts, np.bincount(ref["pred"][256:], minlength=4)))
        assert (counts > 0).sum() >= 3 and (np.bincount(ref["pred"][256:], minlength=4) > 0).sum() >= 2
        ok = S.decided(ref, sizes)
        lim = S.limits(ref, sizes)
        live = sizes > 0
        print("  smallest top-two gap %.3e, largest logit bound %.3e" % (ref["gap"][live].min(), lim["eps_z"].max()))
        assert ok.all()                                    # so the GPU test compares WHOLE confusion matrices
        assert (ref["emb"] >= 0).all() and ref["emb"][live].max(1).min() > 0 and not ref["emb"][~live].any()
    dis = (S.reference(0)["pred"] != S.reference(1)["pred"])
    assert dis[:256].any() and dis[256:].any()


def test_the_long_utterance_needs_all_its_slabs():
    _, sizes, offsets, _, _ = S.split()
    ref = S.reference(0)
    lim = S.limits(ref, sizes)["emb"]
    cut = S.pooled(S.hidden(0), sizes, offsets, "first32")
    f = X.worst(cut[259] - ref["emb"][259], lim[259])
    print("utterance 259 on its first 32 slabs: %.3g x the bound" % f)
    assert f >= FACTOR and np.array_equal(np.delete(cut, 259, 0), np.delete(ref["emb"], 259, 0))


def _members(K, n):
    """models_ref.block on the float32 roundings of the references of the first K networks, first n utterances."""
    refs = [S.reference(k) for k in range(K)]
    probs = np.stack([r["probs"][:n] for r in refs]).astype(np.float32)
    pred = np.stack([r["pred"][:n] for r in refs])
    score = np.stack([r["score_entropy"][:n] for r in refs]).astype(np.float32)
    return probs, pred, score


def _noise_pred():
    return S.noise_reference(0)["pred"]


def _window_summary(n, hop=32, span=1, mode="prefix"):
    ref = S.windows_reference(hop, span, mode)
    off = ref["win_off"][:n + 1]
    w_pred, w_probs = ref["pred"][:off[-1]], ref["probs"][:off[-1]].astype(np.float32)
    return w_pred, off, wr.summaries(w_pred, w_probs, off, _sizes()[:n], hop, span, mode)


@pytest.mark.parametrize("n", [257, 513])
def test_the_utterances_past_256_reach_every_compared_confusion_row(n):
    labels = _labels()[:n]
    preds = {"student": S.reference(0)["pred"][:n], "teacher": S.reference(1)["pred"][:n]}
    for k, p in enumerate(_noise_pred()):
        preds["noise level %d" % k] = p[:n]
    probs, pred, score = _members(8, n)
    for m, p in enumerate(mr.block(L_, probs, pred, score, labels)["member_pred"]):
        preds["member %d of 8" % m] = p
    for m, p in enumerate(mr.block(L_, probs[:3], pred[:3], score[:3], labels)["member_pred"][3:]):
        preds["ensemble / vote %d of 3" % m] = p
    _, _, summ = _window_summary(n)
    for key in ("mean_pred", "vote_pred", "last_pred"):
        preds["windows " + key] = np.maximum(summ[key], 0)
    for name, p in preds.items():
        whole, head = S.confusion(labels, p), S.confusion(labels[:256], p[:256])
        if n == 257:
            assert not np.array_equal(whole, head), name      # one utterance: the block changes without it
        else:
            assert ((whole - head).sum(1) > 0).all(), name


# ---- the wrong-answer controls ------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [257, 513])
def test_control_result_pass_stops_at_256(n):
    labels = _labels()
    for k in (0, 1):
        p = S.reference(k)["pred"]
        moved = np.abs(S.confusion(labels[:n], p[:n]) - S.confusion(labels[:256], p[:256])).sum()
        print("n = %d, network %d: %d confusion counts moved" % (n, k, moved))
        assert moved > 0
    d = S.reference(0)["pred"] != S.reference(1)["pred"]
    if n == 513:
        assert d[:n].sum() != d[:256].sum()
    pn = _noise_pred()
    c_all, _ = nr.block(L_, pn[:, :n], *[np.zeros((3, n), np.float32)] * 3, labels[:n])
    c_cut, _ = nr.block(L_, pn[:, :256], *[np.zeros((3, 256), np.float32)] * 3, labels[:256])
    for slot in (L_.EN_CONF, L_.EN_CONF + 16, L_.EN_CONF + 32):
        assert not np.array_equal(c_all[slot:slot + 16], c_cut[slot:slot + 16])
    if n == 513:
        assert c_all[L_.EN_FLIPS + 2] != c_cut[L_.EN_FLIPS + 2] and c_all[L_.EN_SURVIVE + 2] != c_cut[L_.EN_SURVIVE + 2]


def _pair_tables(counts):
    return np.concatenate([counts[L_.EM_DISAGREE:L_.EM_DISAGREE + 100], counts[L_.EM_ONLY:L_.EM_ONLY + 100]])


@pytest.mark.parametrize("K", [3, 8])
@pytest.mark.parametrize("n", [257, 513])
def test_control_last_wave_dropped(n, K):
    """n rounded down to a multiple of 64 in the pair counts"""
    labels = _labels()
    probs, pred, score = _members(K, n)
    m = n // 64 * 64
    a = _pair_tables(mr.block(L_, probs, pred, score, labels[:n])["counts"])
    b = _pair_tables(mr.block(L_, probs[:, :m], pred[:, :m], score[:, :m], labels[:m])["counts"])
    print("n = %d, K = %d: %d pair counts moved" % (n, K, (a != b).sum()))
    assert (a != b).any()


@pytest.mark.parametrize("K", [3, 8])
@pytest.mark.parametrize("n", [255, 257, 513])
def test_control_partial_wave_counted_whole(n, K):
    """the lanes past n of the last wave counted too (as utterances of class 0 that every member gets right)"""
    labels = _labels()
    probs, pred, score = _members(K, n)
    pad = -n % 64
    assert pad > 0
    a = _pair_tables(mr.block(L_, probs, pred, score, labels[:n])["counts"])
    one = np.zeros((K, pad, 4), np.float32)
    one[..., 0] = 1.0
    b = _pair_tables(mr.block(L_, np.concatenate([probs, one], 1), np.concatenate([pred, np.zeros((K, pad), np.int64)], 1),
                              np.concatenate([score, np.ones((K, pad), np.float32)], 1),
                              np.concatenate([labels[:n], np.zeros(pad, np.int64)]))["counts"])
    print("n = %d, K = %d: %d pair counts moved" % (n, K, (a != b).sum()))
    assert (a != b).any()


@pytest.mark.parametrize("variant,n", [("owner_run_first", 257), ("owner_run_first", 513), ("first16", 513),
                                       ("drop_last", 257), ("drop_last", 513), ("pair_second_lost", 257),
                                       ("pair_second_lost", 513)])
def test_control_slab_walks(variant, n):
    """The owner search off by one inside a run of empty utterances, the head stopping after 16 slabs or dropping
    the last one, the pair kernel losing its second job behind an utterance's last slab."""
    _, sizes, offsets, _, _ = S.split()
    sizes, offsets = sizes[:n], offsets[:n]
    for k in (0, 1):
        ref = S.rows(S.reference(k), np.arange(n))
        lim = S.limits(ref, sizes)
        wrong = S.heads(S.pooled(S.hidden(k), sizes, offsets, variant), S.networks()[k])
        fe = X.worst(wrong["emb"] - ref["emb"], lim["emb"])
        fz = X.worst(wrong["logits"] - ref["logits"], lim["logits"])
        hit = np.flatnonzero(np.abs(wrong["emb"] - ref["emb"]).max(1) > 0)
        print("%s, n = %d, network %d: %d utterance(s) move; embeddings %.3g x, logits %.3g x the bound"
              % (variant, n, k, len(hit), fe, fz))
        assert fe >= FACTOR and fz >= FACTOR
        if variant == "first16":
            assert list(hit) == [259]                      # (n = 257 holds no utterance of more than 11 slabs)
        if variant == "owner_run_first":
            assert wrong["emb"][0].any() and not wrong["emb"][3].any()
    assert np.array_equal(S.pooled(S.hidden(0), sizes, offsets), S.reference(0)["emb"][:n])


@pytest.mark.parametrize("hop,span,mode", S.WINDOW_CASES)
@pytest.mark.parametrize("n", [257, 513])
def test_control_window_summaries_stop_at_256(n, hop, span, mode):
    labels = _labels()[:n]
    w_pred, off, summ = _window_summary(n, hop, span, mode)
    right = wr.block(L_, w_pred, summ, off, labels)
    cut = {k: v.copy() for k, v in summ.items()}
    for k in ("mean_pred", "vote_pred", "last_pred", "settle", "switches"):
        cut[k][256:] = 0                                   # what a zero-filled buffer would hold
    cut["settle_frames"][256:] = 0
    wrong = wr.block(L_, w_pred, cut, off, labels)
    print("(%d, %d, %s), n = %d: %d block words moved" % (hop, span, mode, n, (right != wrong).sum()))
    assert (right != wrong).any()
    if n == 513 and hop == 1:
        assert summ["J"][259] == 1025 > L_.EW_CURVE          # the long utterance runs past the 64 curve slots
