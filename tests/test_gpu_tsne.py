"""Exact t-SNE on the MI355X (evaluate.tsne* + csrc/tsne.hip) against the float64 restatement tests/tsne_ref.py
(computed once per input on the CPU) and the scikit-learn fixture tests/golden/eval_tsne.npz: the three stages one
by one, the whole run, the stop rules, poison / determinism / graph capture, and the Python surface.

Every bound is either derived from the float32 format (u = 2^-24) and the shapes, or a multiple of what the float32
CPU restatement deviates from the float64 one (measured on the reference, stored in the fixture or recomputed here
by the same function); none comes from what the kernels gave."""
import functools
import os

import numpy as np
import pytest
import torch

import dadpkg
import gpu_harness as gh
import tsne_ref as R
from oracle import data_oracle as do

pytestmark = pytest.mark.gpu
PKG = dadpkg.pkg()
D = PKG.data
E = PKG.evaluate
L = PKG._lib
GOLDEN = os.path.join(dadpkg.ROOT, "tests", "golden", "eval_tsne.npz")
U = 2.0 ** -24
FIXTURE_N = (65, 129, 257)


@functools.lru_cache(None)
def _golden():
    return dict(np.load(GOLDEN))


def _synthetic(n, seed):
    """Post-ReLU-like embeddings 0.5 + 0.1 |N(0, 1)| plus a class offset, one exact duplicate row."""
    rs = np.random.RandomState(seed)
    labels = rs.randint(0, 4, n)
    offsets = 0.08 * rs.standard_normal((4, 256))
    emb = (0.5 + 0.1 * np.abs(rs.standard_normal((n, 256))) + offsets[labels]).astype(np.float32)
    src, dst = rs.permutation(n)[:2]
    emb[dst] = emb[src]
    return emb, np.array([src, dst])


@functools.lru_cache(None)
def _case(n):
    """{'emb', 'dup', 'perplexity', 'P' (float64 restatement), 'D', 'dev_p'}; computed once, never modified."""
    g = _golden()
    if n in FIXTURE_N:
        key = "n%d_" % n
        emb, dup, perp = g[key + "emb"], g[key + "dup"], float(g[key + "perplexity"])
    else:
        emb, dup = _synthetic(n, 400 + n)
        perp = 2.0 if n == 7 else 5.0
    Dm = R.sq_distances(emb)
    P, _ = R.joint_probabilities(Dm, perp)
    if n in FIXTURE_N:
        dev = float(g["n%d_dev_p" % n])
    else:
        dev = R.p_deviation(R.joint_probabilities_f32(emb, perp)[0], P)
    return {"emb": emb, "dup": dup, "perplexity": perp, "P": P, "D": Dm, "dev_p": dev}


@functools.lru_cache(None)
def _device_p(n):
    """(P device tensor [n, ld], beta float64 array) of case n; computed once, never modified."""
    c = _case(n)
    P, beta = E.tsne_affinities(torch.from_numpy(c["emb"]).cuda(), c["perplexity"], beta=True)
    return P, beta.cpu().numpy()


@functools.lru_cache(None)
def _points(n, which):
    """Y0 ('y0', exaggeration 12) or the late, spread-out Y ('late', exaggeration 1) for n rows: the fixture's own for
    its cases, the first n rows of case 65's below it."""
    g = _golden()
    src = n if n in FIXTURE_N else 65
    y = g["n%d_%s" % (src, "y0" if which == "y0" else "ylate")][:n]
    return np.ascontiguousarray(y, dtype=np.float32), (12.0 if which == "y0" else 1.0)


def _bits(t):
    return t.detach().cpu().contiguous().numpy().view(np.uint32)


# ---------------------------------------------------------------- 1. affinities
# (577 rows are 10 row tiles: the distance kernel's workgroups then take more than one column tile each)
@pytest.mark.parametrize("n", [7, 63, 64, 65, 129, 257, 577])
def test_affinities(n):
    c = _case(n)
    Pd, beta = _device_p(n)
    assert tuple(Pd.shape) == (n, L.ts_ld(n))
    P = Pd.cpu().numpy()
    Pm = P[:, :n]
    assert np.array_equal(Pm.view(np.uint32), Pm.T.copy().view(np.uint32)), "P is not bit-symmetric"
    assert not np.diag(Pm).any() and not P[:, n:].any()
    total = Pm.astype(np.float64).sum()
    err = np.abs(Pm.astype(np.float64) - c["P"]) / c["P"].max(1, keepdims=True)
    # the entropy each row's beta gives on the exact distances
    a = c["emb"].astype(np.float64) - c["emb"].astype(np.float64).mean(0)
    na = np.sqrt((a * a).sum(1))
    dD = 260 * U * (na[:, None] + na[None, :]).max(1) ** 2
    H = R.entropy_of_rows(c["D"], beta)
    hdev = np.abs(H - np.log(c["perplexity"]))
    print("n=%d: |sum P - 1| %.3e (bound %.3e)  |P - ref| / rowmax %.3e (bound %.3e)  entropy %.3e (bound %.3e)"
          % (n, abs(total - 1), (n + 16) * U, err.max(), 4 * c["dev_p"], hdev.max(), (1e-5 + 2 * beta * dD).min()))
    assert abs(total - 1.0) <= (n + 16) * U
    assert err.max() <= 4 * c["dev_p"]
    assert (hdev <= 1e-5 + 2 * beta * dD).all()
    # the duplicate rows: the same row up to their swap
    s, d = c["dup"]
    swapped = Pm[d].copy()
    swapped[[s, d]] = swapped[[d, s]]
    assert np.array_equal(Pm[s].view(np.uint32), swapped.view(np.uint32))
    assert beta[s] == beta[d]


# ---------------------------------------------------------------- 2. one evaluation
@pytest.mark.parametrize("which", ["y0", "late"])
@pytest.mark.parametrize("n", [63, 64, 65, 129, 257])
def test_one_evaluation(n, which):
    Pd, _ = _device_p(n)
    Y, ex = _points(n, which)
    ref = R.kl_and_gradient(Pd.cpu().numpy()[:, :n].astype(np.float64), Y, ex)
    assert not ref["clamped"]
    gbound = 4 * U * ((n + 16) * ref["Sa"] + (3 * n + 32) * ref["Sr"] / ref["Z"])
    Yd = torch.from_numpy(Y).cuda()
    runs = {}
    for chunks in (1, 3, 0):
        r = E.tsne_gradient(Pd, Yd, ex, _chunks=chunks)
        g = r["grad"].cpu().numpy().astype(np.float64)
        gerr = np.abs(g - ref["grad"])
        print("n=%d %s chunks=%d: grad err / bound %.3f  (bound / max|grad| %.2e)  Z rel %.3e (bound %.3e)  "
              "KL err %.3e (bound %.3e)" % (n, which, chunks, (gerr / gbound).max(), gbound.max() / np.abs(ref["grad"]).max(),
                                            abs(r["z"] / ref["Z"] - 1), (2 * n + 16) * U, abs(r["kl_divergence"] - ref["kl"]),
                                            (n + 16) * U * ref["kl_scale"]))
        assert (gerr <= gbound).all()
        assert abs(r["z"] / ref["Z"] - 1) <= (2 * n + 16) * U
        assert abs(r["kl_divergence"] - ref["kl"]) <= (n + 16) * U * ref["kl_scale"]
        gn = np.sqrt((g * g).sum())
        assert abs(r["grad_norm"] / gn - 1) <= 1e-12
        runs[chunks] = r
    # against scikit-learn's own numbers, where the fixture has them.  Its P differs from the device's by at most
    # dP_i = 4 dev_p rowmax_i per entry (test_affinities), which moves grad_i by at most 4 ex dP_i sum_j w_ij |y_i - y_j|
    # and the error by at most ex sum_ij dP_i (|log p| + |log w| + |log Z| + 1)
    if n in FIXTURE_N:
        g, c = _golden(), _case(n)
        k = "n%d_" % n
        skg = g[k + ("grad0" if which == "y0" else "grad1")]
        skl = float(g[k + ("kl0" if which == "y0" else "kl1")])
        dP = 4 * c["dev_p"] * c["P"].max(1)
        diff = Y.astype(np.float64)[:, None, :] - Y.astype(np.float64)[None, :, :]
        w = 1.0 / (1.0 + (diff * diff).sum(-1))
        off = ~np.eye(n, dtype=bool)
        T = ((w * off)[:, :, None] * np.abs(diff)).sum(1)
        logs = np.abs(np.log(ex * c["P"][off])) + np.abs(np.log(w[off])) + abs(np.log(ref["Z"])) + 1.0
        klb = (n + 16) * U * ref["kl_scale"] + ex * (np.repeat(dP, n - 1) * logs).sum()
        got = runs[0]["grad"].cpu().numpy()
        print("n=%d %s: |grad - scikit-learn| / bound %.3f  |KL - scikit-learn| %.3e (bound %.3e)"
              % (n, which, (np.abs(got - skg) / (gbound + 4 * ex * dP[:, None] * T)).max(),
                 abs(runs[0]["kl_divergence"] - skl), klb))
        assert (np.abs(got - skg) <= gbound + 4 * ex * dP[:, None] * T).all()
        assert abs(runs[0]["kl_divergence"] - skl) <= klb


def test_one_evaluation_across_staged_blocks():
    """2,113 columns in one chunk are two staged blocks of y_j (2,048 + 65); the planner cuts the 34 row tiles into 8
    chunks.  A seeded symmetric P and a spread-out Y."""
    n = 2113
    rs = np.random.RandomState(77)
    Ph = rs.rand(n, n).astype(np.float32) ** 4
    Ph = Ph + Ph.T
    np.fill_diagonal(Ph, 0.0)
    Ph = (Ph / Ph.astype(np.float64).sum()).astype(np.float32)
    Y = (5.0 * rs.standard_normal((n, 2))).astype(np.float32)
    ref = R.kl_and_gradient(Ph.astype(np.float64), Y)
    assert not ref["clamped"] and np.array_equal(Ph, Ph.T)
    gbound = 4 * U * ((n + 16) * ref["Sa"] + (3 * n + 32) * ref["Sr"] / ref["Z"])
    Pd = torch.zeros(n, L.ts_ld(n), device="cuda")
    Pd[:, :n] = torch.from_numpy(Ph).cuda()
    Yd = torch.from_numpy(Y).cuda()
    for chunks in (1, 3, 0):
        r = E.tsne_gradient(Pd, Yd, _chunks=chunks)
        gerr = np.abs(r["grad"].cpu().numpy().astype(np.float64) - ref["grad"])
        print("n=%d chunks=%d: grad err / bound %.3f  Z rel %.3e  KL err %.3e (bound %.3e)"
              % (n, chunks, (gerr / gbound).max(), abs(r["z"] / ref["Z"] - 1), abs(r["kl_divergence"] - ref["kl"]),
                 (n + 16) * U * ref["kl_scale"]))
        assert (gerr <= gbound).all()
        assert abs(r["z"] / ref["Z"] - 1) <= (2 * n + 16) * U
        assert abs(r["kl_divergence"] - ref["kl"]) <= (n + 16) * U * ref["kl_scale"]


def test_two_points_and_coincident_points():
    P = torch.zeros(2, L.ts_ld(2), device="cuda")
    P[0, 1] = P[1, 0] = 0.5
    Y = torch.tensor([[0.25, -1.0], [1.5, 0.5]], device="cuda")
    r = E.tsne_gradient(P, Y)
    ref = R.kl_and_gradient(np.array([[0.0, 0.5], [0.5, 0.0]]), Y.cpu().numpy())
    assert abs(r["z"] / ref["Z"] - 1) <= 20 * U and abs(r["kl_divergence"] - ref["kl"]) <= 18 * U * ref["kl_scale"]
    bound = 4 * U * (18 * ref["Sa"] + 38 * ref["Sr"] / ref["Z"])
    assert (np.abs(r["grad"].cpu().numpy() - ref["grad"]) <= bound).all()
    # two points a rounding apart in a Gram form; coincident here: w is exactly 1 and their mutual force 0
    Y = torch.tensor([[3.0e3, -7.0e3], [3.0e3, -7.0e3]], device="cuda")
    r = E.tsne_gradient(P, Y)
    assert r["z"] == 2.0 and not r["grad"].cpu().numpy().any() and r["grad_norm"] == 0.0


# ---------------------------------------------------------------- 3. the first iterations
@pytest.mark.parametrize("n", FIXTURE_N)
def test_five_iterations_follow_the_float64_trajectory(n):
    g, c = _golden(), _case(n)
    k = "n%d_" % n
    Pd, _ = _device_p(n)
    r = E.tsne(torch.from_numpy(c["emb"]).cuda(), c["perplexity"], max_iter=5, init=torch.from_numpy(g[k + "y0"]), _P=Pd)
    want = g[k + "traj5"]
    dev = np.abs(r["embedding"].cpu().numpy() - want).max() / np.abs(want).max()
    print("n=%d: |Y5 - float64| / max|Y| %.3e (float32 restatement %.3e, bound 16 x)" % (n, dev, g[k + "dev_traj5"]))
    assert r["n_iter"] == 4
    assert dev <= 16 * float(g[k + "dev_traj5"])


# ---------------------------------------------------------------- 4. the whole run
@functools.lru_cache(None)
def _whole_run(n):
    g, c = _golden(), _case(n)
    y0 = torch.from_numpy(g["n%d_y0" % n])
    r = E.tsne(torch.from_numpy(c["emb"]).cuda(), c["perplexity"], init=y0, history=True, _P=_device_p(n)[0])
    assert torch.equal(y0, torch.from_numpy(g["n%d_y0" % n]))          # (init is never modified)
    return r


@pytest.mark.parametrize("n", [129, 257])
def test_whole_run_reaches_the_references_error(n):
    g, c = _golden(), _case(n)
    r = _whole_run(n)
    finals = g["n%d_kl_final_f32" % n]
    ref = R.kl_and_gradient(c["P"], r["embedding"].cpu().numpy())
    assert not ref["clamped"]
    print("n=%d: float64 KL of the device's final Y %.5f; float32 restatement runs %.5f .. %.5f; after exploration %.3f; "
          "scikit-learn %.5f; device kl_divergence %.6f (|d| %.2e, bound %.2e)"
          % (n, ref["kl"], finals.min(), finals.max(), g["n%d_kl_explore" % n], g["n%d_kl_final" % n],
             r["kl_divergence"], abs(r["kl_divergence"] - ref["kl"]), (n + 16) * U * ref["kl_scale"]))
    assert r["n_iter"] == 999 and len(r["history"]) == 20
    assert ref["kl"] <= finals.max() + (finals.max() - finals.min())
    assert abs(r["kl_divergence"] - ref["kl"]) <= (n + 16) * U * ref["kl_scale"]


# ---------------------------------------------------------------- 5. stop rules
def test_gradient_norm_rule_stops_each_phase_at_its_first_check():
    g, c = _golden(), _case(65)
    emb, y0 = torch.from_numpy(c["emb"]).cuda(), torch.from_numpy(g["n65_y0"])
    runs = [E.tsne(emb, c["perplexity"], max_iter=m, init=y0, min_grad_norm=1e9, history=True, _P=_device_p(65)[0])
            for m in (100, 300)]
    for r in runs:
        assert r["n_iter"] == 99 and len(r["history"]) == 2
    assert np.array_equal(_bits(runs[0]["embedding"]), _bits(runs[1]["embedding"]))     # the launches after a stop
    assert runs[0]["kl_divergence"] == runs[1]["kl_divergence"] == runs[0]["history"][-1, 0]


def test_progress_rule_on_the_devices_own_history():
    """scikit-learn's rule, applied on the host to the history of a run that never stops, predicts where the run with
    n_iter_without_progress=50 stops.  The map is chaotic, so which of the pinned learning rates gives the device a
    non-monotone history is not known beforehand: every one is checked, and at least one must stop early."""
    g, c = _golden(), _case(129)
    emb, y0 = torch.from_numpy(c["emb"]).cuda(), torch.from_numpy(g["n129_y0"])
    early = 0
    for lr in R.NONMONOTONE_LRS:
        args = dict(init=y0, learning_rate=lr, history=True, _P=_device_p(129)[0])
        full = E.tsne(emb, c["perplexity"], n_iter_without_progress=10 ** 6, **args)
        r = E.tsne(emb, c["perplexity"], n_iter_without_progress=50, **args)
        assert full["n_iter"] == 999
        want, used = R.predict_n_iter([tuple(h) for h in full["history"]], 1000, n_iter_without_progress=50)
        print("learning rate %g: n_iter %d, predicted %d from %d checks" % (lr, r["n_iter"], want, used))
        assert r["n_iter"] == want and len(r["history"]) == used
        assert np.array_equal(r["history"], full["history"][:used])
        early += want < 999
    assert early, "none of the pinned learning rates gives the device a non-monotone history"


# ---------------------------------------------------------------- 6. robustness
def _raw_run(n, max_iter, poison):
    """Affinities, one evaluation and a run through the enqueue functions, on a workspace and a P that are filled with
    0xFF bytes first (poison) or zeros."""
    g, c = _golden(), _case(n)
    emb = torch.from_numpy(c["emb"]).cuda()
    fill = 0xFF if poison else 0
    ws = E._tsne_workspace(n, emb.device).fill_(fill)
    P = torch.empty(n, L.ts_ld(n), dtype=torch.float32, device="cuda")
    P.view(torch.uint8).fill_(fill)
    E._enqueue_tsne_affinities(emb, c["perplexity"], P, None, ws)
    Y = torch.from_numpy(g["n%d_y0" % n]).cuda()
    ev = E.tsne_gradient(P, Y, 12.0, _ws=ws)
    hist, out = E.tsne_run_buffers(n, max_iter, emb.device)
    E.enqueue_tsne_run(P, Y, hist, out, ws, max_iter=max_iter)
    torch.cuda.synchronize()
    return P, ev, Y, hist, out


def test_poisoned_workspace_and_padding_change_no_bit_and_two_runs_agree():
    a, b, p = _raw_run(65, 60, False), _raw_run(65, 60, False), _raw_run(65, 60, True)
    for other in (b, p):
        assert np.array_equal(_bits(a[0]), _bits(other[0]))
        assert np.array_equal(_bits(a[1]["grad"]), _bits(other[1]["grad"]))
        assert a[1]["kl_divergence"] == other[1]["kl_divergence"] and a[1]["z"] == other[1]["z"]
        assert np.array_equal(_bits(a[2]), _bits(other[2]))
        assert a[3].cpu().numpy().tobytes() == other[3].cpu().numpy().tobytes()
        assert a[4].cpu().numpy().tobytes() == other[4].cpu().numpy().tobytes()
    assert int(a[4][L.TS_N_ITER]) == 59 and int(a[4][L.TS_N_CHECKS]) == 1


def test_poisoned_padding_of_a_given_p_changes_no_bit():
    Pd, _ = _device_p(65)
    Y, ex = _points(65, "late")
    Yd = torch.from_numpy(Y).cuda()
    want = E.tsne_gradient(Pd, Yd, ex)
    bad = Pd.clone()
    bad[:, 65:] = float("nan")
    got = E.tsne_gradient(bad, Yd, ex)
    assert np.array_equal(_bits(want["grad"]), _bits(got["grad"])) and want["kl_divergence"] == got["kl_divergence"]


def test_captured_run_replays_like_eager():
    g, c = _golden(), _case(65)
    n, Pd = 65, _device_p(65)[0]
    y0 = torch.from_numpy(g["n65_y0"]).cuda()
    want = E.tsne(torch.from_numpy(c["emb"]).cuda(), c["perplexity"], max_iter=60, init=y0, _P=Pd)
    ws = E._tsne_workspace(n, y0.device)
    hist, out = E.tsne_run_buffers(n, 60, y0.device)
    Y = torch.empty_like(y0)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        Y.copy_(y0)
        E.enqueue_tsne_run(Pd, Y, hist, out, ws, max_iter=60)      # (warm-up on the capture's stream)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        Y.copy_(y0)
        E.enqueue_tsne_run(Pd, Y, hist, out, ws, max_iter=60)
    for _ in range(2):
        Y.fill_(-1.0)
        out.fill_(-1.0)
        graph.replay()
        torch.cuda.synchronize()
        assert np.array_equal(_bits(Y), _bits(want["embedding"]))
        assert float(out[L.TS_KL]) == want["kl_divergence"] and int(out[L.TS_N_ITER]) == 59


def test_non_finite_row_raises_with_the_count():
    emb = _case(65)["emb"].copy()
    emb[3, 17] = np.nan
    emb[40, 255] = np.inf
    with pytest.raises(L.DadError, match="2 of 65 row"):
        E.tsne_affinities(torch.from_numpy(emb).cuda(), 5.0)


def test_bad_shapes_are_refused_before_any_launch():
    emb = torch.from_numpy(_case(65)["emb"]).cuda()
    for perp in (65.0, 100.0, 0.0, -1.0):
        with pytest.raises(ValueError, match="perplexity"):
            E.tsne_affinities(emb, perp)
    with pytest.raises(ValueError, match="2 <= n"):
        E.tsne_affinities(emb[:1], 0.5)
    with pytest.raises(ValueError, match="2 <= n"):
        E.tsne_affinities(torch.empty(L.TS_MAX_N + 1, 256, device="cuda"), 30.0)
    # the C entry points themselves: a code, and P untouched
    lib = L.lib()
    P = torch.full((65, 128), -3.0, device="cuda")
    ws = E._tsne_workspace(65, emb.device)
    stream = torch.cuda.current_stream().cuda_stream
    assert lib.dad_tsne_affinities(L.ptr(emb), 65, 65.0, L.ptr(P), None, L.ptr(ws), stream) == L.E_ARG
    assert lib.dad_tsne_affinities(L.ptr(emb), 65, float("nan"), L.ptr(P), None, L.ptr(ws), stream) == L.E_ARG
    assert lib.dad_tsne_affinities(L.ptr(emb), 1, 0.5, L.ptr(P), None, L.ptr(ws), stream) == L.E_SHAPE
    assert lib.dad_tsne_affinities(L.ptr(emb), L.TS_MAX_N + 1, 30.0, L.ptr(P), None, L.ptr(ws), stream) == L.E_SHAPE
    assert lib.dad_tsne_affinities(None, 65, 5.0, L.ptr(P), None, L.ptr(ws), stream) == L.E_ARG
    torch.cuda.synchronize()
    assert bool((P == -3.0).all())


# ---------------------------------------------------------------- 7. the Python surface
@pytest.mark.parametrize("n", FIXTURE_N)
def test_pca_init_matches_scikit_learn(n):
    g = _golden()
    got = E.tsne_pca_init(torch.from_numpy(g["n%d_emb" % n]).cuda())
    assert got.dtype == torch.float32 and tuple(got.shape) == (n, 2)
    dev = np.abs(got.cpu().numpy().astype(np.float64) - g["n%d_pca" % n]).max()
    print("n=%d: |pca init - scikit-learn| %.3e at scale %.3e" % (n, dev, np.abs(g["n%d_pca" % n]).max()))
    assert dev <= 1e-8


@functools.lru_cache(None)
def _model(seed=11):
    stu, tea = do.eval_weights(seed)
    model = PKG.SSRLModel().cuda()
    with torch.no_grad():
        model.student_flat.copy_(torch.from_numpy(gh.flat(stu)))
        model.teacher_flat.copy_(torch.from_numpy(gh.flat(tea)))
    return model


@functools.lru_cache(None)
def _store():
    """A 39-row store of short utterances with labels in [0, 4)."""
    sizes = np.concatenate([[1, 3, 31, 32, 33, 63, 64, 65, 96], np.random.RandomState(13).randint(1, 71, 30)])
    labels = np.random.RandomState(14).randint(0, 4, len(sizes))
    offsets = np.concatenate([[0], np.cumsum(sizes)[:-1]])
    feats = np.random.RandomState(12).standard_normal((int(sizes.sum()), 768)).astype(np.float32)
    return D.FeatureStore(feats, sizes, offsets, labels.astype(np.int64))


@pytest.mark.parametrize("use_teacher", [False, True], ids=["student", "teacher"])
def test_store_path_equals_the_two_step_path(use_teacher):
    model, store = _model(), _store()
    args = dict(perplexity=10.0, max_iter=60)
    got = E.tsne_store(model, store, use_teacher=use_teacher, **args)
    want = E.tsne(E.embed_store(model, store, use_teacher=use_teacher), **args)
    assert tuple(got["embedding"].shape) == (39, 2) and got["n_iter"] == 59
    assert np.array_equal(_bits(got["embedding"]), _bits(want["embedding"]))
    assert got["kl_divergence"] == want["kl_divergence"]


def test_report_of_two_models():
    model, store = _model(), _store()
    other = PKG.SSRLModel().cuda()
    with torch.no_grad():
        other.student_flat.copy_(model.teacher_flat)
        other.teacher_flat.copy_(model.teacher_flat)
    rep = E.tsne_report(model, other, store, perplexity=10.0, max_iter=60)
    assert rep["initial"].shape == rep["trained"].shape == (39, 2) and rep["initial"].dtype == np.float32
    assert np.array_equal(rep["labels"], np.asarray(store.labels))
    assert rep["class_counts"] == [int((np.asarray(store.labels) == c).sum()) for c in range(4)]
    assert np.array_equal(rep["trained"], E.tsne_store(model, store, use_teacher=True, perplexity=10.0,
                                                       max_iter=60)["embedding"].cpu().numpy())
    assert PKG.tsne is E.tsne and PKG.tsne_report is E.tsne_report
