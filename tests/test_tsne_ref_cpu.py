"""tests/tsne_ref.py (the float64 restatement the GPU tests of csrc/tsne.hip compare with) against the scikit-learn
fixture tests/golden/eval_tsne.npz and, where scikit-learn is importable, against its private functions directly;
the mutants that show the first iterations pin the schedule; and the library's host-only t-SNE queries."""
import ctypes
import functools
import os

import numpy as np
import pytest

import dadpkg
import tsne_ref as R

GOLDEN = os.path.join(dadpkg.ROOT, "tests", "golden", "eval_tsne.npz")
CASES = (65, 129, 257)


@functools.lru_cache(None)
def _golden():
    return dict(np.load(GOLDEN))


@functools.lru_cache(None)
def _p(n):
    g = _golden()
    return R.joint_probabilities(R.sq_distances(g["n%d_emb" % n]), float(g["n%d_perplexity" % n]))


@pytest.mark.parametrize("n", [65, 129])
def test_joint_probabilities_match_the_fixture(n):
    P, beta = _p(n)
    want = _golden()["n%d_p" % n]
    off = ~np.eye(n, dtype=bool)
    assert np.array_equal(P, P.T) and not np.diag(P).any()
    assert (np.abs(P - want)[off] / want[off]).max() <= 1e-13
    H = R.entropy_of_rows(R.sq_distances(_golden()["n%d_emb" % n]).astype(np.float32), beta)
    assert np.abs(H - np.log(float(_golden()["n%d_perplexity" % n]))).max() <= 1.0001e-5


@pytest.mark.parametrize("n", CASES)
def test_error_and_gradient_match_the_fixture(n):
    g, k = _golden(), "n%d_" % n
    P, _ = _p(n)
    for y, ex, kl, grad in ((g[k + "y0"], 12.0, g[k + "kl0"], g[k + "grad0"]), (g[k + "ylate"], 1.0, g[k + "kl1"], g[k + "grad1"])):
        r = R.kl_and_gradient(P, y, ex)
        assert not r["clamped"]                       # scikit-learn's Q clamp, which the device leaves out
        assert abs(r["kl"] / float(kl) - 1) <= 1e-12
        # (float64 rounding of sums whose terms cancel near convergence: relative to the terms' size)
        assert (np.abs(r["grad"] - grad) <= 1e-13 * 4 * (r["Sa"] + r["Sr"] / r["Z"])).all()
        # the magnitude sums bound the gradient's own size
        assert (np.abs(r["grad"]) <= 4 * (r["Sa"] + r["Sr"] / r["Z"]) * (1 + 1e-12)).all()


@pytest.mark.parametrize("n", CASES)
def test_duplicate_rows_and_float32_restatement(n):
    g, k = _golden(), "n%d_" % n
    emb, (s, d) = g[k + "emb"], g[k + "dup"]
    assert np.array_equal(emb[s], emb[d])
    D32 = R.gram_sq_distances_f32(emb)
    assert D32[s, d] == 0.0 and (D32 >= 0).all()
    P32, _ = R.joint_probabilities_f32(emb, float(g[k + "perplexity"]))
    assert abs(R.p_deviation(P32, _p(n)[0]) / float(g[k + "dev_p"]) - 1) <= 1e-6     # the fixture's figure, recomputed


@pytest.mark.parametrize("n", CASES)
def test_first_iterations_and_mutants(n):
    """The float64 trajectory of the fixture, and that the bound the GPU test puts on iteration 5 (16 x the float32
    restatement's deviation) separates every mutant of the schedule by at least 100 x."""
    g, k = _golden(), "n%d_" % n
    P, _ = _p(n)
    y0, want = g[k + "y0"], g[k + "traj5"]
    got = R.descend(P, y0, max_iter=5, snapshots=(5,))
    assert got["n_iter"] == 4 and np.abs(got["snapshots"][5] - want).max() <= 1e-12 * np.abs(want).max()
    bound = 16 * float(g[k + "dev_traj5"])
    lr = R.auto_learning_rate(n)
    mutants = {"momentum 0.8 from the start": dict(momentum0=0.8), "no exaggeration": dict(exaggerate=False),
               "gain rule swapped": dict(swap_gains=True), "learning rate doubled": dict(learning_rate=2 * lr)}
    for name, kw in mutants.items():
        y = R.descend(P, y0, max_iter=5, snapshots=(5,), **kw)["snapshots"][5]
        dev = np.abs(y - want).max() / np.abs(want).max()
        assert dev >= 100 * bound, (name, dev, bound)


@pytest.mark.parametrize("n", [129, 257])
def test_fixture_finals_are_far_from_a_stalled_run(n):
    g, k = _golden(), "n%d_" % n
    finals = g[k + "kl_final_f32"]
    limit = finals.max() + (finals.max() - finals.min())
    assert limit < 0.5 * float(g[k + "kl_explore"])           # a run that never drops the exaggeration, or stalls
    assert abs(float(g[k + "kl_final"]) - finals.mean()) <= 2 * (finals.max() - finals.min())    # scikit-learn's own run
    assert int(g[k + "n_iter"]) == 999
    assert not R.kl_and_gradient(_p(n)[0], g[k + "ylate"], sums=False)["clamped"]


def test_pca_init_matches_the_fixture():
    g = _golden()
    for n in CASES:
        assert np.abs(R.pca_init(g["n%d_emb" % n]).astype(np.float64) - g["n%d_pca" % n]).max() <= 1e-8


def test_non_monotone_history_is_pinned():
    """Learning rate 1300 on case 129: the float64 error rises at iterations 599 and 649, so n_iter_without_progress =
    50 stops the run at 649; descend's own stop and predict_n_iter on the unstopped history agree."""
    g = _golden()
    P, _ = _p(129)
    lr = R.NONMONOTONE_LRS[0]
    full = R.descend(P, g["n129_y0"], learning_rate=lr, n_iter_without_progress=10 ** 6)
    err = np.array(full["history"])[:, 0]
    assert full["n_iter"] == 999 and len(err) == 20 and (np.diff(err[5:]) > 0).any()
    want, used = R.predict_n_iter(full["history"], 1000, n_iter_without_progress=50)
    assert (want, used) == (649, 13)
    cut = R.descend(P, g["n129_y0"], learning_rate=lr, n_iter_without_progress=50)
    assert cut["n_iter"] == want and cut["history"] == full["history"][:used]
    assert R.predict_n_iter([(1.0, 0.0)] * 2, 1000, min_grad_norm=1e9) == (99, 2)      # the gradient-norm rule


def test_against_scikit_learn_directly():
    sk = pytest.importorskip("sklearn.manifold._t_sne")
    from scipy.spatial.distance import squareform
    rs = np.random.RandomState(7)
    n = 40
    emb = (0.5 + 0.1 * np.abs(rs.standard_normal((n, 256)))).astype(np.float32)
    D = R.sq_distances(emb)
    P, _ = R.joint_probabilities(D, 7.0)
    Psk = sk._joint_probabilities(D.astype(np.float32), 7.0, 0)
    off = ~np.eye(n, dtype=bool)
    assert (np.abs(P - squareform(Psk))[off] / squareform(Psk)[off]).max() <= 1e-13
    y0 = 1e-4 * rs.standard_normal((n, 2))
    kl, grad = sk._kl_divergence(y0.ravel(), Psk * 12.0, 1.0, n, 2)
    r = R.kl_and_gradient(P, y0, 12.0)
    assert abs(r["kl"] / kl - 1) <= 1e-12 and np.abs(r["grad"].ravel() - grad).max() <= 1e-12 * np.abs(grad).max()
    # _gradient_descent's schedule: 20 exploration iterations from the same start
    p, _, it = sk._gradient_descent(sk._kl_divergence, y0.ravel().copy(), it=0, max_iter=20, n_iter_check=50,
                                    momentum=0.5, learning_rate=50.0, min_gain=0.01, min_grad_norm=1e-7,
                                    args=[Psk * 12.0, 1.0, n, 2])
    mine = R.descend(P, y0, max_iter=20, learning_rate=50.0)
    assert it == 19 and mine["n_iter"] == 19
    assert np.abs(mine["Y"].ravel() - p).max() <= 1e-8 * np.abs(p).max()


def test_host_only_queries_of_the_library():
    p = dadpkg.pkg()
    lib = p._lib.lib()
    ws = p._lib.require("dad_tsne_workspace_bytes", "tsne")
    plan = p._lib.require("dad_tsne_plan", "tsne")
    assert ws(1) == 0 and ws(p._lib.TS_MAX_N + 1) == 0
    sizes = [ws(n) for n in (2, 64, 65, 1100, 5531, p._lib.TS_MAX_N)]
    assert all(a > 0 for a in sizes) and sizes == sorted(sizes)
    rt, ch, per = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    for n, cus in ((2, 256), (65, 256), (1100, 256), (5531, 256), (5531, 8), (p._lib.TS_MAX_N, 304)):
        assert plan(n, cus, ctypes.byref(rt), ctypes.byref(ch), ctypes.byref(per)) == 0
        tiles = -(-n // p._lib.TS_TILE)
        assert rt.value == tiles and 1 <= ch.value <= min(tiles, p._lib.TS_MAX_CHUNKS)
        assert per.value * ch.value >= tiles > per.value * (ch.value - 1)          # every tile once, no empty chunk
    assert (rt.value, p._lib.ts_ld(65), p._lib.ts_ld(64)) == (256, 128, 64)
    assert plan(1, 256, ctypes.byref(rt), ctypes.byref(ch), ctypes.byref(per)) == p._lib.E_SHAPE
    assert plan(p._lib.TS_MAX_N + 1, 256, ctypes.byref(rt), ctypes.byref(ch), ctypes.byref(per)) == p._lib.E_SHAPE
    assert plan(100, 0, ctypes.byref(rt), ctypes.byref(ch), ctypes.byref(per)) == p._lib.E_SHAPE
    assert plan(100, 256, None, ctypes.byref(ch), ctypes.byref(per)) == p._lib.E_ARG
    assert ctypes.sizeof(p._lib.DadTsneArgs) == 32
    assert lib.dad_abi_version() == p._lib.DAD_ABI_VERSION
