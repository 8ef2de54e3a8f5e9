"""Float64 NumPy restatement of scikit-learn 1.7.2's exact t-SNE (sklearn/manifold/_t_sne.py, _utils.pyx), in the
three stages csrc/tsne.hip computes, for tests/test_tsne_ref_cpu.py and tests/test_gpu_tsne.py:

  joint_probabilities(D, perplexity)        _joint_probabilities (as a full n x n matrix) and each row's beta
  kl_and_gradient(P, Y, exaggeration)       _kl_divergence with one degree of freedom, plus the magnitude sums the
                                            GPU tests build their bounds from
  descend(P, Y0, ...)                       TSNE._tsne / _gradient_descent, at a chosen dtype

and the float32 restatement (the arithmetic the device does, on the CPU): gram_sq_distances_f32,
joint_probabilities_f32, and descend(..., dtype=np.float32).
"""
import numpy as np

EPS = float(np.finfo(np.float64).eps)          # scikit-learn's MACHINE_EPSILON
N_ITER_CHECK = 50
EXPLORATION = 250
# Learning rates at which case n = 129's error history is not monotone (tests/test_tsne_ref_cpu.py pins the float64
# one): 1300 rises at iteration 599 in float64 and at 899 in float32, 1000 at 649 in float32, 1600 at 599 in float64.
NONMONOTONE_LRS = (1300.0, 1000.0, 1600.0)


def sq_distances(X):
    """Squared Euclidean distances from the differences, float64, the diagonal exactly 0."""
    X = np.asarray(X, dtype=np.float64)
    D = ((X[:, None, :] - X[None, :, :]) ** 2).sum(-1)
    np.fill_diagonal(D, 0.0)
    return D


def gram_sq_distances_f32(X):
    """The device's distances on the CPU: float32 Gram form on rows centred on their float32 mean, the norms taken
    from the Gram matrix's own diagonal, clamped at 0."""
    X = np.asarray(X, dtype=np.float32)
    mu = X.astype(np.float64).mean(0).astype(np.float32)
    a = X - mu
    G = a @ a.T
    nrm = np.diag(G).copy()
    D = np.maximum((nrm[:, None] + nrm[None, :]) - np.float32(2.0) * G, np.float32(0.0))
    np.fill_diagonal(D, 0.0)
    return D.astype(np.float32)


def entropy_of_rows(D, beta):
    """H_i = log(sum_j e^(-beta_i D_ij)) + beta_i sum_j D_ij c_ij over j != i, float64."""
    D = np.asarray(D, dtype=np.float64)
    off = ~np.eye(D.shape[0], dtype=bool)
    e = np.exp(-D * beta[:, None]) * off
    s = e.sum(1)
    return np.log(s) + beta * (D * e).sum(1) / s


def binary_search(D, perplexity):
    """_binary_search_perplexity: the conditional matrix (float64, diagonal 0) and the beta each row ended with.
    The distances are taken as float32 and the search runs in double, as scikit-learn's does."""
    D = np.asarray(D, dtype=np.float32).astype(np.float64)
    n = D.shape[0]
    desired = np.log(np.float64(np.float32(perplexity)))
    tol, tiny = np.float64(np.float32(1e-5)), np.float64(np.float32(1e-8))     # (C floats in _utils.pyx)
    off = ~np.eye(n, dtype=bool)
    beta = np.ones(n)
    bmin = np.full(n, -np.inf)
    bmax = np.full(n, np.inf)
    used = beta.copy()
    P = np.zeros((n, n))
    active = np.ones(n, dtype=bool)
    for _ in range(100):
        idx = np.where(active)[0]
        if not len(idx):
            break
        b = beta[idx]
        e = np.exp(-D[idx] * b[:, None]) * off[idx]
        s = e.sum(1)
        s[s == 0.0] = tiny
        Pi = e / s[:, None]
        diff = np.log(s) + b * (D[idx] * Pi).sum(1) - desired
        P[idx] = Pi
        used[idx] = b
        done = np.abs(diff) <= tol
        active[idx[done]] = False
        up = idx[~done & (diff > 0.0)]
        dn = idx[~done & ~(diff > 0.0)]
        bmin[up] = beta[up]
        beta[up] = np.where(np.isinf(bmax[up]), beta[up] * 2.0, (beta[up] + bmax[up]) / 2.0)
        bmax[dn] = beta[dn]
        beta[dn] = np.where(np.isinf(bmin[dn]), beta[dn] / 2.0, (beta[dn] + bmin[dn]) / 2.0)
    return P, used


def joint_probabilities(D, perplexity):
    """(P, beta): P the full symmetric matrix of _joint_probabilities (diagonal 0), float64."""
    C, beta = binary_search(D, perplexity)
    P = C + C.T
    P = np.maximum(P / max(P.sum(), EPS), EPS)
    np.fill_diagonal(P, 0.0)
    return P, beta


def joint_probabilities_f32(X, perplexity):
    """The float32 restatement's (P, beta): the device's arithmetic on the CPU -- Gram-form float32 distances, the
    double search on them, P rounded to float32 (returned as float64 values)."""
    P, beta = joint_probabilities(gram_sq_distances_f32(X), perplexity)
    return P.astype(np.float32).astype(np.float64), beta


def p_deviation(P32, P):
    """max |P32 - P| relative to the row maximum of P: the figure the GPU tests' bound on P is built from."""
    return float((np.abs(P32 - P) / P.max(1, keepdims=True)).max())


def kl_and_gradient(P, Y, exaggeration=1.0, dtype=np.float64, sums=True):
    """_kl_divergence (degrees_of_freedom = 1) at Y with p = exaggeration * P.  Returns {'kl', 'grad' [n, 2], 'Z',
    'Sa', 'Sr' [n, 2], 'clamped', 'kl_scale'}: Sa_i = sum_j p_ij w_ij |y_i - y_j| and Sr_i = sum_j w_ij^2 |y_i - y_j|
    per coordinate, 'clamped' whether scikit-learn's Q = max(w / Z, eps) acts anywhere, 'kl_scale' = sum p (|log p| +
    |log w| + |log Z|).  dtype: the arithmetic of w and of the per-row force sums (Z and KL are always float64);
    sums=False leaves out Sa, Sr and kl_scale."""
    n = len(Y)
    off = ~np.eye(n, dtype=bool)
    Y = np.asarray(Y).astype(dtype)
    p = (np.asarray(P, dtype=np.float64) * exaggeration).astype(dtype)
    diff = Y[:, None, :] - Y[None, :, :]
    w = (dtype(1.0) / (dtype(1.0) + (diff * diff).sum(-1))).astype(dtype)
    w[~off] = 0
    Z = float(w.astype(np.float64).sum())
    q = w.astype(np.float64) / Z
    clamped = bool((q[off] < EPS).any())
    pd, wd = p.astype(np.float64), w.astype(np.float64)
    logp = np.log(np.maximum(pd[off], EPS))
    logw = np.log(wd[off])
    kl = float((pd[off] * (logp - logw)).sum() + np.log(Z) * pd[off].sum())
    att = ((p * w)[:, :, None] * diff).sum(1, dtype=dtype)
    rep = ((w * w)[:, :, None] * diff).sum(1, dtype=dtype)
    grad = 4.0 * (att.astype(np.float64) - rep.astype(np.float64) / Z)
    if not sums:
        return {"kl": kl, "grad": grad.astype(dtype), "Z": Z, "clamped": clamped}
    kl_scale = float((pd[off] * (np.abs(logp) + np.abs(logw) + abs(np.log(Z)))).sum())
    Sa = ((pd * wd)[:, :, None] * np.abs(diff.astype(np.float64))).sum(1)
    Sr = ((wd * wd)[:, :, None] * np.abs(diff.astype(np.float64))).sum(1)
    return {"kl": kl, "grad": grad.astype(dtype), "Z": Z, "Sa": Sa, "Sr": Sr, "clamped": clamped, "kl_scale": kl_scale}


def auto_learning_rate(n, early_exaggeration=12.0):
    return max(n / early_exaggeration / 4.0, 50.0)


def predict_n_iter(history, max_iter, n_iter_without_progress=300, min_grad_norm=1e-7):
    """scikit-learn's stop rules applied to a run's own check records [(error, grad_norm)]: (n_iter, records used)."""
    k, it, i = 0, 0, 0
    for phase in (0, 1):
        nwp = EXPLORATION if phase == 0 else n_iter_without_progress
        end = min(EXPLORATION, max_iter) if phase == 0 else max_iter
        best, best_iter = np.finfo(np.float64).max, it
        i = it
        for i in range(it, end):
            if (i + 1) % N_ITER_CHECK:
                continue
            err, gn = history[k]
            k += 1
            stop = False
            if err < best:
                best, best_iter = err, i
            elif i - best_iter > nwp:
                stop = True
            if gn <= min_grad_norm:
                stop = True
            if stop:
                break
        if phase == 0 and i + 1 < max_iter:
            it = i + 1
            continue
        break
    return i, k


def descend(P, Y0, max_iter=1000, early_exaggeration=12.0, learning_rate=None, min_grad_norm=1e-7,
            n_iter_without_progress=300, dtype=np.float64, snapshots=(), momentum0=0.5, exaggerate=True,
            swap_gains=False):
    """TSNE._tsne: min(250, max_iter) exploration iterations (momentum 0.5, early_exaggeration * P), then momentum
    0.8 on P up to max_iter.  Returns {'Y', 'n_iter', 'kl_divergence', 'history' [(error, grad_norm)], 'checks'
    [iteration of each record], 'snapshots' {k: Y after k iterations}}.  momentum0 / exaggerate / swap_gains are the
    mutants of tests/test_tsne_ref_cpu.py."""
    n = len(Y0)
    lr = dtype(auto_learning_rate(n, early_exaggeration) if learning_rate is None else learning_rate)
    Y = np.array(Y0, dtype=dtype)
    history, checks, snaps = [], [], {}
    if 0 in snapshots:
        snaps[0] = Y.copy()
    explore_n = min(EXPLORATION, max_iter)
    it, error, done = 0, np.finfo(np.float64).max, False
    for phase in (0, 1):
        ex = early_exaggeration if (phase == 0 and exaggerate) else 1.0
        mom = dtype(momentum0 if phase == 0 else 0.8)
        nwp = EXPLORATION if phase == 0 else n_iter_without_progress
        end = explore_n if phase == 0 else max_iter
        update, gains = np.zeros_like(Y), np.ones_like(Y)
        best, best_iter = np.finfo(np.float64).max, it
        i = it
        for i in range(it, end):
            check = (i + 1) % N_ITER_CHECK == 0
            r = kl_and_gradient(P, Y, ex, dtype, sums=False)
            if check or i == end - 1:
                error = r["kl"]
            grad = r["grad"].astype(dtype)
            inc = update * grad < 0
            if swap_gains:
                inc = ~inc
            gains = np.where(inc, gains + dtype(0.2), gains * dtype(0.8)).astype(dtype)
            gains = np.maximum(gains, dtype(0.01))
            grad = grad * gains
            update = (mom * update - lr * grad).astype(dtype)
            Y = (Y + update).astype(dtype)
            if i + 1 in snapshots:
                snaps[i + 1] = Y.copy()
            if check:
                gn = float(np.sqrt((grad.astype(np.float64) ** 2).sum()))
                history.append((error, gn))
                checks.append(i)
                stop = False
                if error < best:
                    best, best_iter = error, i
                elif i - best_iter > nwp:
                    stop = True
                if gn <= min_grad_norm:
                    stop = True
                if stop:
                    break
        if phase == 0 and i + 1 < max_iter:
            it = i + 1
            continue
        break
    return {"Y": Y, "n_iter": i, "kl_divergence": error, "history": history, "checks": checks, "snapshots": snaps}


def pca_init(X):
    """TSNE's init='pca' with the exact components: the top two principal components of the centred rows (float64),
    each signed so that its largest-magnitude loading is positive (svd_flip(u_based_decision=False)), cast to float32
    and scaled so that column 0 has standard deviation 1e-4."""
    X = np.asarray(X, dtype=np.float64)
    Xc = X - X.mean(0)
    _, V = np.linalg.eigh(Xc.T @ Xc)
    V = V[:, ::-1][:, :2]
    V = V * np.sign(V[np.abs(V).argmax(0), range(2)])
    Y = (Xc @ V).astype(np.float32)
    return Y / np.std(Y[:, 0]) * np.float32(1e-4)
