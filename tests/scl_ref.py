"""The supervised-contrastive loss of include/dad.h (dad_scl), restated twice on the CPU.

`scl_autograd`: the definition, written with torch and differentiated by autograd.
`scl_closed_form`: the closed-form gradient the kernels implement (G = H + H^T), in NumPy, sharing nothing with
the first path but the member selection.  Both run in float64 by default; `dtype=float32` runs the same formulas
in single precision, which shows how much room the kernels' fp32 arithmetic has below the GPU tests' bound.

Definition.  A = rows with member != 0, a label in [0, 4) and |e| > 1e-12; z = e / |e|; s = z z^T;
P(i) = {p in A, p != i, y_p = y_i};  l_i = -(1 / |P(i)|) sum_{p in P(i)} [s_ip / tau - log sum_{a != i} exp(s_ia / tau)];
L = mean of l_i over the V anchors with |P(i)| >= 1, 0 when V = 0.  Rows outside A get a zero gradient and their
values are never read."""
import numpy as np
import torch

C = 4


def members(emb, labels, member):
    """Indices of A.  A flagged, labelled row's norm is taken in float64; a non-finite one is not > 1e-12."""
    labels = np.asarray(labels)
    flag = (np.asarray(member) != 0) & (labels >= 0) & (labels < C)
    idx = []
    for i in np.flatnonzero(flag):
        with np.errstate(all="ignore"):
            nrm = np.sqrt(np.sum(np.asarray(emb[i], np.float64) ** 2))
        if nrm > 1e-12:
            idx.append(i)
    return np.asarray(idx, np.int64)


def stats(emb, labels, member):
    """out block of dad_scl without the loss: V, |A|, anchors per class, flagged rows with a non-finite value."""
    labels = np.asarray(labels)
    idx = members(emb, labels, member)
    nc = np.bincount(labels[idx], minlength=C)[:C] if idx.size else np.zeros(C, np.int64)
    anchors = np.where(nc >= 2, nc, 0)
    flag = (np.asarray(member) != 0) & (labels >= 0) & (labels < C)
    bad = int(sum(not np.all(np.isfinite(emb[i])) for i in np.flatnonzero(flag)))
    return {"V": int(anchors.sum()), "members": int(idx.size), "anchors": anchors, "nonfinite": bad}


def scl_torch(e, y, tau):
    """The definition on member rows e (a torch tensor, every row in A) with classes y: the loss as a tensor that
    autograd can differentiate, or None when no row is an anchor."""
    y = torch.as_tensor(np.asarray(y))
    z = e / e.norm(dim=1, keepdim=True)
    s = (z @ z.T) / tau
    m = e.shape[0]
    eye = torch.eye(m, dtype=torch.bool)
    lse = torch.logsumexp(s.masked_fill(eye, -float("inf")), dim=1) if m > 1 else torch.zeros(m, dtype=e.dtype)
    pos = (y[:, None] == y[None, :]) & ~eye
    npos = pos.sum(1)
    anchor = npos >= 1
    if not bool(anchor.any()):
        return None
    li = -((s - lse[:, None]) * pos).sum(1)[anchor] / npos[anchor]
    return li.mean()


def scl_autograd(emb, labels, member, tau, dtype=torch.float64):
    """(loss, grad [n][256]) by autograd of the definition."""
    emb = np.asarray(emb)
    labels = np.asarray(labels)
    idx = members(emb, labels, member)
    grad = np.zeros(emb.shape, np.float64)
    if idx.size == 0:
        return 0.0, grad
    e = torch.tensor(emb[idx], dtype=dtype, requires_grad=True)
    loss = scl_torch(e, labels[idx], tau)
    if loss is None:
        return 0.0, grad
    loss.backward()
    grad[idx] = e.grad.double().numpy()
    return float(loss.detach()), grad


def scl_closed_form(emb, labels, member, tau, dtype=np.float64):
    """(loss, grad [n][256]) by the closed form; every array in `dtype`."""
    emb = np.asarray(emb)
    labels = np.asarray(labels)
    idx = members(emb, labels, member)
    grad = np.zeros(emb.shape, np.float64)
    m = idx.size
    if m == 0:
        return 0.0, grad
    f = dtype
    e = emb[idx].astype(f)
    y = labels[idx]
    nrm = np.sqrt(np.sum(e * e, axis=1, dtype=f)).astype(f)
    z = (e / nrm[:, None]).astype(f)
    u = ((z @ z.T).astype(f) / f(tau)).astype(f)
    off = ~np.eye(m, dtype=bool)
    pos = (y[:, None] == y[None, :]) & off
    npos = pos.sum(1)
    v = (npos >= 1).astype(f)
    V = int(v.sum())
    if V == 0:
        return 0.0, grad
    um = np.where(off, u, -np.inf)
    mx = um.max(axis=1) if m > 1 else np.zeros(m, f)
    ex = np.where(off, np.exp((u - mx[:, None]).astype(f)), f(0)).astype(f)
    lse = (mx + np.log(ex.sum(axis=1, dtype=f))).astype(f)
    c = np.where(npos >= 1, v / np.maximum(npos, 1), 0).astype(f)
    li = lse - np.where(pos, u, f(0)).sum(axis=1, dtype=f) * c
    loss = float(np.sum(np.where(npos >= 1, li, 0), dtype=np.float64) / V)
    p = np.where(off, np.exp((u - lse[:, None]).astype(f)), f(0)).astype(f)
    H = ((v[:, None] * p - c[:, None] * pos) / f(V * tau)).astype(f)
    G = (H + H.T).astype(f)
    gz = (G @ z).astype(f)
    ge = ((gz - z * np.sum(z * gz, axis=1, dtype=f)[:, None]) / nrm[:, None]).astype(f)
    grad[idx] = ge.astype(np.float64)
    return loss, grad


def relu_like_rows(n, seed, classes=C):
    """Embeddings of the shape ReLU pooling gives: non-negative, with a common offset (rows nearly parallel), and
    a class-dependent part smaller than the rows' own spread: the classes overlap, as a training batch's do, so the
    gradient is of the size of its terms (on well-separated classes it is their small difference, and float32
    loses digits of it on any device).  Returns (emb [n][256] float32, labels [n] int64)."""
    rs = np.random.RandomState(seed)
    proto = rs.normal(0.0, 0.12, size=(classes, 256))
    y = rs.randint(0, classes, size=n).astype(np.int64)
    e = np.maximum(0.6 + proto[y] + rs.normal(0.0, 0.25, size=(n, 256)), 0.0)
    return e.astype(np.float32), y


GPU_NS = (2, 7, 63, 64, 65, 128, 130)      # below, at and above one tile and two tiles
GPU_TAUS = (0.07, 0.1, 0.5)
GPU_KINDS = ("plain", "singleton", "no_positives", "nan_nonmembers", "zero_member", "identical")


def gpu_case(n, kind="plain"):
    """The inputs of the GPU tests (tests/test_gpu_scl.py), also run here in float32 on the CPU: (emb, labels,
    member uint8).  `plain`: random classes, about one row in eight left out by its flag or its label."""
    emb, y = relu_like_rows(n, 1000 + n)
    rs = np.random.RandomState(77 + n)
    member = np.ones(n, np.uint8)
    if kind == "plain":
        if n <= 4:
            y[:] = y[0]                  # (so the smallest case has anchors)
        else:
            member[rs.rand(n) < 0.08] = 0
            y[rs.rand(n) < 0.05] = -1
    elif kind == "singleton":            # class 3 has one member: no anchor, but in every denominator
        y[:] = np.arange(n) % 3
        y[n // 2] = 3
    elif kind == "no_positives":         # four members of four classes: V = 0
        y[:] = -1
        y[:min(4, n)] = np.arange(min(4, n))
        member[4:] = rs.randint(0, 2, size=max(n - 4, 0))
    elif kind == "nan_nonmembers":       # left out by the flag, by the label, by both
        k = max(1, n // 6)
        out = rs.choice(n, size=min(3 * k, n - 2), replace=False)
        emb[out] = np.nan
        emb[out[0], 5] = np.inf
        member[out[:k]] = 0
        y[out[k:2 * k]] = -1
        y[out[2 * k:]] = 4
    elif kind == "zero_member":          # flagged and labelled, but without a direction
        emb[n // 3] = 0.0
        emb[n - 1] = 1e-20
    elif kind == "identical":            # duplicates within a class and across classes
        emb[n - 1] = emb[0]
        y[n - 1] = y[0]
        if n > 3:
            emb[2] = emb[1]
            y[2] = (y[1] + 1) % C
    else:
        raise ValueError(kind)
    return emb, y, member


def rel(a, b):
    """The project's measure (gpu_harness.close): max |a - b| over max |b|, floored at 1e-6."""
    a = np.asarray(a, np.float64)
    b = np.asarray(b, np.float64)
    return float(np.max(np.abs(a - b)) / max(1e-6, float(np.max(np.abs(b)))))
