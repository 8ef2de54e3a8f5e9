"""tests/scl_ref.py against itself: the definition under autograd and the closed form the kernels implement agree,
a finite difference confirms both, the edge rules of include/dad.h hold, and the float32 run of the closed form on the
GPU tests' inputs leaves the 1e-4 bound of tests/test_gpu_scl.py two orders of magnitude of room."""
import numpy as np
import pytest

import scl_ref as R


def _maxabs(g):
    return max(1e-300, float(np.max(np.abs(g))))


@pytest.mark.parametrize("n,tau", [(5, 0.1), (40, 0.07), (100, 0.1), (65, 0.5)])
def test_autograd_and_closed_form_agree(n, tau):
    emb, y, mem = R.gpu_case(n, "plain")
    la, ga = R.scl_autograd(emb, y, mem, tau)
    lc, gc = R.scl_closed_form(emb, y, mem, tau)
    assert abs(la - lc) <= 1e-12 * max(1.0, abs(la))
    assert np.max(np.abs(ga - gc)) <= 1e-12 * _maxabs(ga)
    assert la > 0 and np.any(ga != 0)


def test_central_finite_difference():
    emb, y, mem = R.gpu_case(7, "singleton")
    emb = emb.astype(np.float64)
    tau = 0.1
    _, g = R.scl_closed_form(emb, y, mem, tau)
    rs = np.random.RandomState(0)
    h = 1e-6
    for _ in range(24):
        i, k = rs.randint(0, 7), rs.randint(0, 256)
        ep, em = emb.copy(), emb.copy()
        ep[i, k] += h
        em[i, k] -= h
        fd = (R.scl_autograd(ep, y, mem, tau)[0] - R.scl_autograd(em, y, mem, tau)[0]) / (2 * h)
        assert abs(fd - g[i, k]) <= 1e-6 * _maxabs(g), (i, k, fd, g[i, k])


def test_no_anchor_gives_zero_loss_and_gradient():
    emb, y, mem = R.gpu_case(7, "no_positives")
    for fn in (R.scl_autograd, R.scl_closed_form):
        loss, g = fn(emb, y, mem, 0.1)
        assert loss == 0.0 and not np.any(g)
    assert R.stats(emb, y, mem)["V"] == 0 and R.stats(emb, y, mem)["members"] == 4
    # one member, and none
    one = np.zeros(7, np.uint8)
    one[2] = 1
    assert R.scl_closed_form(emb, np.zeros(7, np.int64), one, 0.1)[0] == 0.0
    assert R.scl_autograd(emb, np.zeros(7, np.int64), np.zeros(7, np.uint8), 0.1)[0] == 0.0


def test_singleton_class_is_no_anchor_but_a_negative():
    emb, y, mem = R.gpu_case(7, "singleton")
    st = R.stats(emb, y, mem)
    assert st["anchors"][3] == 0 and st["V"] == 6 and st["members"] == 7
    loss, g = R.scl_closed_form(emb, y, mem, 0.1)
    single = int(np.flatnonzero(y == 3)[0])
    without = mem.copy()
    without[single] = 0
    loss2, _ = R.scl_closed_form(emb, y, without, 0.1)
    assert loss > loss2              # it sits in the other rows' denominators
    assert np.any(g[single] != 0)    # and is pushed away from them
    # by hand: l_i over the six anchors, every log-sum-exp over the six other members
    z = emb.astype(np.float64)
    z /= np.linalg.norm(z, axis=1, keepdims=True)
    u = z @ z.T / 0.1
    tot = 0.0
    for i in range(7):
        if i == single:
            continue
        lse = np.log(sum(np.exp(u[i, a]) for a in range(7) if a != i))
        ps = [p for p in range(7) if p != i and y[p] == y[i]]
        tot += -sum(u[i, p] - lse for p in ps) / len(ps)
    assert abs(tot / 6 - loss) <= 1e-12 * loss


@pytest.mark.parametrize("kind", ["nan_nonmembers", "zero_member"])
def test_rows_outside_the_member_set_change_nothing(kind):
    emb, y, mem = R.gpu_case(65, kind)
    idx = R.members(emb, y, mem)
    assert 2 < idx.size < 65
    loss, g = R.scl_closed_form(emb, y, mem, 0.1)
    la, ga = R.scl_autograd(emb, y, mem, 0.1)
    lo, go = R.scl_closed_form(emb[idx], y[idx], np.ones(idx.size, np.uint8), 0.1)
    assert np.isfinite(loss) and loss == lo and abs(la - loss) <= 1e-12 * loss
    assert np.array_equal(g[idx], go)
    rest = np.setdiff1d(np.arange(65), idx)
    assert not np.any(g[rest]) and not np.any(ga[rest]) and np.all(np.isfinite(g))
    assert np.max(np.abs(g)) < 1e3      # no 1 / clamp(|e|) from the zero row
    if kind == "nan_nonmembers":
        # only flagged rows with a label in range are counted as non-finite
        assert R.stats(emb, y, mem)["nonfinite"] == 0


def test_identical_rows():
    emb, y, mem = R.gpu_case(64, "identical")
    _, g = R.scl_closed_form(emb, y, mem, 0.1)
    assert np.allclose(g[63], g[0], rtol=0, atol=1e-12 * _maxabs(g))      # same row, same class: same gradient
    assert np.all(np.isfinite(g))


@pytest.mark.parametrize("n", [7, 65, 130])
@pytest.mark.parametrize("tau", R.GPU_TAUS)
def test_float32_formulas_leave_the_gpu_bound_room(n, tau):
    """The GPU tests' bound is 1e-4 (max-abs over max |ref|); the same formulas in float32 on the CPU stay below 1e-5."""
    worst = [0.0, 0.0]
    for kind in R.GPU_KINDS:
        emb, y, mem = R.gpu_case(n, kind)
        l64, g64 = R.scl_closed_form(emb, y, mem, tau)
        l32, g32 = R.scl_closed_form(emb, y, mem, tau, dtype=np.float32)
        if R.stats(emb, y, mem)["V"] == 0:
            assert l32 == 0.0 and not np.any(g32)
            continue
        worst = [max(worst[0], R.rel(l32, l64)), max(worst[1], R.rel(g32, g64))]
    print("float32 n=%d tau=%g: loss %.3g grad %.3g" % (n, tau, worst[0], worst[1]))
    assert worst[0] < 1e-5 and worst[1] < 1e-5
