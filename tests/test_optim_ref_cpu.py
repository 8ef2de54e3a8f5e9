"""The optimizer reference validates itself without a GPU (tests/optim_ref.py): the float32 restatement
of the kernel's arithmetic stays inside the error bounds against the float64 reference on the very
vectors the GPU cases use, every named mutation of it leaves them, and the shadow's fragment index is
the bijection the kernels assume."""
import numpy as np
import pytest

import optim_ref as R


def _run(name, mutation=None):
    inp, kw = R.make_case(name)
    return R.f32_restatement(inp["G"], inp["p"], inp["m"], inp["v"], inp["teacher"], mutation=mutation, **kw)


@pytest.mark.parametrize("name", sorted(R.CASES))
def test_f32_restatement_is_inside_the_bounds(name):
    ref, bnd = R.case_reference(name)
    got = _run(name)
    assert got["m"].size == R.NPARAM == 197892
    w = R.worst(got, ref, bnd)
    print(name, "worst multiple of the bound:", w, "in u:", R.worst_u(got, ref))
    for k, (bad, ratio) in w.items():
        assert bad == 0, (name, k, bad, ratio)
    assert abs(got["norm"] - ref["norm"]) <= bnd["norm_rel"] * ref["norm"]
    if name in ("clip_inactive", "fresh"):
        assert got["coef"] == 1.0 and not ref["clip_active"]
    else:
        assert ref["clip_active"] and abs(got["coef"] - ref["coef"]) <= R.K_COEF * R.U * ref["coef"]
    if name == "warmup":
        inp, _ = R.make_case(name)
        np.testing.assert_array_equal(got["teacher"], inp["teacher"])


def test_the_cases_are_what_they_claim():
    for name, (norm, t, warmup, fresh) in R.CASES.items():
        inp, kw = R.make_case(name)
        assert abs(np.linalg.norm(inp["G"].astype(np.float64)) - norm) < 1e-6 * norm
        rows = inp["G"][:R.NW1].reshape(R.H, R.D)
        dead = (rows == 0).all(axis=1)
        assert 10 < dead.sum() < 50 and (rows[~dead] != 0).all()
        assert fresh == (not inp["m"].any() and not inp["v"].any())
        assert kw["t"] == t and kw["warmup"] == warmup
    ref, _ = R.case_reference("fresh")
    # a zero-gradient row of a fresh optimizer moves by about lr sign(p), driven by weight decay alone:
    # lr g / (|g| + eps) with g = wd p, i.e. within eps / (wd |p|) <= 5 % of lr where |p| >= 0.02
    inp, kw = R.make_case("fresh")
    z = np.flatnonzero((inp["G"][:R.NW1] == 0) & (np.abs(inp["p"][:R.NW1]) >= 0.02))
    assert z.size > 1000
    move = (ref["p"] - ref["p0"])[z]
    np.testing.assert_allclose(move, -kw["lr"] * np.sign(inp["p"][z]), rtol=0.06)


@pytest.mark.parametrize("mutation", R.MUTATIONS)
def test_every_mutation_leaves_the_bounds(mutation):
    failed = {}
    for name in sorted(R.CASES):
        ref, bnd = R.case_reference(name)
        w = R.worst(_run(name, mutation), ref, bnd)
        bad = {k: n for k, (n, _) in w.items() if n}
        if bad:
            failed[name] = bad
    print(mutation, failed)
    assert failed, "no case tells %s from the kernel's arithmetic" % mutation
    # the mutations that act on every step are seen by every case that can see them
    if mutation in ("t_minus_1", "t_plus_1", "bc2_no_sqrt"):
        assert set(failed) >= set(R.CASES) - {"late"}       # (t = 20000: the corrections round to 1)
    if mutation in ("no_weight_decay", "eps_in_sqrt"):
        assert set(failed) == set(R.CASES)
    if mutation == "ema_pre_update":
        assert set(failed) == set(R.CASES) - {"warmup"}
    if mutation == "no_coef":
        assert set(failed) == {n for n, c in R.CASES.items() if c[0] > 1.0}
    if mutation == "ema_in_warmup":
        assert set(failed) == {"warmup"}


def test_frag_index_is_a_bijection_and_inverts_the_walk():
    h, k = np.meshgrid(np.arange(R.H), np.arange(R.D), indexing="ij")
    f = R.frag_index(h, k).reshape(-1)
    assert f.min() == 0 and f.max() == R.NW1 - 1
    assert np.array_equal(np.sort(f), np.arange(R.NW1))
    # w1_param_of_frag: the parameter of shadow slot f
    assert np.array_equal(R.param_of_frag(f), (h * R.D + k).reshape(-1))
    assert np.array_equal(R.frag_index(*np.divmod(R.param_of_frag(np.arange(R.NW1)), R.D)), np.arange(R.NW1))
    # 4 consecutive k of one h are 4 consecutive slots (the vector path's 8-byte shadow stores), and a
    # block's 1024 consecutive slots are 16 h x 64 k
    assert np.array_equal(f.reshape(-1, 4)[:, 1:] - f.reshape(-1, 4)[:, :1], np.tile([1, 2, 3], (R.NW1 // 4, 1)))
    blk = R.param_of_frag(np.arange(1024) + 5 * 1024)
    assert len(set(blk // R.D)) == 16 and len(set(blk % R.D)) == 64
    # spot values from the formula by hand: (h, k) = (0, 8) is lane 16, (16, 0) the next t
    assert int(R.frag_index(0, 8)) == 16 * 8 and int(R.frag_index(16, 0)) == 24 * 64 * 8
    assert int(R.frag_index(255, 767)) == R.NW1 - 1
