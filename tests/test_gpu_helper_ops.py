"""The stand-alone helper operators of csrc/utils_abi.hip against oracle/dad_oracle.py at the shapes the golden replays
of test_gpu_utils.py never reach, through the ctypes entry points and through the utils.py classes.  The cases, the
references and every tolerance come from tests/operators_ref.py; tests/test_operators_ref_cpu.py checks, without a
GPU, that the cases reach the branches named here and that the tolerances reject wrong answers.

  dad_augment           odd element counts (the pair's `e >= n` break), D != 768, 2-D input, T = 1, mask_len == T and
                        0, feat_p == 0, the weak path ignoring feat_p / mask_len, B == 0, counter draws added to a
                        nonzero x at D = 7, start_hi
  dad_certainty_scores  B on both sides of one 256-thread block, p = 0 entries, uniform rows, exact ties, null outputs
  dad_dacp_mask         Bn = 1 ... 1024 (second trip of the TAIL_THREADS loops), one class of 513 and of 1024 rows (a
                        class sort of more than 512 scores), an empty class, a single-member class, accumulation over
                        two calls, the epoch update on the device log, Bn = 1025
  dad_ecda_loss         B != Bn, B = Bn = 1, both sides of ECDA_PRE = 64 rows and ECDA_NZ = 80 members, B = Bn = 520,
                        the global MMD, no valid class, one valid class, a clean class of one row, ones(Bn) weights
                        (classes >= Bn skipped), n_weights == Bn == 4, the float-mask re-cast, NaN workspace, null grads
Each test prints the worst measured error relative to its tolerance."""
import numpy as np
import pytest
import torch

import dadpkg
import gpu_harness as gh
import operators_ref as R
from oracle import dad_oracle

pytestmark = pytest.mark.gpu
PKG = dadpkg.pkg()
L = PKG._lib


def _view(**over):
    return PKG.ConfigView(R.cfg(**over), flavor="iemocap")


def _cuda(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return t.to("cuda", dtype) if dtype is not None else t.cuda()


def _p(t):
    return None if t is None else t.data_ptr()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int32) if a.dtype == np.float32 else a


# ------------------------------------------------------------------------------------------- dad_augment
def _augment(x, strong, sd, feat_p, mask_len, noise=None, u=None, start=None, seed=0, counter=0, B=None, fill=None):
    """dad_augment on x [B, T, D] (numpy) -> (rc, out numpy).  fill: the value the output holds before the call."""
    Bx, T, Dd = x.shape
    xd = _cuda(x)
    out = torch.full_like(xd, fill) if fill is not None else torch.empty_like(xd)
    keep = [None if a is None else _cuda(a, dt) for a, dt in ((noise, torch.float32), (u, torch.float32),
                                                              (start, torch.int64))]
    rc = L.lib().dad_augment(xd.data_ptr(), Bx if B is None else B, T, Dd, int(strong), np.float32(sd),
                             np.float32(feat_p), int(mask_len), seed, counter, _p(keep[0]), _p(keep[1]), _p(keep[2]),
                             out.data_ptr(), _stream())
    torch.cuda.synchronize()
    return rc, out.cpu().numpy()


@pytest.mark.parametrize("shape", R.AUG_SHAPES, ids=str)
def test_augment_injected_draws_match_the_oracle_bit_for_bit(shape):
    x, nw, ns, u, start = R.augment_case(shape)
    c = R.cfg()
    aug = PKG.DataAugmentation(cfg=_view())
    two_d = shape == R.AUG_2D
    give = (lambda a: a[0]) if two_d else (lambda a: a)
    w = aug.weak_augment(_cuda(give(x)), noise=give(nw))
    st = aug.strong_augment(_cuda(give(x)), noise=give(ns), u=u, start=start)
    assert w.shape == give(x).shape and st.shape == give(x).shape
    np.testing.assert_array_equal(_bits(w.cpu().numpy().reshape(shape)),
                                  _bits(dad_oracle.weak_augment(x, nw, c["WEAK_NOISE_STD"])))
    want = dad_oracle.strong_augment(x, ns, u, start, c["STRONG_NOISE_STD"], c["DROPOUT_RATE"], c["TEMPORAL_MASK_RATIO"])
    np.testing.assert_array_equal(_bits(st.cpu().numpy().reshape(shape)), _bits(want))


def test_augment_edge_arguments():
    shape = (3, 5, 7)                                           # 105 elements: the last pair holds one
    x, nw, ns, u, start = R.augment_case(shape)
    sd, p = 0.05, 0.3
    assert 0 < (u > np.float32(p)).sum() < 7
    # mask_len == T: every frame zero, with the start given and with the counter start (start_hi = 1)
    for st in (np.zeros(3, np.int64), None):
        rc, out = _augment(x, 1, sd, p, 5, noise=ns, u=u, start=st)
        assert rc == 0 and not out.any()
    # mask_len == 0 on the strong path: noise and feature mask only
    rc, out = _augment(x, 1, sd, p, 0, noise=ns, u=u, start=start)
    assert rc == 0
    np.testing.assert_array_equal(_bits(out), _bits(dad_oracle.strong_augment(x, ns, u, start, sd, p, 0.0)))
    # feat_p == 0: noise and temporal mask only (two frames from start[b])
    st2 = np.array([0, 3, 1], np.int64)
    rc, out = _augment(x, 1, sd, 0.0, 2, noise=ns, u=u, start=st2)
    assert rc == 0
    np.testing.assert_array_equal(_bits(out), _bits(dad_oracle.strong_augment(x, ns, u, st2, sd, 0.0, 0.4)))
    # strong == 0: feat_p and mask_len are ignored
    rc, out = _augment(x, 0, sd, p, 2, noise=ns, u=u, start=st2)
    assert rc == 0
    np.testing.assert_array_equal(_bits(out), _bits(dad_oracle.weak_augment(x, ns, sd)))
    # B == 0: DAD_OK and the output untouched
    rc, out = _augment(x, 1, sd, p, 2, noise=ns, u=u, start=st2, B=0, fill=7.0)
    assert rc == 0 and np.all(out == 7.0)
    # mask_len > T is an argument error
    assert _augment(x, 1, sd, p, 6, noise=ns, u=u, start=st2)[0] == L.E_ARG


def _draws(which, cfg, n):
    out = torch.empty(n, device="cuda")
    L.check(L.lib().dad_rng_draws(cfg, which, 0, n, out.data_ptr(), _stream()), "dad_rng_draws")
    torch.cuda.synchronize()
    return out.cpu().numpy()


def test_augment_counter_draws_at_D7_are_the_step_streams():
    B, T, Dd, seed, counter = 3, 40, 7, 1234, 5
    n = B * T * Dd
    view = _view()
    cfg = PKG.config.dad_config_for(view, 1, 1, B, T, 60, 1, seed=seed, counter=counter)
    assert cfg.Bn * cfg.Tn * 768 >= n and cfg.mask_len == 4 and cfg.start_hi == T - 4 + 1
    # small integers: x + noise is one fp32 addition of the drawn value, and x never cancels it to 0
    x = np.random.RandomState(3).randint(1, 9, size=(B, T, Dd)).astype(np.float32)
    rc, weak = _augment(x, 0, cfg.weak_std, 0.0, 0, seed=seed, counter=counter)
    assert rc == 0
    nw = _draws(L.DRAW_WEAK, cfg, n).reshape(B, T, Dd)
    np.testing.assert_array_equal(_bits(weak), _bits(x + nw))
    rc, strong = _augment(x, 1, cfg.strong_std, cfg.feat_p, cfg.mask_len, seed=seed, counter=counter)
    assert rc == 0
    ns = _draws(L.DRAW_STRONG, cfg, n).reshape(B, T, Dd)
    keep = _draws(L.DRAW_FEAT_KEEP, cfg, Dd)
    start = _draws(L.DRAW_TSTART, cfg, B).astype(np.int64)
    assert set(np.unique(keep)) <= {0.0, 1.0} and np.all(start >= 0) and np.all(start + cfg.mask_len <= T)
    want = (x + ns) * keep[None, None, :]                       # 0 or x + noise: exact
    for b in range(B):
        want[b, start[b]:start[b] + cfg.mask_len] = 0
    np.testing.assert_array_equal(_bits(strong), _bits(want))
    assert np.abs(nw).max() > 0 and np.abs(weak - x).max() > 0 and not np.array_equal(nw, ns)
    # x = 0: the output is the draw itself
    rc, weak0 = _augment(np.zeros_like(x), 0, cfg.weak_std, 0.0, 0, seed=seed, counter=counter)
    assert rc == 0
    np.testing.assert_array_equal(_bits(weak0), _bits(nw))


def test_augment_counter_starts_respect_start_hi():
    """Every drawn start leaves the whole mask inside the utterance: start + mask_len <= T (start_hi = T - mask_len + 1).
    x = 1 with no noise and no feature mask: the zero frames of the output ARE the mask."""
    B, T, Dd, mlen = 64, 5, 3, 4
    x = np.ones((B, T, Dd), np.float32)
    seen = set()
    for counter in range(3):
        rc, out = _augment(x, 1, 0.0, 0.0, mlen, seed=9, counter=counter)
        assert rc == 0 and set(np.unique(out)) <= {0.0, 1.0}
        zero = out == 0
        assert np.all(zero == zero[:, :, :1])                   # a frame is masked as a whole
        for b in range(B):
            t = np.nonzero(zero[b, :, 0])[0]
            assert len(t) == mlen and t[-1] - t[0] == mlen - 1 and t[-1] < T
            seen.add(int(t[0]))
    assert seen == {0, 1}, seen


# ---------------------------------------------------------------------------------- dad_certainty_scores
def _certainty(p, use_entropy, want_score=True, want_pred=True):
    B = p.shape[0]
    q = _cuda(p)
    s = torch.full((B,), -7.0, device="cuda") if want_score else None
    pr = torch.full((B,), -7, dtype=torch.int64, device="cuda") if want_pred else None
    rc = L.lib().dad_certainty_scores(q.data_ptr(), B, int(use_entropy), _p(s), _p(pr), _stream())
    torch.cuda.synchronize()
    assert rc == 0
    return (None if s is None else s.cpu().numpy()), (None if pr is None else pr.cpu().numpy())


@pytest.mark.parametrize("use_entropy", [True, False])
@pytest.mark.parametrize("B", R.CERT_B)
def test_certainty_scores_match_the_oracle(B, use_entropy):
    if B == 1:
        # the special rows, each a launch of one row; compared together (the tolerance is relative to the largest
        # score of a batch, and a uniform row's own score is 0)
        alone = [_certainty(r[None], use_entropy) for r in R.SPECIAL_ROWS]
        want_s, want_p = dad_oracle.certainty_scores(R.SPECIAL_ROWS, use_entropy)
        np.testing.assert_array_equal(np.concatenate([a[1] for a in alone]), want_p)
        gh.close(np.concatenate([a[0] for a in alone]), want_s, R.CERT_TOL, "special rows alone")
    p = R.certainty_case(B)
    want_s, want_p = dad_oracle.certainty_scores(p, use_entropy)
    s, pred = _certainty(p, use_entropy)
    np.testing.assert_array_equal(pred, want_p)
    gh.close(s, want_s, R.CERT_TOL, "certainty B=%d" % B)
    # a null output leaves the other one as it was
    s2, none = _certainty(p, use_entropy, want_pred=False)
    none2, p2 = _certainty(p, use_entropy, want_score=False)
    assert none is None and none2 is None
    np.testing.assert_array_equal(_bits(s2), _bits(s))
    np.testing.assert_array_equal(p2, pred)
    # the class method (config switch) gives the same bits
    s3, p3 = PKG.DACPManager.calculate_certainty_scores(_cuda(p), cfg=_view(USE_ENTROPY_IN_SCORE=use_entropy))
    np.testing.assert_array_equal(_bits(s3.cpu().numpy()), _bits(s))
    np.testing.assert_array_equal(p3.cpu().numpy(), pred)
    print("certainty B=%d entropy=%s: worst err / tol %.3g" % (B, use_entropy, gh.rel(s, want_s) / R.CERT_TOL))


# ----------------------------------------------------------------------------------------- dad_dacp_mask
def _manager():
    c = R.cfg()
    return PKG.DACPManager(4, c["EPOCHS"], "cuda", cfg=_view())


def _check_dacp(what, got, want, worst):
    np.testing.assert_array_equal(got["mask"], want["mask"], err_msg=what + " mask")
    np.testing.assert_array_equal(got["pred"], want["pred"], err_msg=what + " pred")
    np.testing.assert_array_equal(got["counts"], want["counts"].astype(np.float32), err_msg=what + " counts")
    for k in ("score", "w", "tau", "sums"):         # (gh.close is relative to the largest magnitude: the sums' own)
        gh.close(got[k], want[k], 1e-6, "%s %s" % (what, k))
        worst[k] = max(worst.get(k, 0.0), gh.rel(got[k], want[k]) / 1e-6)


@pytest.mark.parametrize("case", R.DACP_CASES, ids=R.dacp_id)
def test_dacp_mask_matches_the_oracle_over_two_calls(case):
    Bn = case[0]
    probs, tau, Q, anchors, epoch = R.dacp_case(case)
    calls, ref_state = R.dacp_reference(case)
    mgr = _manager()
    q = _cuda(probs)
    worst = {}
    # the entry point on a 20-float state of its own
    state = torch.zeros(L.DAD_DACP_FLOATS, device="cuda")
    state[0:4], state[4:8], state[16:20] = _cuda(tau), _cuda(Q), _cuda(anchors)
    cfg = mgr._config(Bn, epoch)
    for i, want in enumerate(calls):
        mask = torch.full((Bn,), 9, dtype=torch.uint8, device="cuda")
        s, pr, w = torch.empty(Bn, device="cuda"), torch.empty(Bn, dtype=torch.int64, device="cuda"), torch.empty(4, device="cuda")
        rc = L.lib().dad_dacp_mask(cfg, q.data_ptr(), Bn, state.data_ptr(), mask.data_ptr(), s.data_ptr(),
                                   pr.data_ptr(), w.data_ptr(), _stream())
        torch.cuda.synchronize()
        assert rc == 0
        st = state.cpu().numpy()
        got = dict(mask=mask.cpu().numpy().astype(bool), score=s.cpu().numpy(), pred=pr.cpu().numpy(), w=w.cpu().numpy(),
                   tau=st[0:4], sums=st[8:12], counts=st[12:16])
        assert set(np.unique(mask.cpu().numpy())) <= {0, 1}
        _check_dacp("%s call %d" % (R.dacp_id(case), i), got, want, worst)
        np.testing.assert_array_equal(st[4:8], Q)
        np.testing.assert_array_equal(st[16:20], anchors)
    # null score / pred / weights: the mask and the state update are the same
    state2 = torch.zeros(L.DAD_DACP_FLOATS, device="cuda")
    state2[0:4], state2[4:8], state2[16:20] = _cuda(tau), _cuda(Q), _cuda(anchors)
    mask2 = torch.empty(Bn, dtype=torch.uint8, device="cuda")
    assert L.lib().dad_dacp_mask(cfg, q.data_ptr(), Bn, state2.data_ptr(), mask2.data_ptr(), None, None, None,
                                 _stream()) == 0
    torch.cuda.synchronize()
    np.testing.assert_array_equal(mask2.cpu().numpy().astype(bool), calls[0]["mask"])
    gh.close(state2[0:4].cpu().numpy(), calls[0]["tau"], 1e-6, "tau (null outputs)")
    # DACPManager: the same two calls, then the epoch update on the device log (a class with count 0 keeps its Q)
    mgr.ema_thresholds, mgr.class_quality_scores = tau, Q
    for i, want in enumerate(calls):
        mask, s, w = mgr.calculate_mask(q, epoch, torch.from_numpy(anchors))
        torch.cuda.synchronize()
        assert mask.dtype == torch.bool
        st = mgr.state.cpu().numpy()
        got = dict(mask=mask.cpu().numpy(), score=s.cpu().numpy(), pred=mgr.batch_scores_per_class.parts[-1][1].cpu().numpy(),
                   w=w.cpu().numpy(), tau=mgr.ema_thresholds.cpu().numpy(), sums=st[8:12], counts=st[12:16])
        _check_dacp("%s manager call %d" % (R.dacp_id(case), i), got, want, worst)
    assert [len(v) for v in mgr.batch_scores_per_class] == list(calls[-1]["counts"])
    beta = R.cfg()["DACP_QUALITY_SMOOTHING_BETA"]
    empty = ref_state.score_cnt == 0
    ref_state.epoch_end(beta)
    mgr.update_class_quality_scores_epoch(mgr.batch_scores_per_class)
    torch.cuda.synchronize()
    gh.close(mgr.class_quality_scores.cpu().numpy(), ref_state.Q, 1e-6, "epoch Q")
    worst["Q"] = gh.rel(mgr.class_quality_scores.cpu().numpy(), ref_state.Q) / 1e-6
    if empty.any():
        gh.close(mgr.class_quality_scores.cpu().numpy()[empty], Q[empty], 1e-6, "Q of an empty class")
    assert not mgr.state[8:16].any() and [len(v) for v in mgr.batch_scores_per_class] == [0, 0, 0, 0]
    print("%s: worst err / 1e-6: %s" % (R.dacp_id(case), {k: float("%.3g" % v) for k, v in worst.items()}))


def test_dacp_mask_refuses_more_than_1024_rows():
    mgr = _manager()
    q = torch.full((1025, 4), 0.25, device="cuda")
    state = torch.full((L.DAD_DACP_FLOATS,), 0.5, device="cuda")
    before = state.clone()
    mask = torch.zeros(1025, dtype=torch.uint8, device="cuda")
    for Bn in (1025, 0):
        assert L.lib().dad_dacp_mask(mgr._config(1024, 60), q.data_ptr(), Bn, state.data_ptr(), mask.data_ptr(), None,
                                     None, None, _stream()) == L.E_SHAPE
    torch.cuda.synchronize()
    assert torch.equal(state, before)


# ----------------------------------------------------------------------------------------- dad_ecda_loss
ECDA_RUNS = [(n, a) for n in R.ECDA_CASES for a in R.ECDA_CASES[n]["aware"]]


def _ecda_id(run):
    return "%s-%s" % (run[0], "class_aware" if run[1] else "global")


def _ecda(k, class_aware, ws_fill=0, grad_clean=True, grad_noisy=True):
    """dad_ecda_loss on a case -> (loss float32, d/d clean, d/d noisy) as numpy (None for a null output).  The
    outputs start as NaN; ws_fill: the byte the workspace is filled with (0xff: every float a NaN)."""
    view = _view(USE_CLASS_AWARE_MMD=class_aware)
    c = PKG.config.dad_config_for(view, 1, 1, 1, 1, view.WARMUP_EPOCHS, 1)
    c.class_aware = int(class_aware)
    B, Bn = k["B"], k["Bn"]
    t = dict(ec=_cuda(k["clean"]), en=_cuda(k["noisy"]), yc=_cuda(k["yc"]), yn=_cuda(k["pred"]),
             m=_cuda(R.ecda_bool_mask(k).astype(np.uint8)), sc=_cuda(k["scores"]), w=_cuda(k["w"]))
    loss = torch.full((), float("nan"), device="cuda")
    gc = torch.full((B, R.H), float("nan"), device="cuda") if grad_clean else None
    gn = torch.full((Bn, R.H), float("nan"), device="cuda") if grad_noisy else None
    nbytes = int(L.lib().dad_ecda_workspace_bytes(B, Bn))
    assert nbytes > 0
    ws = torch.full((nbytes,), ws_fill, dtype=torch.uint8, device="cuda")
    rc = L.lib().dad_ecda_loss(c, t["ec"].data_ptr(), B, t["en"].data_ptr(), Bn, t["yc"].data_ptr(), t["yn"].data_ptr(),
                               t["m"].data_ptr(), t["sc"].data_ptr(), t["w"].data_ptr(), len(k["w"]), loss.data_ptr(),
                               _p(gc), _p(gn), ws.data_ptr(), _stream())
    torch.cuda.synchronize()
    assert rc == 0
    return loss.cpu().numpy(), (None if gc is None else gc.cpu().numpy()), (None if gn is None else gn.cpu().numpy())


def _same_bits(a, b, what):
    for x, y, n in zip(a, b, ("loss", "d/d clean", "d/d noisy")):
        if x is not None and y is not None:
            np.testing.assert_array_equal(_bits(x), _bits(y), err_msg="%s: %s" % (what, n))


def _norm_rel(a, b):
    return float(np.linalg.norm(np.asarray(a, np.float64) - b) / max(1e-12, np.linalg.norm(b)))


@pytest.mark.parametrize("run", ECDA_RUNS, ids=_ecda_id)
def test_ecda_loss_matches_the_oracle(run):
    name, aware = run
    k = R.ecda_case(name)
    want, wc, wn = R.ecda_reference(name, aware)
    got = _ecda(k, aware)
    loss, gc, gn = got
    assert np.isfinite(loss) and np.all(np.isfinite(gc)) and np.all(np.isfinite(gn))
    print("%s: loss %.6f (oracle %.6f) err / tol %.3g; grad norm-rel / 1e-4: clean %.3g noisy %.3g" % (
        _ecda_id(run), loss, want, abs(float(loss) - want) / (R.ECDA_LOSS_TOL * max(1.0, abs(want))),
        _norm_rel(gc, wc) / 1e-4 if wc.any() else 0.0, _norm_rel(gn, wn) / 1e-4 if wn.any() else 0.0))
    assert R.ecda_loss_ok(loss, want), (float(loss), want)
    gh.close_grad(gc, wc, "%s d/d clean" % name)
    gh.close_grad(gn, wn, "%s d/d noisy" % name)
    if want == 0.0:
        assert loss == 0.0
    # rows outside every member set: exactly zero
    assert not gc[~np.any(wc != 0, axis=1)].any() and not gn[~np.any(wn != 0, axis=1)].any()
    # a second call, and one on a workspace of NaNs, give the same bits
    _same_bits(_ecda(k, aware), got, "second call")
    _same_bits(_ecda(k, aware, ws_fill=0xff), got, "NaN workspace")
    # a null gradient pointer leaves the loss and the other gradient unchanged
    only_n = _ecda(k, aware, grad_clean=False)
    only_c = _ecda(k, aware, grad_noisy=False)
    assert only_n[1] is None and only_c[2] is None
    _same_bits(only_n, got, "null grad_clean")
    _same_bits(only_c, got, "null grad_noisy")


@pytest.mark.parametrize("run", ECDA_RUNS, ids=_ecda_id)
def test_ecda_loss_module_delivers_the_same_gradients(run):
    """ECDALoss (autograd) on the case as the trainer passes it: a bool mask, or confidences to re-cast."""
    name, aware = run
    k = R.ecda_case(name)
    want, wc, wn = R.ecda_reference(name, aware)
    crit = PKG.ECDALoss(cfg=_view(USE_CLASS_AWARE_MMD=aware))
    ec, en = _cuda(k["clean"]).requires_grad_(True), _cuda(k["noisy"]).requires_grad_(True)
    loss = crit(ec, en, _cuda(k["yc"]), _cuda(k["pred"]), _cuda(k["mask"]), _cuda(k["scores"]), _cuda(k["w"]))
    loss.backward()
    torch.cuda.synchronize()
    direct = _ecda(k, aware)
    _same_bits((loss.detach().cpu().numpy(), ec.grad.cpu().numpy(), en.grad.cpu().numpy()), direct, name)
    assert R.ecda_loss_ok(float(loss.detach()), want)
    gh.close_grad(ec.grad.cpu().numpy(), wc, "%s d/d clean (module)" % name)
    gh.close_grad(en.grad.cpu().numpy(), wn, "%s d/d noisy (module)" % name)


def test_ecda_loss_argument_checks():
    k = R.ecda_case("B5_Bn7")
    view = _view()
    c = PKG.config.dad_config_for(view, 1, 1, 1, 1, view.WARMUP_EPOCHS, 1)
    t = [_cuda(k[n]) for n in ("clean", "noisy", "yc", "pred")] + [_cuda(R.ecda_bool_mask(k).astype(np.uint8)),
                                                                   _cuda(k["scores"]), _cuda(k["w"])]
    loss = torch.zeros((), device="cuda")
    ws = torch.zeros(int(L.lib().dad_ecda_workspace_bytes(5, 7)), dtype=torch.uint8, device="cuda")

    def call(B, Bn, nw):
        return L.lib().dad_ecda_loss(c, t[0].data_ptr(), B, t[1].data_ptr(), Bn, t[2].data_ptr(), t[3].data_ptr(),
                                     t[4].data_ptr(), t[5].data_ptr(), t[6].data_ptr(), nw, loss.data_ptr(), None, None,
                                     ws.data_ptr(), _stream())
    assert call(5, 7, 5) == L.E_ARG and call(5, 7, 0) == L.E_ARG          # neither [4] nor ones(Bn)
    assert call(0, 7, 4) == L.E_SHAPE and call(5, 1025, 4) == L.E_SHAPE and call(1025, 7, 4) == L.E_SHAPE
    torch.cuda.synchronize()
