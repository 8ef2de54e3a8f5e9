"""The supervised-contrastive term on the MI355X (csrc/scl.hip): dad_scl alone against the float64 definition
(tests/scl_ref.py), and the train step with the term switched on against the same step with the weight 0, the
oracle's gradient plus the term's float64 autograd, a captured graph and preparation ahead.

Bounds.  Loss and gradient of dad_scl: the project's 1e-4 (gpu_harness.close: max-abs over max |ref|); the same
formulas in float32 on the CPU stay below 1e-5 on these inputs (tests/test_scl_ref_cpu.py), so a miss means a wrong
term or a wrong order of summation.  The step's dW1 / db1: gpu_harness.close_grad's bounds in fp32; in fp16 the
gradient bound of tests/test_gpu_16bit.py (direction cosine > 0.99 when the discrete DACP mask agrees).  Every element
of the step's dW1 and db1 with the term on is held to a float64 reference, in fp32, fp16 and bf16, by
tests/test_gpu_exact_scl.py."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import dadpkg
import gpu_harness as gh
import scl_ref as R
from oracle import dad_oracle, synth
from test_gpu_graph import _device_batches, _state
from test_gpu_parity import _problem

pytestmark = pytest.mark.gpu
PKG = dadpkg.pkg()
LIB = PKG._lib
TOL = 1e-4


@functools.lru_cache(None)
def _case(n, kind, tau):
    """(emb, labels, member, reference loss, reference gradient, stats); computed once, never modified."""
    emb, y, mem = R.gpu_case(n, kind)
    loss, grad = R.scl_autograd(emb, y, mem, tau)
    return emb, y, mem, loss, grad, R.stats(emb, y, mem)


def _run(emb, y, mem, tau, chunks=0, want_grad=True):
    """dad_scl_chunked -> (out [8], grad [n][256] or None) as NumPy arrays."""
    L = PKG.lib()
    n = emb.shape[0]
    e = torch.from_numpy(np.ascontiguousarray(emb)).cuda()
    yy = torch.from_numpy(np.ascontiguousarray(y)).cuda()
    mm = torch.from_numpy(np.ascontiguousarray(mem)).cuda()
    out = torch.full((LIB.SCL_SLOTS,), -7.0, device="cuda")
    grad = torch.full((n, 256), -7.0, device="cuda") if want_grad else None
    ws = torch.empty(int(L.dad_scl_workspace_bytes(n)), dtype=torch.uint8, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    LIB.check(L.dad_scl_chunked(e.data_ptr(), yy.data_ptr(), mm.data_ptr(), n, tau, out.data_ptr(),
                                grad.data_ptr() if want_grad else None, chunks, ws.data_ptr(), stream), "dad_scl")
    torch.cuda.synchronize()
    return out.cpu().numpy(), (grad.cpu().numpy() if want_grad else None)


def _check(out, grad, case, what):
    emb, y, mem, loss, ref, st = case
    print("%s: loss %.9g ref %.9g rel %.3g; grad rel %.3g; V %d |A| %d" % (
        what, out[LIB.SCL_LOSS], loss, R.rel(out[LIB.SCL_LOSS], loss), R.rel(grad, ref), st["V"], st["members"]))
    assert out[LIB.SCL_V] == st["V"] and out[LIB.SCL_MEMBERS] == st["members"]
    assert list(out[LIB.SCL_ANCHORS:LIB.SCL_ANCHORS + 4]) == list(st["anchors"])
    assert out[LIB.SCL_NONFINITE] == st["nonfinite"]
    gh.close(out[LIB.SCL_LOSS], loss, TOL, what + " loss")
    gh.close(grad, ref, TOL, what + " grad")
    outside = np.setdiff1d(np.arange(emb.shape[0]), R.members(emb, y, mem))
    assert not np.any(grad[outside]), what + ": a row outside the member set has a gradient"
    assert np.all(np.isfinite(grad))


@pytest.mark.parametrize("tau", R.GPU_TAUS)
@pytest.mark.parametrize("n", R.GPU_NS)
def test_dad_scl_matches_the_definition(n, tau):
    case = _case(n, "plain", tau)
    out, grad = _run(*case[:3], tau)
    _check(out, grad, case, "n=%d tau=%g" % (n, tau))
    if n >= 7:
        assert case[5]["V"] > 0 and case[5]["members"] < n


@pytest.mark.parametrize("tau", [0.07, 0.5])
@pytest.mark.parametrize("n", [7, 65, 130])
@pytest.mark.parametrize("kind", [k for k in R.GPU_KINDS if k != "plain"])
def test_dad_scl_edge_cases(kind, n, tau):
    """A class with one member, no positives at all, non-members holding NaN / inf, a zero row flagged as a member,
    identical rows."""
    case = _case(n, kind, tau)
    out, grad = _run(*case[:3], tau)
    _check(out, grad, case, "%s n=%d tau=%g" % (kind, n, tau))
    if kind == "no_positives":
        assert out[LIB.SCL_LOSS] == 0.0 and out[LIB.SCL_V] == 0 and not np.any(grad)


def test_flagged_nonfinite_rows_are_counted():
    emb, y, mem = (a.copy() for a in R.gpu_case(65, "plain"))
    rows = [i for i in range(65) if mem[i] and 0 <= y[i] < 4][:2]
    emb[rows[0], 3] = np.nan
    emb[rows[1], 200] = np.inf
    out, _ = _run(emb, y, mem, 0.1)
    assert out[LIB.SCL_NONFINITE] == 2 == R.stats(emb, y, mem)["nonfinite"]


@pytest.mark.parametrize("chunks", [1, 2, 3])
def test_forced_chunk_counts(chunks):
    """n = 130 is three row tiles: one, two (2 + 1 tiles) and three column chunks per row tile."""
    case = _case(130, "plain", 0.1)
    out, grad = _run(*case[:3], 0.1, chunks=chunks)
    _check(out, grad, case, "n=130 chunks=%d" % chunks)
    edge = _case(130, "nan_nonmembers", 0.07)
    out, grad = _run(*edge[:3], 0.07, chunks=chunks)
    _check(out, grad, edge, "n=130 nan_nonmembers chunks=%d" % chunks)


def test_two_calls_are_bit_identical_and_null_grad_writes_only_out():
    case = _case(130, "identical", 0.07)
    a = _run(*case[:3], 0.07)
    b = _run(*case[:3], 0.07)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
    out, none = _run(*case[:3], 0.07, want_grad=False)
    assert none is None and out.tobytes() == a[0].tobytes()


def test_large_and_tiny_temperatures_stay_finite():
    """The log-sum-exp runs under a running row maximum: 1 / tau = 1e4 neither overflows nor meets log 0.  (The
    loss is then of the order (1 - s) / tau ~ 1e3 and the fp32 similarities' 1e-7 makes 1e-3 of it: 1e-6.)"""
    emb, y, mem = R.gpu_case(65, "plain")
    for tau in (1e-4, 50.0):
        loss, ref = R.scl_autograd(emb, y, mem, tau)
        out, grad = _run(emb, y, mem, tau)
        print("tau=%g: loss %.9g ref %.9g" % (tau, out[LIB.SCL_LOSS], loss))
        assert np.isfinite(out[LIB.SCL_LOSS]) and np.all(np.isfinite(grad))
        gh.close(out[LIB.SCL_LOSS], loss, TOL, "tau=%g loss" % tau)


def test_supervised_contrastive_loss_module():
    emb, y, mem, loss, ref, _ = _case(65, "plain", 0.1)
    f = torch.from_numpy(emb).cuda().requires_grad_(True)
    crit = PKG.SupervisedContrastiveLoss(temperature=0.1)
    out = crit(f, torch.from_numpy(y).cuda(), torch.from_numpy(mem).cuda())
    (2.0 * out).backward()
    gh.close(float(out.detach()), loss, TOL, "module loss")
    gh.close(f.grad.cpu().numpy(), 2.0 * ref, TOL, "module grad")
    assert int(crit.last_stats[LIB.SCL_MEMBERS]) == len(R.members(emb, y, mem))
    # mask = None: every row is flagged
    l_all, _ = R.scl_autograd(emb, y, np.ones(65, np.uint8), 0.1)
    gh.close(float(crit(f.detach(), torch.from_numpy(y).cuda())), l_all, TOL, "module loss, no mask")


# ------------------------------------------------------------------------------------------------- the step

W_SCL = 1.0
EPOCH = 60
FWD = ("e_clean", "e_teacher", "e_strong", "z_clean", "z_teacher", "z_strong", "score", "pred", "mask", "q")
LOSSES = ("supervised_ce_loss", "consistency_loss", "ecda_loss")


def _cfgs(**kw):
    base = dict(GRADIENT_CLIPPING=False, SCL_START_EPOCH=0, SCL_TEMPERATURE=0.1, **kw)
    return (dad_oracle.make_cfg("iemocap", TARGET_SCL_WEIGHT=W_SCL, **base),
            dad_oracle.make_cfg("iemocap", TARGET_SCL_WEIGHT=0.0, **base))


def _scl_through_encoder(inp, st, cfg, pred, mask, tau):
    """(loss, dW1, db1) of w_scl * SCL in float64, by autograd through a float64 restatement of the student's
    masked-mean ReLU encoder on the clean rows and the strong-augmented noisy rows."""
    W1 = torch.tensor(st["student"][0], dtype=torch.float64, requires_grad=True)
    b1 = torch.tensor(st["student"][1], dtype=torch.float64, requires_grad=True)

    def enc(x, pad):
        valid = torch.from_numpy(~np.asarray(pad, bool)).double()
        act = torch.relu(torch.from_numpy(np.asarray(x, np.float64)) @ W1.T + b1) * valid[..., None]
        return act.sum(1) / torch.clamp(valid.sum(1), min=1.0)[:, None]

    xs = dad_oracle.strong_augment(inp["xn"], inp["ns"], inp["u"], inp["start"], cfg["STRONG_NOISE_STD"],
                                   cfg["DROPOUT_RATE"], cfg["TEMPORAL_MASK_RATIO"])
    e = torch.cat([enc(inp["xc"], inp["mc"]), enc(xs, inp["mn"])])
    labels = np.concatenate([inp["yc"], np.asarray(pred, np.int64)])
    member = np.concatenate([np.ones(len(inp["yc"]), np.uint8), (np.asarray(mask) != 0).astype(np.uint8)])
    idx = R.members(e.detach().numpy(), labels, member)
    loss = R.scl_torch(e[torch.from_numpy(idx)], labels[idx], tau)
    (W_SCL * loss).backward()
    return float(loss.detach()), W1.grad.numpy(), b1.grad.numpy()


def _on_off(B, precision, seed, cfg_kw=None, tau_range=(0.0, 0.01), Bn=None):
    cfg_on, cfg_off = _cfgs(**(cfg_kw or {}))
    inp = _problem(B=B, T=40, seed=seed, Bn=Bn)
    st = synth.make_state(seed, 1, tau_range=tau_range)
    outs = []
    for cfg in (cfg_on, cfg_off):
        step = gh.make_step(cfg, precision=precision)
        gh.load_state(step, st)
        outs.append(gh.run_step(step, inp, EPOCH))
    orc = dad_oracle.DADOracle(*synth.init_weights(seed)[:4], cfg_off)
    orc.load_state(st)
    return cfg_on, inp, st, outs[0], outs[1], orc.step(inp, EPOCH)


def _check_step(B, precision, seed, cfg_kw=None, tau_range=(0.0, 0.01), Bn=None, masked_in="most"):
    cfg, inp, st, on, off, ref = _on_off(B, precision, seed, cfg_kw, tau_range, Bn)
    what = "B%d %s seed %d" % (B, precision, seed)
    Bn = B if Bn is None else Bn
    n_in = int((on["mask"] != 0).sum())
    print("%s: %d of %d noisy rows masked in; scl %.7g total on %.7g off %.7g" % (
        what, n_in, Bn, on["scl_loss"], on["total_loss"], off["total_loss"]))
    assert (n_in > Bn // 2) if masked_in == "most" else (0 < n_in < Bn)
    # the forward pass and the other losses: the same bits
    for k in FWD:
        assert np.array_equal(on[k], off[k]), k
    for k in LOSSES:
        assert on[k] == off[k], k
    assert "scl_loss" not in off
    # the loss of the device's own embeddings, labels, pseudo-labels and mask
    emb = np.concatenate([on["e_clean"], on["e_strong"]])
    labels = np.concatenate([inp["yc"], on["pred"].astype(np.int64)])
    member = np.concatenate([np.ones(B, np.uint8), (on["mask"] != 0).astype(np.uint8)])
    want, _ = R.scl_autograd(emb, labels, member, cfg["SCL_TEMPERATURE"])
    assert want > 0
    gh.close(on["scl_loss"], want, TOL, what + " scl_loss")
    d = (on["total_loss"] - off["total_loss"]) - W_SCL * on["scl_loss"]
    assert abs(d) <= TOL * abs(on["total_loss"]), (what, d)
    # the term never passes through the classifier
    assert np.array_equal(on["grads"][2], off["grads"][2]) and np.array_equal(on["grads"][3], off["grads"][3])
    assert not np.array_equal(on["grads"][0], off["grads"][0])
    # dW1, db1: the oracle's gradient plus the term's float64 autograd through the encoder
    assert np.array_equal(on["mask"], ref["mask"]) and np.array_equal(on["pred"], ref["pred"]), what + ": DACP mask"
    _, gw, gb = _scl_through_encoder(inp, st, cfg, ref["pred"], ref["mask"], cfg["SCL_TEMPERATURE"])
    share = np.linalg.norm(gw) / np.linalg.norm(ref["grads"][0] + gw)
    print("%s: the term is %.3g of |dW1|" % (what, share))
    assert share > 1e-3
    if precision == "fp32":
        gh.close_grad(on["grads"][0], ref["grads"][0] + gw, what + " dW1")
        gh.close_grad(on["grads"][1], ref["grads"][1] + gb, what + " db1")
        gh.close_grad(off["grads"][0], ref["grads"][0], what + " dW1, weight 0")
    else:
        a = np.concatenate([on["grads"][0].reshape(-1), on["grads"][1]]).astype(np.float64)
        b = np.concatenate([(ref["grads"][0] + gw).reshape(-1), ref["grads"][1] + gb]).astype(np.float64)
        assert a @ b / (np.linalg.norm(a) * np.linalg.norm(b)) > 0.99, what
        # and the term's own share of it: the difference of the two steps against the autograd
        da = (on["grads"][0].astype(np.float64) - off["grads"][0]).reshape(-1)
        assert da @ gw.reshape(-1) / (np.linalg.norm(da) * np.linalg.norm(gw)) > 0.99, what


@pytest.mark.parametrize("precision", ["fp32", "fp16"])
@pytest.mark.parametrize("B", [8, 16])
def test_step_with_the_term_against_weight_zero(B, precision):
    _check_step(B, precision, seed=40 + B)


def test_step_with_default_thresholds_masks_some_rows_in():
    _check_step(16, "fp32", seed=3, tau_range=(0.55, 0.9), masked_in="some")      # 12 of the 16 noisy rows


@pytest.mark.parametrize("precision", ["fp32", "fp16"])
def test_step_without_ecda_flags_rows_for_the_term_alone(precision):
    _check_step(8, precision, seed=51, cfg_kw={"USE_ECDA": False})


def test_step_at_b80_takes_the_general_tail():
    cfg = PKG.dad_config_for(PKG.ConfigView(_cfgs()[0], flavor="iemocap"), 80, 40, 80, 40, EPOCH, 1)
    info = LIB.DadStepPlanInfo()
    LIB.check(PKG.lib().dad_step_plan(cfg, None, None, 0, 256, info), "dad_step_plan")
    assert info.tail == b"dad_tail_ecda" and info.pool_grid > 0
    _check_step(80, "fp32", seed=9)


def test_warmup_and_early_epochs_run_without_the_term():
    cfg_on, cfg_off = _cfgs()
    cfg_late = dict(cfg_on, SCL_START_EPOCH=EPOCH + 1)
    inp = _problem(B=8, T=40, seed=3)
    st = synth.make_state(3, 1, tau_range=(0.0, 0.01))
    for cfg, epoch in ((cfg_on, 5), (cfg_late, EPOCH)):
        res = []
        for c in (cfg, cfg_off):
            step = gh.make_step(c, precision="fp32")
            gh.load_state(step, st)
            res.append(gh.run_step(step, inp, epoch))
        assert res[0]["total_loss"] == res[1]["total_loss"] and "scl_loss" not in res[0]
        for a, b in zip(res[0]["grads"], res[1]["grads"]):
            assert np.array_equal(a, b)


@pytest.mark.parametrize("precision,rng", [("fp32", "explicit"), ("fp16", "counter")])
def test_captured_step_with_the_term_replays_like_eager(precision, rng):
    cfg = _cfgs()[0]
    inp = _problem(B=16, T=40, seed=21, Bn=12, Tn=50)
    st = synth.make_state(21, 1, tau_range=(0.0, 0.01))
    clean, noisy, draws = _device_batches(inp)
    dr = draws if rng == "explicit" else None
    eager = gh.make_step(cfg, precision=precision, rng=rng, seed=3)
    gh.load_state(eager, st)
    n0, g0 = eager.adam_step, eager.global_step
    le = eager.step(clean, noisy, EPOCH, draws=dr)
    torch.cuda.synchronize()
    want, want_losses = _state(eager), {k: float(v) for k, v in le.items()}
    assert want_losses["scl_loss"] > 0

    cap = gh.make_step(cfg, precision=precision, rng=rng, seed=3)
    gh.load_state(cap, st)
    side = torch.cuda.Stream()          # one eager step first: the lazy buffers, then back to the start state
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        cap.step(clean, noisy, EPOCH, draws=dr)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    gh.load_state(cap, st)
    with torch.no_grad():
        cap.dacp[8:16].zero_()
    cap.adam_step, cap.global_step = n0, g0
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        lc = cap.step(clean, noisy, EPOCH, draws=dr)
    g.replay()
    torch.cuda.synchronize()
    for name, a, b in zip(("student", "teacher", "exp_avg", "exp_avg_sq", "dacp", "grad"), _state(cap), want):
        assert torch.equal(a, b), name
    for k, v in lc.items():
        assert float(v) == want_losses[k], k


def test_preparation_ahead_with_the_term_gives_the_same_bits():
    cfg = _cfgs()[0]
    st = synth.make_state(21, 1, tau_range=(0.0, 0.01))
    data = [_device_batches(_problem(B=16, T=40, seed=s, Bn=12, Tn=50))[:2] for s in (31, 32)]
    res = []
    for ahead in (False, True):
        step = gh.make_step(cfg, precision="fp16", rng="counter", seed=3)
        gh.load_state(step, st)
        step.step(*data[0], EPOCH, next_batch=data[1] if ahead else None)
        losses = step.step(*data[1], EPOCH)
        torch.cuda.synchronize()
        assert step.last_prepped == ahead
        res.append((_state(step), {k: float(v) for k, v in losses.items()}))
    for name, a, b in zip(("student", "teacher", "exp_avg", "exp_avg_sq", "dacp", "grad"), res[0][0], res[1][0]):
        assert torch.equal(a, b), name
    assert res[0][1] == res[1][1] and res[0][1]["scl_loss"] > 0
