"""Parity of the fused HIP step (through the C ABI) with the reference goldens and the oracle.

Every golden step is an independent state transition from a seeded state (see
tests/golden/gen_golden.py); the HIP step starts from the same state with the same
injected draws (rng='explicit') in FP32 mode (exact-f32 MFMA).  Tolerance: 1e-4 relative
to the tensor's max magnitude (the north_star's loss/logit bound) for every float; the
DACP mask and pseudo-labels bit-exact.  Gradients, post-step parameters and Adam moments
use gpu_harness.close_grad (Frobenius-relative 1e-4, elementwise 1e-3): the ReLU' pattern
is a discrete decision that can flip on a pre-activation rounding to ~0.  BF16 mode is
checked against the oracle with a bf16-appropriate tolerance.
"""
import numpy as np
import pytest
import torch

import goldens
import gpu_harness as gh
from oracle import dad_oracle, synth

pytestmark = pytest.mark.gpu
TOL = 1e-4


def _cmp_loss(a, b, what):
    assert abs(a - b) <= TOL * max(1.0, abs(b)), (what, a, b)


@pytest.mark.parametrize("name", goldens.variants())
def test_fused_step_matches_reference_goldens(name):
    d, spec, cfg = goldens.load(name)
    step = gh.make_step(cfg, anchors=d["anchors"])
    orc = dad_oracle.DADOracle(*goldens.problem(spec), cfg, anchors=d["anchors"])
    idx = d["w1_index"]
    for s, epoch in goldens.schedule(d):
        p = "s%d_" % s
        st = goldens.state(spec, s)
        gh.load_state(step, st)
        orc.load_state(st)
        inp = goldens.step_inputs(spec, s)
        lr = float(d[p + "lr"])
        o = gh.run_step(step, inp, epoch, lr=lr)
        r = orc.step(inp, epoch, lr=lr)
        for k in ("total_loss", "supervised_ce_loss", "consistency_loss", "ecda_loss"):
            _cmp_loss(o[k], float(d[p + k]), (name, s, k))
        assert gh.rel(o["z_clean"], d[p + "z_clean"]) < TOL, (name, s)
        assert gh.rel(o["e_clean"], d[p + "e_clean"]) < TOL, (name, s)
        if p + "z_strong" in d:
            assert gh.rel(o["z_strong"], d[p + "z_strong"]) < TOL, (name, s)
            assert gh.rel(o["z_teacher"], d[p + "z_teacher"]) < TOL, (name, s)
            assert gh.rel(o["e_strong"], d[p + "e_strong"]) < TOL, (name, s)
            assert gh.rel(o["e_teacher"], d[p + "e_teacher"]) < TOL, (name, s)
            np.testing.assert_array_equal(o["pred"], np.argmax(d[p + "z_teacher"], 1))
        if p + "mask" in d:
            np.testing.assert_array_equal(o["mask"], d[p + "mask"])
            assert gh.rel(o["score"], d[p + "score"]) < TOL
            np.testing.assert_allclose(o["tau_after"], d[p + "tau_after"], atol=1e-6)
            np.testing.assert_allclose(o["w"], d[p + "w"], atol=1e-6)
            np.testing.assert_allclose(o["dacp"][0:4], d[p + "tau_after"], atol=1e-6)   # committed
        elif p + "z_strong" in d:                                                      # fixed threshold
            np.testing.assert_array_equal(o["mask"], r["mask"])
        _cmp_loss(float(o["clip_norm"]), float(d[p + "clip_norm"]), (name, s, "clip_norm"))
        coef = float(o["clip_coef"])
        g = [x * np.float32(coef) for x in o["grads"]]
        # full tensors against the oracle (pre-clip grads), then sampled vs the reference
        for k, (a, b_) in enumerate(zip(o["grads"], r["grads"])):
            gh.close_grad(a, b_, "%s step %d oracle grad %d" % (name, s, k))
        gh.close_grad(g[0].reshape(-1)[idx], d[p + "gW1c_s"], "%s step %d gW1" % (name, s))
        gh.close_grad(g[1], d[p + "gb1c"], "%s step %d gb1" % (name, s))
        gh.close_grad(g[2], d[p + "gW2c"], "%s step %d gW2" % (name, s))
        gh.close_grad(g[3], d[p + "gb2c"], "%s step %d gb2" % (name, s))
        for who in ("s", "t"):
            prm = o["student"] if who == "s" else o["teacher"]
            gh.close_grad(prm[0].reshape(-1)[idx], d[p + who + "W1_s"], "%s %d %sW1" % (name, s, who))
            gh.close_grad(prm[1], d[p + who + "b1"], "%s %d %sb1" % (name, s, who))
            gh.close_grad(prm[2], d[p + who + "W2"], "%s %d %sW2" % (name, s, who))
            gh.close_grad(prm[3], d[p + who + "b2"], "%s %d %sb2" % (name, s, who))
        gh.close_grad(o["student"][0], r["student"][0], "%s %d oracle sW1" % (name, s))
        gh.close_grad(o["teacher"][0], r["teacher"][0], "%s %d oracle tW1" % (name, s))
        gh.close_grad(o["exp_avg"][1], d[p + "exp_avg_b1"], "%s %d exp_avg" % (name, s))
        gh.close_grad(o["exp_avg_sq"][2], d[p + "exp_avg_sq_W2"], "%s %d exp_avg_sq" % (name, s))
    # epoch-end quality update over the post-warm-up steps' certainty statistics
    n = int(d["epoch_end_after_step"])
    with torch.no_grad():
        step.dacp[4:8].copy_(torch.from_numpy(goldens.state(spec, n)["Q"]))
    np.testing.assert_array_equal(step.dacp[12:16].cpu().numpy(), d["epoch_end_counts"])
    step.epoch_end()
    np.testing.assert_allclose(step.dacp[4:8].cpu().numpy(), d["epoch_end_Q"], atol=2e-6)
    assert float(step.dacp[8:16].abs().sum()) == 0.0


def _problem(B, T, seed=5, Bn=None, Tn=None, ragged=True, snr=5.0):
    """Inputs with independent clean/noisy geometry (the reference collates them separately)."""
    Bn = B if Bn is None else Bn
    Tn = T if Tn is None else Tn
    _, _, _, _, P = synth.init_weights(seed)
    xc, mc, yc = synth.make_batch(P, seed * 11 + 1, B, T, ragged=ragged)
    xn, mn, yn = synth.make_batch(P, seed * 11 + 2, Bn, Tn, snr_db=snr, noisy=True, ragged=ragged, label_shift=1)
    dr = synth.make_draws(seed * 11 + 3, Bn, Tn)
    dr["keep1"] = synth.make_draws(seed * 11 + 4, B, 1)["keep1"]
    return dict(xc=xc, mc=mc, yc=yc, xn=xn, mn=mn, yn=yn, **dr)


EDGE = [
    dict(B=1, T=1, Bn=2, Tn=3),          # smallest shapes, gates closed
    dict(B=5, T=33, Bn=7, Tn=31),        # slab boundary crossings, Bc != Bn, Tc != Tn
    dict(B=16, T=64, Bn=16, Tn=64),      # exact slab multiples
    dict(B=12, T=45, Bn=20, Tn=70, ragged=False),
    dict(B=64, T=40, Bn=64, Tn=40),
]


@pytest.mark.parametrize("geom", EDGE, ids=lambda g: "B%dT%d_Bn%dTn%d" % (g["B"], g["T"], g["Bn"], g["Tn"]))
@pytest.mark.parametrize("flavor", ["iemocap", "casia_ecda"])
def test_fused_step_edge_geometries_match_oracle(geom, flavor):
    """The inputs come from _problem(seed=5), the weights from synth.make_state(3, 1): the classifier is not
    confident on them, so the post-warm-up DACP mask is empty at every geometry (gates closed, consistency and
    ECDA loss 0) and the strong slabs add exactly nothing to the weight gradient.  The strong branch's gradient
    at these shapes is held to the oracle by tests/test_gpu_exact_operands.py."""
    if flavor == "casia_ecda":
        cfg = dad_oracle.make_cfg("casia", USE_ECDA=True)
    else:
        cfg = dad_oracle.make_cfg("iemocap")
    g = dict(geom)
    ragged = g.pop("ragged", True)
    inp = _problem(ragged=ragged, **g)
    st = synth.make_state(3, 1)
    step = gh.make_step(cfg)
    orc = dad_oracle.DADOracle(*synth.init_weights(3)[:4], cfg)
    for epoch in (0, 60):
        gh.load_state(step, st)
        orc.load_state(st)
        o = gh.run_step(step, inp, epoch)
        r = orc.step(inp, epoch)
        for k in ("total_loss", "supervised_ce_loss", "consistency_loss", "ecda_loss"):
            _cmp_loss(o[k], r[k], (geom, epoch, k))
        assert gh.rel(o["z_clean"], r["z_clean"]) < TOL
        if epoch >= 30:
            assert gh.rel(o["z_strong"], r["z_strong"]) < TOL
            np.testing.assert_array_equal(o["mask"], r["mask"])
        for k, (a, b_) in enumerate(zip(o["grads"], r["grads"])):
            gh.close_grad(a, b_, "%s epoch %d grad %d" % (geom, epoch, k))
        gh.close_grad(o["student"][0], r["student"][0], "%s epoch %d sW1" % (geom, epoch))


def test_bf16_step_close_to_oracle():
    """BF16 MFMA mode: embeddings/logits within bf16 rounding of the fp32 oracle."""
    cfg = dad_oracle.make_cfg("iemocap")
    inp = _problem(B=32, T=96, seed=9)
    st = synth.make_state(9, 2)
    step = gh.make_step(cfg, precision="bf16")
    orc = dad_oracle.DADOracle(*synth.init_weights(9)[:4], cfg)
    gh.load_state(step, st)
    orc.load_state(st)
    o = gh.run_step(step, inp, 60)
    r = orc.step(inp, 60)
    assert gh.rel(o["e_clean"], r["e_clean"]) < 2e-2
    assert gh.rel(o["z_clean"], r["z_clean"]) < 2e-2
    assert gh.rel(o["z_strong"], r["z_strong"]) < 2e-2
    assert abs(o["supervised_ce_loss"] - r["supervised_ce_loss"]) < 2e-2 * max(1, abs(r["supervised_ce_loss"]))
    # gradient direction agrees (bf16 operands, fp32 accumulate)
    g1 = np.concatenate([x.reshape(-1) for x in o["grads"]]).astype(np.float64)
    g2 = np.concatenate([x.reshape(-1) for x in r["grads"]]).astype(np.float64)
    if np.array_equal(o["mask"], r["mask"]):
        cos = g1 @ g2 / (np.linalg.norm(g1) * np.linalg.norm(g2))
        assert cos > 0.99, cos


def test_modular_encoder_bf16_matches_torch_fp32():
    """The modular encoder op in BF16 (set_precision): within bf16 rounding of the fp32 torch op,
    with padded frames and a slab count that leaves a sub-slab past every utterance's end."""
    import dadpkg
    p = dadpkg.pkg()
    torch.manual_seed(1)
    m = p.SSRLModel().cuda()
    m.set_precision(p._lib.PREC_BF16)
    B, T = 5, 300
    x = torch.randn(B, T, 768, device="cuda")
    pad = torch.zeros(B, T, dtype=torch.bool, device="cuda")
    pad[1, 140:] = True
    pad[3, 17:] = True
    enc = m.student_encoder
    e = enc(x, pad)
    torch.cuda.synchronize()
    W, b = enc.pre_net.weight.detach(), enc.pre_net.bias.detach()
    h = torch.relu(x @ W.T + b) * (~pad).unsqueeze(-1).float()
    ref = h.sum(1) / (~pad).float().sum(1, keepdim=True).clamp(min=1.0)
    assert torch.isfinite(e).all()
    assert gh.rel(e.detach().cpu(), ref.cpu()) < 2e-2


def test_modular_encoder_matches_torch_fp32():
    """Emotion2VecEncoder forward/backward (HIP) vs a plain PyTorch fp32 reference of the op."""
    import dadpkg
    p = dadpkg.pkg()
    torch.manual_seed(0)
    m = p.SSRLModel().cuda()
    B, T = 6, 37
    x = torch.randn(B, T, 768, device="cuda")
    pad = torch.zeros(B, T, dtype=torch.bool, device="cuda")
    pad[1, 20:] = True
    pad[4, 5:] = True
    enc = m.student_encoder
    e = enc(x, pad)
    W = enc.pre_net.weight.detach().clone().requires_grad_(True)
    b = enc.pre_net.bias.detach().clone().requires_grad_(True)
    h = torch.relu(x @ W.T + b) * (~pad).unsqueeze(-1).float()
    ref = h.sum(1) / (~pad).float().sum(1, keepdim=True).clamp(min=1.0)
    assert gh.rel(e.detach().cpu(), ref.detach().cpu()) < 1e-5
    g = torch.randn(B, 256, device="cuda")
    (e * g).sum().backward()
    (ref * g).sum().backward()
    assert gh.rel(enc.pre_net.weight.grad.cpu(), W.grad.cpu()) < 1e-5
    assert gh.rel(enc.pre_net.bias.grad.cpu(), b.grad.cpu()) < 1e-5
    # predict / get_embeddings (eval path) and the teacher EMA entry point
    logits = m.predict(x, pad)
    assert logits.shape == (B, 4)
    t0 = m.teacher_flat.clone()
    with torch.no_grad():
        m.student_flat.add_(1.0)
    m.update_teacher_ema()
    exp = t0 * np.float32(0.99) + m.student_flat * np.float32(1.0 - 0.99)
    assert gh.rel(m.teacher_flat.cpu(), exp.cpu()) < 1e-6


def test_train_step_shim_with_reference_loop_body():
    """Autograd-compatible train_step + the reference's own loop body (I/train.py:484-492):
    total_loss.backward(), torch clip_grad_norm_, torch Adam (seeded with the same moments),
    update_teacher_ema -- against the oracle's full step."""
    cfg = dad_oracle.make_cfg("iemocap")
    inp = _problem(B=16, T=40, seed=4)
    st = synth.make_state(4, 1)
    step = gh.make_step(cfg)
    gh.load_state(step, st)
    orc = dad_oracle.DADOracle(*synth.init_weights(4)[:4], cfg)
    orc.load_state(st)
    m = step.model
    m.ema_momentum = cfg["EMA_MOMENTUM"]
    params = m._plist(m.student_encoder, m.student_classifier)
    lr = dad_oracle.cosine_lr(cfg, 60)
    opt = torch.optim.Adam(params, lr=lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=cfg["WEIGHT_DECAY"])
    for p, ea, eas in zip(params, st["exp_avg"], st["exp_avg_sq"]):
        opt.state[p] = {"step": torch.tensor(float(st["nstep"])),
                        "exp_avg": torch.from_numpy(np.asarray(ea, np.float32)).cuda(),
                        "exp_avg_sq": torch.from_numpy(np.asarray(eas, np.float32)).cuda()}
    clean, noisy, draws = gh.batches(inp)
    opt.zero_grad()
    losses = step.train_step(clean, noisy, 60, draws=draws)
    assert losses["total_loss"].requires_grad
    losses["total_loss"].backward()
    torch.nn.utils.clip_grad_norm_(params, cfg["MAX_GRAD_NORM"])
    opt.step()
    m.update_teacher_ema()
    torch.cuda.synchronize()
    r = orc.step(inp, 60)
    for k in ("total_loss", "supervised_ce_loss", "consistency_loss", "ecda_loss"):
        _cmp_loss(float(losses[k].detach()), r[k], k)
    student = gh.unflat(m.student_flat.detach().cpu().numpy())
    teacher = gh.unflat(m.teacher_flat.detach().cpu().numpy())
    for k in range(4):
        gh.close_grad(student[k], r["student"][k], "shim student %d" % k)
        gh.close_grad(teacher[k], r["teacher"][k], "shim teacher %d" % k)
    np.testing.assert_allclose(step.dacp[0:4].cpu().numpy(), r["tau_after"], atol=1e-6)
    # a fused step afterwards sees the caller-updated parameters (bf16 shadows refreshed)
    assert step._shadow_dirty


@pytest.mark.parametrize("prec", ["fp32", "fp16"])
@pytest.mark.parametrize("class_aware,B", [(True, 200), (False, 96), (True, 64), (False, 64)],
                         ids=["class_aware", "global_mmd", "class_aware_b64", "global_mmd_b64"])
def test_large_member_sets_match_oracle(class_aware, B, prec):
    """Large member sets: beyond the LDS-staged size (ECDA_NZ = 80 rows in csrc/tail_general.hip) the
    member rows and the distance matrix go through the global-memory path of dad_tail_ecda's
    class blocks, and the DACP ranks span several 512-thread rounds (B = 200 / 96, no register
    prefetch).  B = 64: the prefetch path (every row in registers at entry) with one class
    holding every clean utterance.  fp16 (the timed mode's operands; the tail arithmetic is fp32
    in every mode): losses at north_star's 1e-4, the mask bit-exact, logits within test_gpu_16bit's
    bound for short synthetic utterances (T = 6 here: little averaging of the operand rounding;
    measured 1.9e-4), gradients within test_gpu_throughput_parity's fp16 bounds."""
    cfg = dad_oracle.make_cfg("iemocap", USE_CLASS_AWARE_MMD=class_aware)
    inp = _problem(B, 6, seed=9, snr=20.0)
    if class_aware:
        inp["yc"] = np.zeros_like(inp["yc"])          # one class holds every clean utterance
    st = synth.make_state(4, 1, tau_range=(0.0, 0.01))   # low thresholds: most noisy rows masked in
    step = gh.make_step(cfg, precision=prec)
    orc = dad_oracle.DADOracle(*synth.init_weights(4)[:4], cfg)
    gh.load_state(step, st)
    orc.load_state(st)
    o = gh.run_step(step, inp, 60)
    r = orc.step(inp, 60)
    assert r["ecda_loss"] != 0.0 and int(np.sum(r["mask"])) > (80 if B > 64 else 16)
    for k in ("total_loss", "supervised_ce_loss", "consistency_loss", "ecda_loss"):
        _cmp_loss(o[k], r[k], (class_aware, prec, k))
    np.testing.assert_array_equal(o["mask"], r["mask"])
    if prec == "fp32":
        for k, (a, b_) in enumerate(zip(o["grads"], r["grads"])):
            gh.close_grad(a, b_, "large B grad %d" % k)
        return
    from test_gpu_throughput_parity import TOL, _cos, _normrel
    from test_gpu_16bit import LOGIT_TOL
    for k in ("z_clean", "z_strong", "z_teacher"):   # six-frame utterances: test_gpu_16bit's synthetic bound
        assert gh.rel(o[k], r[k]) <= LOGIT_TOL["fp16"], (class_aware, k, gh.rel(o[k], r[k]))
    g = np.concatenate([x.reshape(-1) for x in o["grads"]])
    gr = np.concatenate([np.asarray(x).reshape(-1) for x in r["grads"]])
    print("fp16 large B=%d class_aware=%s: grad normrel %.3g cos %.7f" % (B, class_aware, _normrel(g, gr), _cos(g, gr)))
    assert _normrel(g, gr) <= TOL["fp16"]["grad"] and _cos(g, gr) >= TOL["fp16"]["cos"]


LARGE_CLASS_CASES = {
    # clean label counts, DACP thresholds (None: synth's low ones), what the geometry must show
    "one_large": ((40, 8, 8, 8), None, "large"),
    "two_large": ((30, 30, 2, 2), None, "large"),
    "idle_others": ((20, 16, 14, 14), (0.0, 1.0, 1.0, 1.0), "large,idle"),
    "partial_mask": ((20, 16, 14, 14), (0.82, 0.0, 0.0, 0.0), "partial"),
    "partial_mask_large": ((40, 8, 8, 8), (0.82, 0.0, 0.0, 0.0), "large,partial"),
}


@pytest.mark.parametrize("prec", ["fp32", "fp16"])
@pytest.mark.parametrize("case", sorted(LARGE_CLASS_CASES))
def test_large_class_tiling_matches_oracle(case, prec):
    """ECDA classes of 33..64 members (clean rows of the label + masked noisy rows of the
    pseudo-label): dad_tail_ecda_w's 64-row tiling of a class block (3 Gram tile pairs, the
    coefficient columns of ceil(n / 8) 8-candidate blocks).  one_large / two_large: one or two
    such classes next to classes with work; idle_others: thresholds mask in only class 0's noisy
    rows (36 members), so classes 1..3 have neither ECDA nor repulsion work (the geometry of a
    collapsed teacher).  partial_mask(_large): class 0's threshold leaves 6 of its 16 noisy rows of
    pseudo-label 0 out of the mask; they are not members (I/utils.py:573-576) and the class blocks
    no longer stage them (round 6: they had sized the tiling, up to the wide path).  Losses at 1e-4,
    mask bit-exact, gradients as the other parity tests (fp32: gh.close_grad; fp16: the throughput
    bounds); the test checks that the geometry does produce what the case names."""
    counts, tau, expect = LARGE_CLASS_CASES[case]
    cfg = dad_oracle.make_cfg("iemocap")
    inp = _problem(64, 6, seed=21, snr=20.0)
    inp["yc"] = np.repeat(np.arange(4), counts).astype(inp["yc"].dtype)
    st = synth.make_state(21, 1, tau_range=(0.0, 0.01))     # low thresholds: most noisy rows masked in
    if tau is not None:
        st["tau"] = np.asarray(tau, np.float32)
    step = gh.make_step(cfg, precision=prec)
    orc = dad_oracle.DADOracle(*synth.init_weights(21)[:4], cfg)
    gh.load_state(step, st)
    orc.load_state(st)
    o = gh.run_step(step, inp, 60)
    r = orc.step(inp, 60)
    m = np.asarray(r["mask"]) > 0
    pred = np.asarray(r["pred"])
    members = [int(np.sum(inp["yc"] == c)) + int(np.sum((pred == c) & m)) for c in range(4)]
    if "large" in expect:
        assert any(32 < n <= 64 for n in members), members
    if "idle" in expect:   # one class with work, the others idle
        assert [int(np.sum((pred == c) & m)) for c in range(1, 4)] == [0, 0, 0], members
    if "partial" in expect:
        assert 0 < int(np.sum((pred == 0) & ~m)) < int(np.sum(pred == 0)), members
    for k in ("total_loss", "supervised_ce_loss", "consistency_loss", "ecda_loss"):
        _cmp_loss(o[k], r[k], (case, prec, k))
    np.testing.assert_array_equal(o["mask"], r["mask"])
    if prec == "fp32":
        for k, (a, b_) in enumerate(zip(o["grads"], r["grads"])):
            gh.close_grad(a, b_, "large class grad %d" % k)
        return
    from test_gpu_throughput_parity import TOL, _cos, _normrel
    g = np.concatenate([x.reshape(-1) for x in o["grads"]])
    gr = np.concatenate([np.asarray(x).reshape(-1) for x in r["grads"]])
    assert _normrel(g, gr) <= TOL["fp16"]["grad"] and _cos(g, gr) >= TOL["fp16"]["cos"], members


@pytest.mark.parametrize("prec", ["fp32", "fp16"])
def test_ecda_bandwidth_with_large_common_embedding_offset(prec):
    """the detached MMD bandwidth (I/utils.py:537-544, the mean pairwise squared
    distance) is computed from per-class partial sums, sum_ij |z_i - z_j|^2 = 2n sum|d_i|^2 -
    2|sum d_i|^2 with d_i = z_i - z0.  With z0 = 0 that identity cancels digits when the pooled
    embeddings share a large mean (|mean|^2 / variance); the kernel centres on a member row.  Here
    b1 += 30 makes every hidden unit active with a common offset of ~30 and the ECDA loss and
    gradients are held to the float64 oracle's."""
    cfg = dad_oracle.make_cfg("iemocap")
    inp = _problem(64, 40, seed=13, snr=20.0)
    st = synth.make_state(13, 1, tau_range=(0.0, 0.01))     # low thresholds: ECDA members on
    for net in ("student", "teacher"):
        st[net] = [np.array(a, np.float32) for a in st[net]]
        st[net][1] = st[net][1] + np.float32(30.0)
    W1, b1, W2, b2, _ = synth.init_weights(13)
    orc = dad_oracle.DADOracle(W1, b1, W2, b2, cfg)
    orc.load_state(st)
    step = gh.make_step(cfg, precision=prec)
    gh.load_state(step, st)
    o = gh.run_step(step, inp, 60)
    r = orc.step(inp, 60)
    e = np.asarray(r["e_clean"], np.float64)
    assert e.mean() > 20.0 and r["ecda_loss"] != 0.0, (e.mean(), r["ecda_loss"])
    tol = 1e-4
    for k in ("ecda_loss", "total_loss"):
        err = abs(o[k] - r[k]) / max(1.0, abs(r[k]))
        print("%s offset-30 %s: got %.9g want %.9g rel %.3g" % (prec, k, o[k], r[k], err))
        assert err <= tol, (prec, k, o[k], r[k], err)
    if prec == "fp32":
        for k, (a, b_) in enumerate(zip(o["grads"], r["grads"])):
            gh.close_grad(a, b_, "offset-30 grad %d" % k)
