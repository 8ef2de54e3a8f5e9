"""dad_optim on its own (csrc/optim.hip) against the float64 reference of tests/optim_ref.py, within
per-element bounds counted in float32 roundings: the whole-step tests see the parameters only to a
tolerance wider than one update, and nothing else compares the W1 moments with a reference.

Vehicle 1, apply only: dad_step_apply with dp_world = 2 and no communicator runs dad_norm (which halves
the stored gradient 2 G exactly) and then dad_optim on exactly the gradient the test chose, over state
vectors the test owns -- so they can also start one float past a 16-byte boundary, which is the only way
into the kernel's scalar path.  Vehicle 2, whole step: the step's own gradient and squared-norm partials.

The vectors are the seeded 197,892-element cases of optim_ref.make_case (W1 included in full); the
bounds are validated without a GPU by tests/test_optim_ref_cpu.py."""
import numpy as np
import pytest
import torch

import dadpkg
import gpu_harness as gh
import optim_ref as R
from oracle import dad_oracle, synth
from test_gpu_parity import _problem

pytestmark = pytest.mark.gpu
PKG = dadpkg.pkg()
LIB = PKG._lib
NP = LIB.DAD_NPARAM
F = np.float32
TDT = {"fp16": torch.float16, "bf16": torch.bfloat16}
ALPHA = 0.9                                     # DACP_THRESHOLD_SMOOTHING_ALPHA of the iemocap config
EX = np.array([0.61, 0.72, 0.55, 0.83,          # floored thresholds (summed over the two "ranks")
               1.25, 0.5, 2.75, 0.0,            # per-class certainty sums
               3.0, 1.0, 5.0, 0.0,              # per-class counts
               2.5, 1.5, 0.75, 0.25], F)        # losses (summed)
DACP0 = np.array([0.7, 0.6, 0.8, 0.65, 0.5, 0.4, 0.6, 0.55, 1.5, 0.25, 0.0, 2.0, 4.0, 1.0, 0.0, 3.0,
                  0.5, 0.6, 0.7, 0.8], F)


class Vehicle:
    """A DADStep at the smallest geometry (B=1, T=1, Bn=2, Tn=3) that lends its config, tail buffer and
    workspace; the optimizer state lives in tensors of this object, `off` floats past their allocation."""

    def __init__(self, precision="fp32", off=0):
        self.step = gh.make_step(dad_oracle.make_cfg("iemocap"), precision=precision, rng="counter", seed=1)
        self.precision = precision
        dev = self.step.device
        self.clean = {"net_input": {"feats": torch.zeros(1, 1, 768), "padding_mask": torch.zeros(1, 1, dtype=torch.bool)},
                      "labels": torch.zeros(1, dtype=torch.int64)}
        self.noisy = {"net_input": {"feats": torch.zeros(2, 3, 768), "padding_mask": torch.zeros(2, 3, dtype=torch.bool)},
                      "labels": torch.zeros(2, dtype=torch.int64)}
        self._raw = {k: torch.zeros(NP + LIB.DAD_GRAD_EXTRA + off, device=dev)
                     for k in ("student", "teacher", "exp_avg", "exp_avg_sq", "grad")}
        self.t = {k: v[off:] for k, v in self._raw.items()}
        for k, v in self.t.items():
            assert v.data_ptr() % 16 == (4 * off) % 16, k
        self.shadow = {k: torch.zeros(R.NW1, dtype=torch.int16, device=dev) for k in ("student", "teacher")}
        self.dacp = torch.zeros(LIB.DAD_DACP_FLOATS, device=dev)

    def config(self, t, lr, warmup=False, **fields):
        s = self.step
        s.adam_step = t - 1
        cfg, bt, st = s._prepare(self.clean, self.noisy, 60, lr, None)
        self.ws = s._workspace(cfg)
        cfg = LIB.DadConfig.from_buffer_copy(cfg)
        cfg.dp_world = 2
        cfg.warmup = int(warmup)
        for k, v in fields.items():
            setattr(cfg, k, v)
        st = LIB.DadState.from_buffer_copy(st)
        for k in ("student", "teacher", "exp_avg", "exp_avg_sq", "grad"):
            setattr(st, k, self.t[k].data_ptr())
        st.w1bf_student, st.w1bf_teacher = self.shadow["student"].data_ptr(), self.shadow["teacher"].data_ptr()
        st.dacp = self.dacp.data_ptr()
        self.st, self.tail = st, s._last["tail"]
        return cfg

    def load(self, inp, G=None, ex=EX, dacp=DACP0):
        put = lambda dst, a: dst[:len(a)].copy_(torch.tensor(np.asarray(a)))
        put(self.t["student"], inp["p"]), put(self.t["teacher"], inp["teacher"])
        put(self.t["exp_avg"], inp["m"]), put(self.t["exp_avg_sq"], inp["v"])
        self.set_grad(inp["G"] if G is None else G, ex)
        self.dacp.copy_(torch.tensor(dacp))

    def set_grad(self, G, ex=EX):
        g2 = np.concatenate([np.asarray(G, F) * F(2), ex])
        self.t["grad"][:len(g2)].copy_(torch.tensor(g2))

    def refresh_shadow(self):
        p = LIB.PREC_FP16 if self.precision == "fp16" else LIB.PREC_BF16
        LIB.check(LIB.lib().dad_refresh_shadow(self.st, p, self.step._stream()), "dad_refresh_shadow")

    def apply(self, cfg):
        LIB.check(LIB.lib().dad_step_apply(cfg, self.st, LIB.ptr(self.ws), self.step._stream()), "dad_step_apply")
        return self.read()

    def read(self):
        torch.cuda.synchronize()
        out = {k: v[:NP + LIB.DAD_GRAD_EXTRA].cpu().numpy() for k, v in self.t.items()}
        out = {k: (v if k == "grad" else v[:NP]) for k, v in out.items()}
        out["shadow_s"], out["shadow_t"] = self.shadow["student"].cpu().numpy(), self.shadow["teacher"].cpu().numpy()
        out["dacp"] = self.dacp.cpu().numpy()
        tail = self.tail.cpu().numpy()
        out["clip_norm"], out["clip_coef"] = tail[LIB.T_CLIPNORM], tail[LIB.T_CLIPCOEF]
        out["total"] = tail[LIB.T_TOTAL]
        out["range"] = int(tail[LIB.T_RANGE:LIB.T_RANGE + 1].view(np.int32)[0])
        out["losses"] = self.step._loss_vec.cpu().numpy()
        return out


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({2: np.int16, 4: np.int32}[a.dtype.itemsize])


def _same_bits(got, want, names, what=""):
    for k in names:
        np.testing.assert_array_equal(_bits(got[k]), _bits(want[k]), err_msg="%s %s" % (what, k))


STATE = ("student", "teacher", "exp_avg", "exp_avg_sq", "shadow_s", "shadow_t", "dacp")


def _host_shadow(w, dtype):
    """The shadow of a flat parameter vector: torch's CPU conversion (round to nearest even, subnormals
    kept) of W1[h][k] at frag_index(h, k)."""
    conv = torch.tensor(np.asarray(w[:R.NW1])).to(dtype).view(torch.int16).numpy()
    out = np.empty(R.NW1, np.int16)
    h, k = np.divmod(np.arange(R.NW1), R.D)
    out[R.frag_index(h, k)] = conv
    return out


_RUNS = {}


def _case_run(name, off=0):
    """The result of a case's apply (vector path, or off = 1: every float stream misaligned), once."""
    if (name, off) not in _RUNS:
        inp, kw = R.make_case(name)
        v = Vehicle(off=off)
        cfg = v.config(kw["t"], kw["lr"], kw["warmup"])
        assert (cfg.weight_decay, cfg.max_norm, cfg.ema_m) == (F(kw["weight_decay"]), F(kw["max_norm"]),
                                                              F(kw["ema_momentum"]))
        v.load(inp)
        v.refresh_shadow()
        _RUNS[name, off] = (v.read(), v.apply(cfg))
    return _RUNS[name, off]


def _check_against_reference(name, got, ref, bnd, norm=True):
    res = dict(m=got["exp_avg"], v=got["exp_avg_sq"], p=got["student"], teacher=got["teacher"],
               norm=float(got["clip_norm"]))
    w = R.worst(res, ref, bnd)
    print(name, "worst error / bound:", {k: "%.3f" % r for k, (_, r) in w.items()},
          "worst error in u:", {k: "%.3g" % x for k, x in R.worst_u(res, ref).items()})
    for k, (bad, ratio) in w.items():
        assert bad == 0, "%s: %d elements of %s out of bounds (worst %.3g x the bound)" % (name, bad, k, ratio)
    if norm:
        assert abs(res["norm"] - ref["norm"]) <= bnd["norm_rel"] * ref["norm"], (res["norm"], ref["norm"])


# ------------------------------------------------------------------ cases 1-5: against the reference
@pytest.mark.parametrize("name", sorted(R.CASES))
def test_apply_matches_the_float64_reference(name):
    inp, kw = R.make_case(name)
    ref, bnd = R.case_reference(name)
    before, got = _case_run(name)
    assert got["range"] == 0
    _check_against_reference(name, got, ref, bnd)
    if ref["clip_active"]:
        assert abs(float(got["clip_coef"]) - ref["coef"]) <= R.K_COEF * R.U * ref["coef"]
    else:
        assert got["clip_coef"] == F(1.0)
    # the 16-bit shadows (bf16 in an FP32 step) are the conversions of what the update wrote
    np.testing.assert_array_equal(got["shadow_s"], _host_shadow(got["student"], torch.bfloat16))
    np.testing.assert_array_equal(got["shadow_t"], _host_shadow(got["teacher"], torch.bfloat16))
    if kw["warmup"]:
        _same_bits(got, before, ("teacher", "shadow_t"), name)
        np.testing.assert_array_equal(got["shadow_t"], _host_shadow(inp["teacher"], torch.bfloat16))
    if name == "fresh":
        # weight decay alone moves the zero-gradient rows, by about lr sign(p)
        z = np.flatnonzero((inp["G"][:R.NW1] == 0) & (np.abs(inp["p"][:R.NW1]) >= 0.02))
        move = got["student"].astype(np.float64)[z] - inp["p"][z]
        np.testing.assert_allclose(move, -kw["lr"] * np.sign(inp["p"][z]), rtol=0.06)


# ------------------------------------------------------------------ case 6: averaging and DACP commit
def _expect_dacp(d, ex):
    """dacp_commit in float32, operation by operation (-ffp-contract=off)."""
    want = d.copy()
    want[0:4] = F(ALPHA) * d[0:4] + F(1 - ALPHA) * ex[0:4]
    want[8:12] = d[8:12] + ex[4:8]
    want[12:16] = d[12:16] + ex[8:12]
    return want


def test_apply_averages_the_exchange_buffer_and_commits_dacp():
    inp, kw = R.make_case("clip_active")
    before, got = _case_run("clip_active")
    np.testing.assert_array_equal(_bits(got["grad"][:NP]), _bits(inp["G"]))
    ex = got["grad"][NP:]
    np.testing.assert_array_equal(ex[0:4], EX[0:4] * F(0.5))
    np.testing.assert_array_equal(ex[12:16], EX[12:16] * F(0.5))
    np.testing.assert_array_equal(ex[4:12], EX[4:12])
    want = _expect_dacp(DACP0, ex)
    np.testing.assert_array_equal(_bits(got["dacp"]), _bits(want))
    # and against float64: alpha d + (1 - alpha) ex to 3 roundings per term
    d64 = ALPHA * DACP0[0:4].astype(np.float64) + (1 - ALPHA) * ex[0:4].astype(np.float64)
    assert (np.abs(got["dacp"][0:4] - d64) <= 3 * R.U * (ALPHA * DACP0[0:4] + (1 - ALPHA) * ex[0:4])).all()
    np.testing.assert_array_equal(got["dacp"][16:20], DACP0[16:20])
    np.testing.assert_array_equal(got["losses"], EX[12:16] * F(0.5))
    assert got["total"] == EX[12] * F(0.5)


@pytest.mark.parametrize("how", ["warmup", "use_dacp_0"])
def test_apply_leaves_dacp_alone(how):
    if how == "warmup":
        before, got = _case_run("warmup")
    else:
        inp, kw = R.make_case("clip_active")
        v = Vehicle()
        cfg = v.config(kw["t"], kw["lr"], use_dacp=0)
        v.load(inp)
        got = v.apply(cfg)
        _same_bits(got, _case_run("clip_active")[1], ("student", "teacher", "exp_avg", "exp_avg_sq"), how)
    np.testing.assert_array_equal(_bits(got["dacp"]), _bits(DACP0))
    np.testing.assert_array_equal(got["grad"][NP:NP + 4], EX[0:4] * F(0.5))      # still averaged


# ------------------------------------------------------------------ case 7: the scalar path
def test_unaligned_streams_take_the_scalar_path_to_the_same_bits():
    """Every float stream one float past a 16-byte boundary (the shadows stay aligned): dad_optim's
    `vec == false` branch, which compiles the same unfused expressions."""
    _, want = _case_run("clip_active")
    _, got = _case_run("clip_active", off=1)
    _same_bits(got, want, STATE + ("grad", "clip_norm", "clip_coef", "losses"), "scalar path")
    assert got["range"] == 0


# ------------------------------------------------------------------ case 8: shadow bytes
def _specials(kind):
    e = lambda k: F(2.0 ** k)
    v = [e(-15), e(-24), e(-25), F(1.5) * e(-25), F(1 + 2.0 ** -11), F(1 + 3 * 2.0 ** -11), F(65504.0),
         F(1 + 2.0 ** -8), F(1 + 3 * 2.0 ** -8), F(0.0), e(-14), F(1.0) - e(-12), e(-126), e(-133)]
    return np.array(v + [-x for x in v], F)


def _planted(seed):
    inp, _ = R.make_case("clip_active")
    rs = np.random.RandomState(seed)
    sp = _specials(None)
    out = {}
    for k in ("p", "teacher"):
        a = inp[k].copy()
        # every special at 8 places of W1: every residue of k mod 8 (both lanes of every packed pair)
        pos = rs.choice(R.NW1 // 8, size=len(sp), replace=False)
        for j in range(8):
            a[pos * 8 + j] = sp
        out[k] = a
    out["m"], out["G"] = np.zeros(NP, F), np.zeros(NP, F)
    out["v"] = inp["v"]
    return out


@pytest.mark.parametrize("precision", ["fp16", "bf16"])
def test_shadow_bytes_equal_the_host_conversion(precision):
    """Three writers (dad_pack2 in the vector path, dad_half_bits in the scalar path and in
    dad_shadow_kernel) against torch's CPU conversion, over all of W1, with the values where
    conversions differ planted in both signs: fp16 subnormals (2^-15, 2^-24), 2^-25 (a tie to zero),
    1.5 2^-25, round-to-even ties, 65504, the bf16 ties, +-0, float32 subnormals.  A zero step size in
    warm-up, a zero gradient and zero first moments leave p' = p and the teacher untouched, bit for bit."""
    inp = _planted(77)
    res = {}
    for off in (0, 1):
        v = Vehicle(precision, off=off)
        cfg = v.config(9, 5e-4, warmup=True, lr_step_size=0.0)
        v.load(inp)
        v.refresh_shadow()
        res["refresh", off] = v.read()
        for s in v.shadow.values():
            s.fill_(0x5a5a)
        res["apply", off] = v.apply(cfg)
    for (who, off), got in res.items():
        what = "%s %s off %d" % (precision, who, off)
        np.testing.assert_array_equal(_bits(got["student"]), _bits(inp["p"]), err_msg=what)
        np.testing.assert_array_equal(_bits(got["teacher"]), _bits(inp["teacher"]), err_msg=what)
        for k, src in (("shadow_s", "p"), ("shadow_t", "teacher")):
            want = _host_shadow(inp[src], TDT[precision])
            bad = np.flatnonzero(got[k] != want)
            h, kk = np.divmod(R.param_of_frag(bad[:8]), R.D)
            assert bad.size == 0, "%s %s: %d differ; W1[%s, %s] = %s: got %s want %s" % (
                what, k, bad.size, h, kk, inp[src][R.param_of_frag(bad[:8])], got[k][bad[:8]], want[bad[:8]])


# ------------------------------------------------------------------ case 9: non-finite gradient
@pytest.mark.parametrize("which", ["nan_in_w1", "inf_in_last_b2"])
def test_nonfinite_gradient_with_finite_loss_skips_the_update(which):
    """A NaN / inf gradient element under a finite total loss: norm = NaN gave coef = fminf(NaN, 1) = 1
    and Adam wrote NaN into everything, with no range bit.  The +inf sits in the partial last block
    (197,892 = 193 x 1024 + 260)."""
    inp, kw = R.make_case("clip_active")
    G = inp["G"].copy()
    if which == "nan_in_w1":
        G[123 * R.D + 457] = np.nan
    else:
        G[NP - 1] = np.inf
    v = Vehicle()
    cfg = v.config(kw["t"], kw["lr"])
    v.load(inp, G=G)
    v.refresh_shadow()
    before = v.read()
    assert np.isfinite(EX[12])
    got = v.apply(cfg)
    assert not np.isfinite(got["clip_norm"])
    assert got["range"] & LIB.RANGE_NONFINITE
    _same_bits(got, before, STATE, which)
    assert got["total"] == EX[12] * F(0.5)                     # the losses are still reported
    # a following finite apply is case 2, bit for bit
    v.tail[LIB.T_RANGE] = 0
    v.set_grad(inp["G"])
    again = v.apply(cfg)
    _same_bits(again, _case_run("clip_active")[1], STATE + ("grad", "clip_norm", "clip_coef"), which + ", next")
    assert again["range"] == 0


class _TwoEqualRanks:
    """Stands in for a DPComm of two ranks that computed the same gradient: the SUM all-reduce doubles
    the buffer.  dad_step_apply then averages it and takes the norm of what it averaged (dad_norm)."""
    world = 2

    def allreduce_grad(self, st, stream, grad=None):
        grad.mul_(2.0)


def test_step_with_a_nan_gradient_element_is_skipped_and_flagged():
    """The same through DADStep.step: the after_backward hook overwrites one gradient element between
    the exchange and the update.  (A step of world 1 takes its norm from the partials its backward
    wrote, before the hook runs; the norm that sees the hook's element is the data-parallel step's.)"""
    cfg = dad_oracle.make_cfg("iemocap")
    step = gh.make_step(cfg)
    step.comm = _TwoEqualRanks()
    gh.load_state(step, synth.make_state(3, 1))
    inp = _problem(B=4, T=20, seed=7)
    clean, noisy, draws = gh.batches(inp)
    state = lambda: [t.clone() for t in (step.model.student_flat.detach(), step.model.teacher_flat.detach(),
                                         step.exp_avg, step.exp_avg_sq, step.dacp,
                                         step.w1bf_student.view(torch.int16), step.w1bf_teacher.view(torch.int16))]
    before = state()

    def poison():
        step.grad[57 * 768 + 5] = float("nan")
    losses = step.step(clean, noisy, 60, draws=draws, after_backward=poison)
    torch.cuda.synchronize()
    assert all(np.isfinite(float(x)) for x in losses.values()), losses
    assert step.decode_range_flag(step.range_flag()) == ["nonfinite"]
    assert bool(torch.isfinite(step.model.student_flat).all()) and bool(torch.isfinite(step.model.teacher_flat).all())
    for a, b in zip(state(), before):
        assert torch.equal(a, b)


# ------------------------------------------------------------------ vehicle 2: the whole step
@pytest.mark.parametrize("precision", ["fp32", "fp16"])
def test_whole_step_update_matches_the_reference_on_its_own_gradient(precision):
    """B=5, T=33, Bn=7, Tn=31, epoch 60, dp_world = 1: the update and the clip norm against the
    reference evaluated on the device's own pre-clip gradient -- which ties the squared-norm partials
    (dad_reduce / dad_reduce_w and the extra blocks of the weight-gradient launch) to the gradient they
    describe."""
    cfg = dad_oracle.make_cfg("iemocap")
    st = synth.make_state(3, 1)
    step = gh.make_step(cfg, precision=precision)
    gh.load_state(step, st)
    o = gh.run_step(step, _problem(B=5, T=33, Bn=7, Tn=31), 60)
    assert int(step.range_flag()) == 0
    ref = R.reference_update(o["grad"], R.flat(st["student"]), R.flat(st["exp_avg"]), R.flat(st["exp_avg_sq"]),
                             R.flat(st["teacher"]), lr=dad_oracle.cosine_lr(cfg, 60), t=int(st["nstep"]) + 1,
                             weight_decay=cfg["WEIGHT_DECAY"], max_norm=cfg["MAX_GRAD_NORM"],
                             ema_momentum=cfg["EMA_MOMENTUM"], warmup=False)
    got = dict(student=R.flat(o["student"]), teacher=R.flat(o["teacher"]), exp_avg=R.flat(o["exp_avg"]),
               exp_avg_sq=R.flat(o["exp_avg_sq"]), clip_norm=o["clip_norm"])
    _check_against_reference("whole step " + precision, got, ref, R.bounds(ref))
    coef = float(o["clip_coef"])
    if ref["clip_active"]:
        assert abs(coef - ref["coef"]) <= R.K_COEF * R.U * ref["coef"]
    else:
        assert coef == 1.0
