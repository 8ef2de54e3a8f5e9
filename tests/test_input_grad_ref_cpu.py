"""tests/input_grad_ref.py without a GPU: the closed form against float64 autograd of the CPU model and against the
reference model's golden numbers, the exact grid's premises, every wrong variant failing the comparison the GPU test
makes, the caps holding for the reference's own float32 / fp16-operand restatements, the C layout of
dad_input_grad_args, the host argument checks and the Python-side validation."""
import ctypes
import functools
import os
import subprocess
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import dadpkg
import input_grad_ref as R
from golden.gen_input_grad_golden import EPS as GOLDEN_EPS, GRAD_OF, inputs as golden_inputs
from oracle import data_oracle as do
from oracle.torch_cpu import TorchCPUStep

GOLDEN = os.path.join(dadpkg.ROOT, "tests", "golden", "eval_input_grad.npz")


@functools.lru_cache(None)
def fixture():
    """The random fixture: (feats, sizes, offsets, labels, params, dz float32 [7, 4], float64 reference)."""
    feats, sizes, offsets, labels = golden_inputs()
    params = do.eval_weights(23)[0]
    dz = R.ce_dz(R.forward64(feats, sizes, offsets, params), labels).astype(np.float32)
    return feats, sizes, offsets, labels, params, dz, R.reference(feats, sizes, offsets, params, dz)


def test_closed_form_equals_float64_autograd_and_the_golden():
    feats, sizes, offsets, labels, params, _, _ = fixture()
    W1, b1, W2, b2 = (torch.from_numpy(np.asarray(p, np.float64)) for p in params)
    z64 = R.forward64(feats, sizes, offsets, params)
    ref = R.reference(feats, sizes, offsets, params, R.ce_dz(z64, labels))
    g = np.load(GOLDEN)
    soff = R.slab_prefix(sizes)
    np.testing.assert_array_equal(g["sizes"], sizes)
    for i, (o, L) in enumerate(zip(offsets, sizes)):
        if L == 0:
            continue
        x = torch.from_numpy(feats[o:o + L].astype(np.float64))[None].requires_grad_(True)
        z = F.linear(TorchCPUStep.encode(x, torch.zeros(1, L, dtype=torch.bool), W1, b1), W2, b2)
        G, = torch.autograd.grad(F.cross_entropy(z, torch.tensor([labels[i]])), x)
        G = G.numpy()[0]
        mine = ref["grad"][32 * soff[i]:32 * soff[i] + L]
        assert np.abs(mine - G).max() <= 1e-12 * np.abs(G).max()
        np.testing.assert_allclose(z.detach().numpy()[0], z64[i], rtol=1e-12, atol=1e-12)
        # the reference model (float32 autograd): signs wherever the gradient is not at float32's noise level
        big = np.abs(G) > 1e-5 * np.abs(G).max()
        np.testing.assert_array_equal(g["sign"][o:o + L][big], np.sign(G)[big].astype(np.int8))
        assert big.mean() > 0.999
        if i in GRAD_OF:
            np.testing.assert_allclose(g["grad_%d" % i], G, rtol=1e-3, atol=1e-5 * np.abs(G).max())
    # its logits and losses at x + eps * (its own signs)
    for k, e in enumerate(GOLDEN_EPS):
        assert g["eps"][k] == e
        d = R.to_explicit(np.float32(e) * g["sign"].astype(np.float32), sizes, offsets)
        zk = R.forward64(feats, sizes, offsets, params, d)
        np.testing.assert_allclose(g["logits"][k][1:], zk[1:], rtol=1e-5, atol=1e-4)
        np.testing.assert_allclose(g["loss"][k][1:], R.ce_loss(zk, labels)[1:], rtol=1e-4, atol=1e-5)
        assert (g["loss"][k][1:] > g["loss0"][1:]).all()          # the direction ascends


def _sum_in_order(m, g, W1, order):
    """G in float32, hidden units accumulated one at a time in `order`"""
    acc = np.zeros((m.shape[0], W1.shape[1]), np.float32)
    for j in order:
        acc = acc + np.where(m[:, j:j + 1], np.float32(g[j]), np.float32(0)) * W1[j].astype(np.float32)[None, :]
    return acc


def test_exact_grid_premises():
    feats, sizes, offsets, params, dz, delta = R.exact_problem(R.EXACT_POW2 + R.EXACT_ODD)
    W1, b1, W2, b2 = params
    odd = lambda a, step: (np.round(np.asarray(a, np.float64) / step) == np.asarray(a, np.float64) / step).all() and \
        (np.round(np.asarray(a, np.float64) / step).astype(np.int64) % 2 == 1).all()
    mult = lambda a, step: (np.round(np.asarray(a, np.float64) / step) * step == np.asarray(a, np.float64)).all()
    assert odd(b1, 2.0 ** -14)
    assert mult(feats, 2.0 ** -3) and np.abs(feats).max() < 17
    assert mult(W1, 2.0 ** -10) and np.abs(W1).max() < 0.05
    assert mult(W2, 2.0 ** -4) and np.abs(W2).max() <= 0.5
    assert mult(dz, 2.0 ** -2) and mult(delta, 2.0 ** -3) and np.abs(delta).max() <= 1
    for a in (feats, W1):                                    # exact in fp16 too, with delta added
        assert np.array_equal(R.f16(a), np.asarray(a, np.float64))
    soff = R.slab_prefix(sizes)
    zeros = 0
    for dl in (None, delta):
        ref = R.reference(feats, sizes, offsets, params, dz, dl)
        for i, (o, L) in enumerate(zip(offsets, sizes)):
            r0 = 32 * soff[i]
            x = feats[o:o + L].astype(np.float64) + (0 if dl is None else dl[r0:r0 + L])
            assert np.array_equal(R.f16(x), x)
            pre = x @ np.asarray(W1, np.float64).T + np.asarray(b1, np.float64)
            assert odd(pre, 2.0 ** -14)                      # never 0: the mask is the same in every precision
            assert np.array_equal(pre.astype(np.float32).astype(np.float64), pre)
            if L not in R.EXACT_POW2:
                continue
            m = pre > 0
            g = (np.asarray(W2, np.float64).T @ dz[i]) / L
            want = ref["grad"][r0:r0 + L]
            assert np.array_equal(want.astype(np.float32).astype(np.float64), want)
            rs = np.random.RandomState(int(L))
            for order in (np.arange(R.H), np.arange(R.H)[::-1], rs.permutation(R.H)):
                assert np.array_equal(_sum_in_order(m, g, W1, order).astype(np.float64), want)
            zeros += int((want == 0).sum())
    assert zeros >= 1                                        # sgn(0) is exercised
    # the fp16-operand restatement is exact on the power-of-two lengths as well
    p2 = R.exact_problem(R.EXACT_POW2)
    assert np.array_equal(R.reference(*p2[:5], p2[5], fp16_operands=True)["grad"], R.reference(*p2[:5], p2[5])["grad"])
    assert np.array_equal(R.reference(*p2[:5], p2[5], dtype=np.float32)["grad"], R.reference(*p2[:5], p2[5])["grad"])


def test_every_variant_fails_the_gpu_comparison():
    # the exact grid: bits of grad or step, or a non-zero row past a length
    feats, sizes, offsets, params, dz, delta = R.exact_problem(R.EXACT_POW2 + R.EXACT_ODD)
    kw = dict(delta=delta, alpha=0.25, radius=0.5)
    ref = R.reference(feats, sizes, offsets, params, dz, **kw)
    assert not R.exact_failures(ref, ref, sizes)
    for v in R.VARIANTS:
        bad = R.reference(feats, sizes, offsets, params, dz, variant=v, **kw)
        assert R.exact_failures(bad, ref, sizes), v
    # the random fixture: ten times outside the bound (the three variants that leave G alone are the exact grid's)
    feats, sizes, offsets, labels, params, dz, _ = fixture()
    delta = R.to_explicit(0.25 * np.sign(np.random.RandomState(3).standard_normal(feats.shape)), sizes, offsets)
    ref = R.reference(feats, sizes, offsets, params, dz, delta)
    for v in ("relu_ignored", "no_len_division", "mask_at_x", "w1_tile_transposed"):
        bad = R.reference(feats, sizes, offsets, params, dz, delta, variant=v)
        ratio, _, _ = R.check_grad(bad["grad"], ref, sizes, flips=True)
        assert ratio >= 10.0, (v, ratio)
    bad = R.reference(feats, sizes, offsets, params, dz, delta, variant="rows_past_len")
    assert np.abs(bad["grad"][~R.valid_rows(sizes)]).max() > 0


def test_caps_hold_for_the_reference_restatements():
    feats, sizes, offsets, labels, params, dz, ref = fixture()
    f32 = R.reference(feats, sizes, offsets, params, dz, dtype=np.float32)
    ratio, bad, unchecked = R.check_grad(f32["grad"], ref, sizes, flips=True)
    print("float32 restatement: worst error / bound %.3f, %d sign mismatches, %.2f %% unchecked (%d flip-prone units in "
          "%d of %d frames)" % (ratio, bad, 100 * unchecked, ref["n_flip_units"], ref["flip_frames"], sizes.sum()))
    assert ratio <= 1.0 and bad == 0 and unchecked <= 0.015
    assert R.sign_disagreement(f32["grad"], ref, sizes) <= 0.0005
    h = R.reference(feats, sizes, offsets, params, dz, fp16_operands=True)
    dis = R.sign_disagreement(h["grad"], ref, sizes)
    print("fp16-operand restatement: sign disagreement %.3f %%" % (100 * dis))
    assert dis <= 0.005
    # frame_l1 and the counts of the reference itself
    assert ref["counts"][0] == sizes.sum() and ref["counts"][1] == 0


def test_ctypes_struct_matches_c_layout(tmp_path):
    p = dadpkg.pkg()
    cname, cls = "dad_input_grad_args", p._lib.DadInputGradArgs
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "dad.h"', "int main(void){",
             'printf("%s %%zu\\n", sizeof(%s));' % (cname, cname)]
    for f in cls._fields_:
        lines.append('printf("%s.%s %%zu\\n", offsetof(%s, %s));' % (cname, f[0], cname, f[0]))
    lines.append('printf("counts %d %d %d %d\\n", DAD_IG_FRAMES, DAD_IG_NONFINITE, DAD_IG_ZERO, DAD_IG_COUNTS);')
    lines.append("return 0;}")
    c = tmp_path / "probe.c"
    c.write_text("\n".join(lines))
    exe = tmp_path / "probe"
    subprocess.check_call(["gcc", "-I", os.path.join(dadpkg.ROOT, "include"), str(c), "-o", str(exe)])
    rows = [l.split() for l in subprocess.check_output([str(exe)]).decode().splitlines()]
    out = {r[0]: r[1:] for r in rows}
    assert int(out[cname][0]) == ctypes.sizeof(cls)
    for f in cls._fields_:
        assert int(out["%s.%s" % (cname, f[0])][0]) == getattr(cls, f[0]).offset, f[0]
    L = p._lib
    assert [int(v) for v in out["counts"]] == [L.IG_FRAMES, L.IG_NONFINITE, L.IG_ZERO, L.IG_COUNTS]


def test_host_argument_checks_need_no_device():
    p = dadpkg.pkg()
    p.build(verbose=False)
    L, lib = p._lib, p.lib()
    fn = L.require("dad_input_grad", "the input gradients")
    size = L.require("dad_input_grad_workspace_bytes", "the input gradients")
    assert size(0, 0, L.PREC_FP32) == 0 and size(7, -1, L.PREC_FP32) == 0 and size(1, (1 << 26) + 1, L.PREC_FP32) == 0
    assert size(7, 8, L.PREC_FP32) == 256
    assert size(7, 8, L.PREC_FP16) == 2 * 2 * 256 * 768
    fake = 4096                      # never dereferenced: every call below fails its checks before a launch

    def args(**over):
        a = L.DadInputGradArgs()
        for name in ("store", "rows", "lens", "slab_off", "params", "dz", "counts"):
            setattr(a, name, fake)
        a.n, a.slabs, a.alpha, a.radius = 7, 8, 0.5, float("inf")
        a.store_dtype, a.precision = L.STORE_F32, L.PREC_FP32
        for k, v in over.items():
            setattr(a, k, v)
        return a

    assert fn(None, fake, None) == L.E_ARG
    assert fn(args(), None, None) == L.E_ARG
    for name in ("store", "rows", "lens", "slab_off", "params", "dz", "counts"):
        assert fn(args(**{name: None}), fake, None) == L.E_ARG, name
    assert fn(args(store_dtype=3), fake, None) == L.E_ARG
    assert fn(args(precision=7), fake, None) == L.E_ARG
    for alpha in (float("inf"), float("nan")):
        assert fn(args(alpha=alpha), fake, None) == L.E_ARG
    for radius in (-0.125, float("nan")):
        assert fn(args(radius=radius), fake, None) == L.E_ARG
    assert fn(args(precision=L.PREC_BF16), fake, None) == L.E_UNSUPPORTED
    assert fn(args(n=0), fake, None) == L.E_SHAPE
    assert fn(args(slabs=-1), fake, None) == L.E_SHAPE
    assert fn(args(n=1, slabs=(1 << 26) + 1), fake, None) == L.E_SHAPE
    assert sorted(n for n in L.EXPORTS if "input_grad" in n) == ["dad_input_grad", "dad_input_grad_workspace_bytes"]
    assert "dad_input_grad" in L.OPTIONAL_EXPORTS


def test_python_side_validation_raises_value_error():
    E = dadpkg.pkg().evaluate
    unlabelled = types.SimpleNamespace(labels_d=None)
    with pytest.raises(ValueError, match="unknown target"):
        E._adv_check(unlabelled, "loss")
    with pytest.raises(ValueError, match="no labels"):
        E._adv_check(unlabelled, "label")
    E._adv_check(unlabelled, "pred")
    with pytest.raises(ValueError, match="between 1 and 7"):
        E._adv_epsilons([0.01] * 8)
    with pytest.raises(ValueError, match="between 1 and 7"):
        E._adv_epsilons([])
    for bad in ([-0.1], [float("nan")], [float("inf")]):
        with pytest.raises(ValueError, match="finite"):
            E._adv_epsilons(bad)
    assert E._adv_epsilons((0.01, 0.05)) == [0.01, 0.05]
    for name in ("enqueue_input_grad", "input_gradients", "evaluate_adversarial_store", "adversarial_response_curve",
                 "worst_case_report"):
        assert getattr(dadpkg.pkg(), name) is getattr(E, name)
