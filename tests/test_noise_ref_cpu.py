"""dad_eval_noise without a GPU: the float64 reference (tests/noise_ref.py) against the reference model's golden
numbers, the ctypes mirror of dad_noise_args and the DAD_EN_* slots, the host validation of the entry points,
wrong-answer controls for the GPU module's tolerances, and the near-tie condition of its prediction check."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import dadpkg
import noise_ref as nr
from golden.gen_noise_golden import SIGMAS as GOLDEN_SIGMAS, inputs as golden_inputs, slab_aligned
from oracle import data_oracle as do

PKG = dadpkg.pkg()
E = PKG.evaluate
L_ = PKG._lib

CASES = [(net, sig) for net in "st" for sig in (nr.LEVELS4, nr.LEVELS8)]       # test_gpu_noise's float64 cases


def _close(a, b, rtol, atol):
    return bool(np.all(np.abs(a - b) <= atol + rtol * np.abs(b)))


def test_reference_matches_the_reference_model_golden():
    """noise_ref's float64 forward against SSRLModel.get_embeddings / predict on x + sigma n
    (tests/golden/eval_noise.npz, written by gen_noise_golden.py), at the 1e-4 the eval goldens use."""
    g = np.load(os.path.join(dadpkg.ROOT, "tests", "golden", "eval_noise.npz"))
    feats, noise, sizes, offsets = golden_inputs()
    np.testing.assert_array_equal(g["sizes"], sizes)
    np.testing.assert_array_equal(g["sigmas"], GOLDEN_SIGMAS)
    assert sizes.min() == 0 and sizes.max() == 65 and len(sizes) == 7 and len(GOLDEN_SIGMAS) == 4
    ref = nr.forward64(feats, slab_aligned(noise, sizes, offsets), sizes, offsets, np.arange(len(sizes)),
                       GOLDEN_SIGMAS, do.eval_weights(int(g["seed"]))[0])
    np.testing.assert_allclose(ref["emb"], g["emb"], rtol=1e-5, atol=1e-4)
    np.testing.assert_allclose(ref["logits"], g["logits"], rtol=1e-5, atol=1e-4)
    ok = ref["gap"] > nr.GAP
    assert ok.mean() >= 0.95
    np.testing.assert_array_equal(ref["pred"][ok], g["pred"][ok])
    assert not ref["emb"][:, 0].any() and (ref["drift"][0] == 0).all() and (ref["kl"][0] == 0).all()


def test_noise_args_match_c_layout(tmp_path):
    """Compile a C probe against include/dad.h and compare sizeof / offsetof of dad_noise_args with ctypes, and the
    DAD_EN_* numbers with the binding's."""
    cls = L_.DadNoiseArgs
    consts = {"DAD_EN_MAX_LEVELS": L_.EN_MAX_LEVELS, "DAD_EN_CONF": L_.EN_CONF, "DAD_EN_FLIPS": L_.EN_FLIPS,
              "DAD_EN_SURVIVE": L_.EN_SURVIVE, "DAD_EN_N": L_.EN_N, "DAD_EN_N_LABELLED": L_.EN_N_LABELLED,
              "DAD_EN_N_SKIPPED": L_.EN_N_SKIPPED, "DAD_EN_N_NONFINITE": L_.EN_N_NONFINITE,
              "DAD_EN_LEVELS": L_.EN_LEVELS, "DAD_EN_COUNTS": L_.EN_COUNTS, "DAD_EN_SUM_SCORE": L_.EN_SUM_SCORE,
              "DAD_EN_SUM_DRIFT": L_.EN_SUM_DRIFT, "DAD_EN_SUM_KL": L_.EN_SUM_KL, "DAD_EN_SUMS": L_.EN_SUMS}
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "dad.h"', "int main(void){",
             'printf("size %zu\\n", sizeof(dad_noise_args));']
    for f in cls._fields_:
        lines.append('printf("%s %%zu\\n", offsetof(dad_noise_args, %s));' % (f[0], f[0]))
    for name in consts:
        lines.append('printf("%s %%d\\n", (int)%s);' % (name, name))
    lines.append("return 0;}")
    c = tmp_path / "probe.c"
    c.write_text("\n".join(lines))
    exe = tmp_path / "probe"
    subprocess.check_call(["gcc", "-I", os.path.join(dadpkg.ROOT, "include"), str(c), "-o", str(exe)])
    out = dict(l.split() for l in subprocess.check_output([str(exe)]).decode().splitlines())
    assert int(out["size"]) == ctypes.sizeof(cls)
    for f in cls._fields_:
        assert int(out[f[0]]) == getattr(cls, f[0]).offset, f[0]
    for name, v in consts.items():
        assert int(out[name]) == v, name
    # the slots do not overlap: 8 confusion matrices, two [8] rows, five scalars; three [8] rows of sums
    assert L_.EN_FLIPS == L_.EN_CONF + 16 * L_.EN_MAX_LEVELS and L_.EN_SURVIVE == L_.EN_FLIPS + L_.EN_MAX_LEVELS
    assert L_.EN_N == L_.EN_SURVIVE + L_.EN_MAX_LEVELS and L_.EN_LEVELS < L_.EN_COUNTS
    assert L_.EN_SUMS == 3 * L_.EN_MAX_LEVELS


def test_exports_are_listed():
    for name in ("dad_eval_noise_workspace_bytes", "dad_eval_noise", "dad_eval_noise_draws"):
        assert name in L_.EXPORTS and name in L_.OPTIONAL_EXPORTS
        assert hasattr(L_.lib(), name)
    assert "eval_noise.hip" in PKG._build.SOURCES
    for name in ("noise_draws", "enqueue_eval_noise", "evaluate_noise_store", "noise_response_curve",
                 "robustness_report"):
        assert callable(getattr(PKG, name))


def _host_args(**change):
    """Arguments that pass every pointer check with made-up addresses: only error paths may be called with them."""
    a = L_.DadNoiseArgs()
    for name in ("store", "rows", "lens", "slab_off", "params", "counts", "sums"):
        setattr(a, name, 0x1000)
    a.n, a.slabs, a.levels = 39, 70, 4
    a.sigma[:4] = [0.0, 0.01, 0.05, 0.25]
    a.store_dtype, a.use_entropy, a.precision = L_.STORE_F32, 1, L_.PREC_FP32
    for k, v in change.items():
        if k.startswith("sigma"):
            a.sigma[int(k[5:])] = v
        else:
            setattr(a, k, v)
    return a


def test_host_validation_needs_no_gpu():
    """Every listed error returns its code before anything is launched: these calls run where there is no GPU."""
    fn = L_.lib().dad_eval_noise
    ws = ctypes.c_void_p(0x1000)
    call = lambda **change: fn(_host_args(**change), ws, None)
    for name in ("store", "rows", "lens", "slab_off", "params", "counts", "sums"):
        assert call(**{name: None}) == L_.E_ARG, name
    assert fn(_host_args(), None, None) == L_.E_ARG
    assert fn(None, ws, None) == L_.E_ARG
    for levels in (0, -1, 9):
        assert call(levels=levels) == L_.E_ARG
    for bad in (-0.5, float("nan"), float("inf"), -float("inf")):
        assert call(sigma2=bad) == L_.E_ARG
        assert call(sigma0=bad) == L_.E_ARG
    assert call(store_dtype=3) == L_.E_ARG
    assert call(precision=3) == L_.E_ARG
    assert call(precision=L_.PREC_BF16) == L_.E_UNSUPPORTED
    assert call(n=0) == L_.E_SHAPE
    assert call(slabs=-1) == L_.E_SHAPE
    assert call(n=1, slabs=2 ** 26 + 1) == L_.E_SHAPE
    assert call(n=2 ** 20, slabs=2 ** 21, levels=4) == L_.E_SHAPE          # 2^21 * 4 * 256 = 2^31
    assert call(n=2 ** 20, slabs=2 ** 23, levels=1, sigma0=0.0) == L_.E_SHAPE
    # a sigma beyond `levels` is not read
    assert call(sigma5=float("nan"), n=0) == L_.E_SHAPE
    probe = L_.lib().dad_eval_noise_draws
    out = ctypes.c_void_p(0x1000)
    assert probe(None, out, None) == L_.E_ARG
    assert probe(_host_args(), None, None) == L_.E_ARG
    assert probe(_host_args(lens=None), out, None) == L_.E_ARG
    assert probe(_host_args(slab_off=None), out, None) == L_.E_ARG
    assert probe(_host_args(n=0), out, None) == L_.E_SHAPE
    assert probe(_host_args(n=2 ** 20, slabs=2 ** 23), out, None) == L_.E_SHAPE
    wsb = L_.lib().dad_eval_noise_workspace_bytes
    assert wsb(39, 70, 4, L_.PREC_FP32) >= 70 * 4 * 1024
    assert wsb(39, 70, 4, L_.PREC_FP16) == wsb(39, 70, 4, L_.PREC_FP32) + 2 * 256 * 768
    for n, slabs, levels in ((0, 0, 1), (39, -1, 1), (39, 70, 0), (39, 70, 9), (1, 2 ** 26 + 1, 1),
                             (2 ** 20, 2 ** 21, 4), (2 ** 20, 2 ** 20, 8)):
        assert wsb(n, slabs, levels, L_.PREC_FP32) == 0, (n, slabs, levels)
    assert wsb(2 ** 20, 2 ** 21 - 1, 4, L_.PREC_FP32) > 0
    # the workspace grows as slabs x K x 1 KB
    assert wsb(39, 1070, 8, 0) - wsb(39, 70, 8, 0) == 1000 * 8 * 1024
    with pytest.raises(ValueError):
        E._noise_sigmas([])
    with pytest.raises(ValueError):
        E._noise_sigmas([0.0] * 9)
    with pytest.raises(ValueError):
        E._noise_sigmas([0.0, -1.0])


@pytest.mark.parametrize("variant", nr.VARIANTS)
def test_wrong_references_violate_the_gpu_tolerances(variant):
    """Each wrong reference misses the tolerances test_gpu_noise holds the device to on its float64 cases (both
    networks, LEVELS4 and LEVELS8): the first four the embedding and logit tolerance (rtol 1e-5, atol 1e-4) on every
    case, the swapped KL the derived kl bound.  KL(p0 | pk) and KL(pk | p0) agree to second order, so the swap shows
    only where kl is large against the bound: on the teacher and on LEVELS8's large levels, not on the student's
    four small levels (asserted too, so the statement stays true)."""
    for net, sig in CASES:
        ref = nr.main_reference("f32", net, sig)
        wrong = nr.main_reference("f32", net, sig, False, variant)
        if variant == "kl_swapped":
            assert _close(wrong["emb"], ref["emb"], 0, 0)
            caught = bool(np.any(np.abs(wrong["kl"] - ref["kl"]) > ref["kl_lim"]))
            assert caught == ((net, sig) != ("s", nr.LEVELS4)), (net, sig)
        else:
            for key in ("emb", "logits"):
                assert not _close(wrong[key], ref[key], 1e-5, 1e-4), (variant, net, key)
            assert np.any(np.abs(wrong["drift"] - ref["drift"]) > nr.drift_lim(ref["emb"]))


def test_near_ties_are_rare_and_predictions_move():
    """The GPU module compares predictions on (utterance, level) cells whose reference top-two gap exceeds GAP; the
    filter may drop at most 5 % of a case's cells.  On the reference alone, for the seeds chosen: and in every case
    some prediction at the top level differs from level 0's, so flips / break_level / survive are not trivial."""
    worst = 0.0
    for dt, fp16 in (("f32", False), ("f16", False), ("bf16", False), ("f32", True)):
        for net, sig in CASES:
            ref = nr.main_reference(dt, net, sig, fp16)
            worst = max(worst, float((~nr.decided(ref)).mean()))
            assert (ref["pred"][-1] != ref["pred"][0]).any(), (dt, net, len(sig))
            assert (ref["break_level"] < len(sig)).any() and (ref["break_level"] == len(sig)).any()
    print("largest share of near-tie cells over the cases: %.4f" % worst)
    assert worst <= 0.05


def test_block_on_a_hand_example():
    pred = np.array([[0, 1, 2, 3], [0, 1, 1, 3], [1, 1, 2, 3]])
    one = np.ones((3, 4), np.float32)
    counts, sums = nr.block(L_, pred, one, 2 * one, 3 * one, np.array([0, 1, -1, 3]))
    np.testing.assert_array_equal(nr.break_level(pred), [2, 3, 1, 3])
    np.testing.assert_array_equal(counts[L_.EN_FLIPS:L_.EN_FLIPS + 3], [0, 1, 1])
    np.testing.assert_array_equal(counts[L_.EN_SURVIVE:L_.EN_SURVIVE + 4], [4, 3, 2, 0])
    assert (counts[L_.EN_N], counts[L_.EN_N_LABELLED], counts[L_.EN_N_SKIPPED], counts[L_.EN_LEVELS]) == (4, 3, 1, 3)
    cm2 = counts[L_.EN_CONF + 32:L_.EN_CONF + 48].reshape(4, 4)
    assert cm2[0, 1] == 1 and cm2[1, 1] == 1 and cm2[3, 3] == 1 and cm2.sum() == 3
    np.testing.assert_array_equal(sums[L_.EN_SUM_DRIFT:L_.EN_SUM_DRIFT + 4], [8, 8, 8, 0])
    assert not counts[L_.EN_CONF + 48:L_.EN_FLIPS].any()


def test_default_levels_read_the_config_at_call_time():
    assert E.default_noise_levels() == (0.0, PKG.FLAVOR_DEFAULTS["iemocap"]["WEAK_NOISE_STD"],
                                        PKG.FLAVOR_DEFAULTS["iemocap"]["STRONG_NOISE_STD"])
    view = PKG.ConfigView(flavor="iemocap", WEAK_NOISE_STD=0.02, STRONG_NOISE_STD=0.1)
    assert E.default_noise_levels(view) == (0.0, 0.02, 0.1)
