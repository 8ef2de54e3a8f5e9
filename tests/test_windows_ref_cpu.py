"""dad_eval_windows without a GPU: the host layouts (evaluate.windows_host / window_frames / piece_frames)
against brute-force enumeration from the definitions, the float64 reference (tests/windows_ref.py) against the
reference model's golden numbers, wrong-answer controls for the GPU module's tolerances, the near-tie condition of
its prediction check, and the ctypes mirror of dad_window_args."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import dadpkg
import windows_ref as wr
from golden.gen_windows_golden import MODES as GOLDEN_MODES, inputs as golden_inputs
from oracle import data_oracle as do

PKG = dadpkg.pkg()
E = PKG.evaluate

LENGTHS = np.arange(201)
HOPS = [1, 5, 7, 8, 25, 31, 32, 33, 64, 100]
SPANS = [1, 2, 4]
GEOMETRY = [(h, m, mode) for h in HOPS for m in SPANS for mode in ("sliding", "prefix") if mode == "sliding" or m == 1]


@pytest.mark.parametrize("hop", HOPS)
def test_layouts_equal_brute_force(hop):
    pieces = [wr.pieces_brute(int(L), hop) for L in LENGTHS]
    poff = np.concatenate([[0], np.cumsum([len(p) for p in pieces])])
    for _, span, mode in [g for g in GEOMETRY if g[0] == hop]:
        win_off, piece_off = E.windows_host(LENGTHS, hop, span, mode)
        off, utt, st, en = wr.layout_brute(LENGTHS, hop, span, mode)
        assert win_off.dtype == np.int32 and piece_off.dtype == np.int32
        np.testing.assert_array_equal(win_off, off)
        np.testing.assert_array_equal(piece_off, poff)
        u2, s2, e2 = E.window_frames(LENGTHS, hop, span, mode)
        np.testing.assert_array_equal(u2, utt)
        np.testing.assert_array_equal(s2, st)
        np.testing.assert_array_equal(e2, en)
        # every last window ends at L; prefix ends increase strictly; no window is empty
        for L in LENGTHS:
            a, b = off[L], off[L + 1]
            assert (b - a == 0) == (L == 0)
            if b > a:
                assert en[b - 1] == L and (en[a:b] > st[a:b]).all()
                if mode == "prefix":
                    assert (st[a:b] == 0).all() and (np.diff(en[a:b]) > 0).all()
                else:
                    assert (st[a:b] == np.arange(b - a) * hop).all()
    pu, ps, pe = E.piece_frames(LENGTHS, hop)
    flat = [(L, a, b) for L, p in zip(LENGTHS, pieces) for a, b in p]
    np.testing.assert_array_equal(np.stack([pu, ps, pe], 1), np.array(flat, np.int64).reshape(-1, 3))
    # pieces partition [0, L), none crosses a slab or a hop boundary, and a slab holds at most
    # min(32, ceil(32 / hop) + 1) of them
    for L, p in zip(LENGTHS, pieces):
        assert [a for a, _ in p] == [0] * bool(p) + [b for _, b in p[:-1]] and (not p or p[-1][1] == L)
        assert all(a // 32 == (b - 1) // 32 and a // hop == (b - 1) // hop for a, b in p)
        per_slab = np.bincount([a // 32 for a, _ in p]) if p else np.zeros(1, int)
        assert per_slab.max() <= min(32, -(-32 // hop) + 1)


def test_layout_argument_errors():
    for bad in (dict(hop=0), dict(hop=8, span=0), dict(hop=8, span=2, mode="prefix"), dict(hop=8, mode="causal")):
        with pytest.raises(ValueError):
            E.windows_host([5, 6], **bad)
    with pytest.raises(ValueError, match="32 bits"):
        E.windows_host([2 ** 31 - 1] * 3, 1)


def test_reference_matches_the_reference_model_golden():
    """windows_ref's float64 forward against SSRLModel.predict on cropped features (tests/golden/eval_windows.npz,
    written by gen_windows_golden.py), at the 1e-4 the eval goldens use."""
    g = np.load(os.path.join(dadpkg.ROOT, "tests", "golden", "eval_windows.npz"))
    feats, sizes, offsets = golden_inputs()
    np.testing.assert_array_equal(g["sizes"], sizes)
    W1, b1, W2, b2 = do.eval_weights(int(g["seed"]))[0]
    hid = wr.hidden64(feats, W1, b1)
    for mode, (hop, span) in GOLDEN_MODES.items():
        assert tuple(g[mode + "_hop_span"]) == (hop, span)
        ref = wr.forward64(hid, sizes, offsets, np.arange(len(sizes)), W2, b2, hop, span, mode)
        np.testing.assert_allclose(ref["logits"], g[mode + "_logits"], rtol=1e-5, atol=1e-4)
        ok = ref["gap"] > wr.GAP
        assert ok.mean() >= 0.95
        np.testing.assert_array_equal(ref["pred"][ok], g[mode + "_pred"][ok])


def _close(a, b, rtol, atol):
    return bool(np.all(np.abs(a - b) <= atol + rtol * np.abs(b)))


@pytest.mark.parametrize("hop,span,mode", [(8, 4, "sliding"), (7, 3, "sliding"), (25, 1, "prefix")])
def test_wrong_references_violate_the_gpu_tolerances(hop, span, mode):
    """A window that ends one frame late and a mean over span * hop frames instead of the window's own count must
    each miss the tolerances test_gpu_windows holds the device to (rtol 1e-5, atol 1e-4 on embeddings and logits),
    and the second must differ only where a window is shorter than span * hop frames."""
    _, sizes, offsets, _, order = wr.main_inputs()
    _, _, W2, b2 = do.eval_weights(11)[0]
    hid = wr.main_hidden("f32", "s")
    ref = wr.main_reference("f32", "s", hop, span, mode)
    late = wr.forward64(hid, sizes, offsets, order, W2, b2, hop, span, mode, end_shift=1)
    flat = wr.forward64(hid, sizes, offsets, order, W2, b2, hop, span, mode, divide_by_span=True)
    for name, wrong in (("end + 1", late), ("/ (span * hop)", flat)):
        for key in ("emb", "logits"):
            assert not _close(wrong[key], ref[key], 1e-5, 1e-4), (name, key)
    full = ref["frames"] == span * hop
    assert full.any() and (~full).any()
    np.testing.assert_allclose(flat["emb"][full], ref["emb"][full], rtol=1e-12)
    assert not _close(flat["emb"][~full], ref["emb"][~full], 1e-5, 1e-4)


def test_near_ties_are_rare_and_predictions_move():
    """The GPU module compares predictions on windows whose reference top-two gap exceeds 2e-4; the filter may drop
    at most 5 % of a case's windows.  On the reference alone, both weight sets: and predictions change between
    windows in some utterance of most cases, so settle / switches are not trivially 0."""
    worst, moved = 0.0, 0
    for hop, span, mode in wr.MODE_CASES:
        for net in "st":
            ref = wr.main_reference("f32", net, hop, span, mode)
            ok = wr.decided(ref)
            worst = max(worst, float((~ok).mean()))
            off, pr = ref["win_off"], ref["pred"]
            moved += any(len(set(pr[off[u]:off[u + 1]])) > 1 for u in range(len(off) - 1))
    print("largest share of near-tie windows over the cases: %.4f" % worst)
    assert worst <= 0.05
    assert moved >= len(wr.MODE_CASES)


def test_summaries_and_block_on_a_hand_example():
    """windows_ref's NumPy restatement on a case small enough to check by hand."""
    L = PKG._lib
    win_off = np.array([0, 4, 4, 5, 8])
    w_pred = np.array([1, 2, 2, 1, 3, 0, 0, 0])
    w_probs = np.eye(4, dtype=np.float32)[w_pred]
    sizes = np.array([20, 0, 3, 13])
    s = wr.summaries(w_pred, w_probs, win_off, sizes, 5, 1, "prefix")
    np.testing.assert_array_equal(s["vote_pred"], [1, -1, 3, 0])       # 1 and 2 tie: the lower class
    np.testing.assert_array_equal(s["last_pred"], [1, -1, 3, 0])
    np.testing.assert_array_equal(s["settle"], [3, -1, 0, 0])
    np.testing.assert_array_equal(s["switches"], [2, -1, 0, 0])
    np.testing.assert_array_equal(s["settle_frames"], [20, 0, 3, 5])
    np.testing.assert_array_equal(s["mean_pred"], [1, -1, 3, 0])
    blk = wr.block(L, w_pred, s, win_off, np.array([1, 2, -1, 0]))
    assert (blk[L.EW_N], blk[L.EW_N_LABELLED], blk[L.EW_N_EMPTY], blk[L.EW_N_WINDOWS]) == (4, 3, 1, 8)
    np.testing.assert_array_equal(blk[L.EW_REACHED:L.EW_REACHED + 5], [2, 2, 2, 1, 0])
    np.testing.assert_array_equal(blk[L.EW_CORRECT:L.EW_CORRECT + 5], [2, 1, 1, 1, 0])
    np.testing.assert_array_equal(blk[L.EW_CARRIED:L.EW_CARRIED + 5], [2, 1, 1, 2, 2])
    assert blk[L.EW_CONF_LAST:L.EW_CONF_LAST + 16].reshape(4, 4)[1, 1] == 1
    assert (blk[L.EW_SETTLE_SUM], blk[L.EW_SWITCHES_SUM], blk[L.EW_SETTLE_FRAMES_SUM]) == (3, 2, 28)


def test_window_args_match_c_layout(tmp_path):
    """Compile a C probe against include/dad.h and compare sizeof / offsetof of dad_window_args with ctypes, and the
    DAD_EW_* / DAD_WIN_* numbers with the binding's."""
    L = PKG._lib
    cls = L.DadWindowArgs
    consts = {"DAD_WIN_SLIDING": L.WIN_SLIDING, "DAD_WIN_PREFIX": L.WIN_PREFIX, "DAD_EW_CONF_MEAN": L.EW_CONF_MEAN,
              "DAD_EW_CONF_VOTE": L.EW_CONF_VOTE, "DAD_EW_CONF_LAST": L.EW_CONF_LAST, "DAD_EW_N": L.EW_N,
              "DAD_EW_N_LABELLED": L.EW_N_LABELLED, "DAD_EW_N_EMPTY": L.EW_N_EMPTY, "DAD_EW_N_WINDOWS": L.EW_N_WINDOWS,
              "DAD_EW_N_NONFINITE": L.EW_N_NONFINITE, "DAD_EW_SETTLE_SUM": L.EW_SETTLE_SUM,
              "DAD_EW_SWITCHES_SUM": L.EW_SWITCHES_SUM, "DAD_EW_SETTLE_FRAMES_SUM": L.EW_SETTLE_FRAMES_SUM,
              "DAD_EW_CURVE": L.EW_CURVE, "DAD_EW_REACHED": L.EW_REACHED, "DAD_EW_CORRECT": L.EW_CORRECT,
              "DAD_EW_CARRIED": L.EW_CARRIED, "DAD_EW_SLOTS": L.EW_SLOTS}
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "dad.h"', "int main(void){",
             'printf("size %zu\\n", sizeof(dad_window_args));']
    for f in cls._fields_:
        lines.append('printf("%s %%zu\\n", offsetof(dad_window_args, %s));' % (f[0], f[0]))
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
