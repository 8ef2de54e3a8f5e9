"""What tests/test_gpu_hidden_state.py runs and tests/test_hidden_state_cpu.py checks (TEST INFRASTRUCTURE; no GPU
is needed to import this or to call anything but the functions marked GPU).

A train step must depend on nothing an earlier step left behind: not on the bytes of the workspace, whose regions
dad_ws_layout (csrc/dad_common.h) carves anew for every geometry, not on the per-(Bc, Bn) output buffers, not on
DADStep.grad.  The problems are exact_problem's (gates open, the mask mixed wherever Bn >= 7: KL, ECDA, eflag,
ge_ecda and the ecda scratch are live), plus G65 past the 64-utterance tables.

  UNITS      the four (precision, rng) pairs every part runs; EXPLICIT16: the 16-bit precisions on the problems'
             own draws, which part 1 adds because only a step on those draws can be held to the float64 reference
  SEQUENCE   part 2's (geometry index, epoch) steps through one DADStep; sequence_trace() replays DADStep._workspace
             on dad_workspace_bytes' answers and says which steps grew the buffer and which ran in bytes that a
             step of another layout wrote
  CHAIN      part 3's steps: (batch, epoch, batch named ahead or None, prepared?, named batch accepted?)
  poison_()  every byte of a tensor set to a pattern, but for the exempt words"""
import ctypes

import numpy as np

import dadpkg
import exact_problem as X

UNITS = {"fp32-explicit": ("fp32", "explicit"), "fp32-counter": ("fp32", "counter"),
         "fp16-counter": ("fp16", "counter"), "bf16-counter": ("bf16", "counter")}
EXPLICIT16 = {"fp16-explicit": ("fp16", "explicit"), "bf16-explicit": ("bf16", "explicit")}
ALL_UNITS = dict(UNITS, **EXPLICIT16)
EPOCHS = (0, 60)
# 0xFF: NaN in f32 and fp16, all ones as a flag or a counter.  0x01: a tiny normal f32 (2.4e-38), a non-zero flag,
# a counter of 16843009: what non-finite poison would hide behind a wrap-around or a `!= 0` test
PATTERNS = (0xFF, 0x01)
G65 = dict(B=65, T=8, Bn=65, Tn=8)        # test_gpu_store16's shape B: the general tail, dad_pool, dad_src_row
SCL = dict(TARGET_SCL_WEIGHT=1.0, SCL_START_EPOCH=0, SCL_TEMPERATURE=0.1)

# Part 2.  Geometry indices into exact_problem.GEOMS (G0 .. G4).  Step 3 grows the buffer (G4 is the largest layout
# in every precision); steps 4 .. 9 run without reallocation in bytes that steps of other layouts wrote; (5, 7)
# (G1) comes back at step 7 after (64, 64), (1, 2) and (12, 20); 0 -> 1 and 5 -> 6 are full -> warm-up and warm-up ->
# full at one geometry, 1 -> 2 and 8 -> 9 likewise; G0 (gates closed, Bn = 2) follows G4 with its gates open.
SEQUENCE = [(1, 60), (1, 0), (1, 60), (4, 60), (0, 60), (3, 0), (3, 60), (1, 60), (2, 0), (2, 60)]

# Part 3.  Batches: a, b, c of G1 (three problem seeds), p, q of G3.  (batch, epoch, named ahead, this step's rows
# were prepared by the last one, the library accepted the named batch).  Steps 2: another batch of the named one's
# geometry arrives; 2 -> 3 and 4 -> 5: the named batch has another geometry (test_gpu_prefetch.py's
# test_prefetch_refused_for_other_geometry); 5 -> 6: named in the warm-up (epoch 29), run at epoch 30.
CHAIN_BATCHES = {"a": (1, X.SEED), "b": (1, X.SEED + 1), "c": (1, X.SEED + 2), "p": (3, X.SEED), "q": (3, X.SEED + 1)}
CHAIN = [("a", 60, "b", False, True),
         ("b", 60, "a", True, True),
         ("c", 60, "p", False, False),
         ("p", 60, "q", False, True),
         ("q", 60, "a", True, False),
         ("a", 29, "b", False, False),
         ("b", 30, None, False, False)]
# the padded batch's tensors behind DADStep._prep_key's pointer list in counter mode (store mode: rowc, lenc, rown,
# lenn too; the draws' pointers are null in both)
PADDED_FIELDS = ("xc", "mc", "xn", "mn")


def geom(i):
    return G65 if i == 65 else X.GEOMS[i]


def cfg(scl=False):
    return dict(X.cfg(), **SCL) if scl else X.cfg()


def chain_problem(name):
    """(inputs, geometry) of chain batch `name`: exact_problem.problem at another seed for b, c and q."""
    gi, seed = CHAIN_BATCHES[name]
    g = dict(X.GEOMS[gi])
    ragged = g.pop("ragged", True)
    return X.problem(seed=seed, ragged=ragged, **g), X.GEOMS[gi]


def workspace_bytes(g, epoch, precision, scl=False):
    """dad_workspace_bytes of a step of geometry `g` (a host function: no GPU)."""
    p = dadpkg.pkg()
    c = p.dad_config_for(p.ConfigView(cfg(scl), flavor="iemocap"), g["B"], g["T"], g["Bn"], g["Tn"], epoch, 1,
                         precision={"fp32": p._lib.PREC_FP32, "fp16": p._lib.PREC_FP16, "bf16": p._lib.PREC_BF16}[precision])
    n = ctypes.c_size_t(0)
    assert p.lib().dad_workspace_bytes(c, ctypes.byref(n)) == 0
    return int(n.value)


def sequence_trace(precision, sequence=None):
    """DADStep._workspace replayed over `sequence`: per step dict(need, capacity, grew, inherited).  capacity: the
    buffer's bytes when the step runs; grew: the step allocated a larger one; inherited: it did not, and an earlier
    step of another geometry has written this buffer."""
    out, capacity, writers = [], 0, set()
    for gi, epoch in (SEQUENCE if sequence is None else sequence):
        need = workspace_bytes(geom(gi), epoch, precision)
        grew = need > capacity
        if grew:
            capacity, writers = need, set()
        out.append(dict(need=need, capacity=capacity, grew=grew, inherited=(not grew) and bool(writers - {gi})))
        writers.add(gi)
    return out


def poison_(t, byte, exempt=()):
    """Every byte of contiguous tensor `t` := `byte`, except the 4-byte words whose indices `exempt` lists."""
    import torch
    flat = t.view(-1)
    assert t.is_contiguous() and (flat.element_size() == 4 or not exempt)
    kept = [flat[i].clone() for i in exempt]
    flat.view(torch.uint8).fill_(byte)
    for i, v in zip(exempt, kept):
        flat[i] = v
    return t


def utterances(x, pad):
    """The frames of each utterance of a padded batch: [length, 768] arrays."""
    lens = (~pad).sum(1)
    return [x[b, :lens[b]] for b in range(len(lens))]


def store_layouts(inp, seed=0):
    """(clean, noisy) store layouts of one batch, test_gpu_store16._layout's: every utterance at an odd row with
    unrelated rows between; each (features, sizes, offsets, index)."""
    import test_gpu_store16 as S
    out = []
    for k, (x, pad) in enumerate(((inp["xc"], inp["mc"]), (inp["xn"], inp["mn"]))):
        utt = utterances(x, pad)
        f, s, o, idx = S._layout(np.random.RandomState(7100 + 2 * seed + k), [[len(u) for u in utt]], utterances=utt)
        out.append((f, s, o, idx[0]))
    return out
