"""The conditions tests/test_gpu_hidden_state.py relies on, checked without a GPU (tests/hidden_state.py): part 2's
sequence really reuses, grows and revisits what it claims (by dad_workspace_bytes, a host function), the poison
leaves the exempt words alone, part 3's "other batch" differs from the named one in every tensor the row
preparation's key holds and in content, and every problem's mask has the property its part relies on."""
import numpy as np
import pytest
import torch

import dadpkg
import exact_problem as X
import gpu_harness as gh
import hidden_state as H
import test_exact_problem_cpu as C

LIB = dadpkg.pkg()._lib


# ------------------------------------------------------------------ part 2: the sequence
@pytest.mark.parametrize("precision", ["fp32", "fp16", "bf16"])
def test_sequence_reuses_grows_and_revisits(precision):
    seq, tr = H.SEQUENCE, H.sequence_trace(precision)
    print(precision, [(t["need"], t["capacity"], t["grew"], t["inherited"]) for t in tr])
    assert len(seq) >= 7 and {e for _, e in seq} == {0, 60} and {g for g, _ in seq} == {0, 1, 2, 3, 4}
    assert sum(t["inherited"] for t in tr) >= 4
    assert any(t["grew"] for t in tr[1:])
    # an inherited step's regions really lie elsewhere than the writer's: the layouts differ in size
    for k, t in enumerate(tr):
        if t["inherited"]:
            assert any(tr[j]["need"] != t["need"] for j in range(k)), k
    pairs = [(X.GEOMS[g]["B"], X.GEOMS[g]["Bn"]) for g, _ in seq]
    assert any(pairs[k] in pairs[:k - 1] and pairs[k] != pairs[k - 1] for k in range(2, len(seq)))
    steps = list(zip(seq, seq[1:]))
    assert any(a[0] == b[0] and a[1] >= 30 and b[1] < 30 for a, b in steps)       # warm-up after full
    assert any(a[0] == b[0] and a[1] < 30 and b[1] >= 30 for a, b in steps)       # full after warm-up
    assert any(b == (0, 60) and a[1] >= 30 and X.GEOMS[a[0]]["Bn"] >= 7 for a, b in steps)   # G0 after open gates
    # the warm-up flag is part of the workspace key but not of the layout
    for g in X.GEOMS + [H.G65]:
        assert H.workspace_bytes(g, 0, precision) == H.workspace_bytes(g, 60, precision)
        assert H.workspace_bytes(g, 60, precision, scl=True) > H.workspace_bytes(g, 60, precision)


def test_chain_script_is_consistent():
    """Part 3's expectations follow from its own script: a step's rows were prepared iff the step before named
    exactly this batch at this epoch's warm-up flag and the library accepted it; it accepts iff the named batch has
    this step's geometry and the step is past the warm-up (plan_step: only dad_tail_ecda_w prepares ahead)."""
    prev = None
    for name, epoch, named, prepped, accepted in H.CHAIN:
        same_geom = named is not None and H.CHAIN_BATCHES[named][0] == H.CHAIN_BATCHES[name][0]
        assert accepted == (same_geom and epoch >= 30), name
        assert prepped == (prev is not None and prev[4] and prev[2] == name and (prev[1] < 30) == (epoch < 30)), name
        prev = (name, epoch, named, prepped, accepted)
    kinds = [(p[2] == n[0], p[4], n[3]) for p, n in zip(H.CHAIN, H.CHAIN[1:])]
    assert (True, True, True) in kinds            # named and arrives: prepared
    assert (False, True, False) in kinds          # named, another batch of the geometry arrives
    assert (True, False, False) in kinds          # named with another geometry, or in the warm-up
    assert any(p[1] == 29 and n[1] == 30 and p[2] == n[0] for p, n in zip(H.CHAIN, H.CHAIN[1:]))
    geoms = [H.CHAIN_BATCHES[s[0]][0] for s in H.CHAIN]
    assert geoms[0] == geoms[-1] != geoms[3]      # the geometry changes in mid-chain and comes back


# ------------------------------------------------------------------ the poison
@pytest.mark.parametrize("byte", H.PATTERNS)
def test_poison_leaves_the_exempt_words(byte):
    n = LIB.tail_floats(7)
    t = torch.arange(n, dtype=torch.float32) + 0.5
    t.view(torch.int32)[LIB.T_RANGE] = 2
    H.poison_(t, byte, exempt=(LIB.T_RANGE,))
    raw = t.view(torch.uint8).reshape(n, 4)
    assert int(t.view(torch.int32)[LIB.T_RANGE]) == 2
    others = torch.ones(n, dtype=torch.bool)
    others[LIB.T_RANGE] = False
    assert bool((raw[others] == byte).all())
    word = np.frombuffer(bytes([byte] * 4), np.float32)[0]
    assert np.isnan(word) if byte == 0xFF else (word > 0 and word < 1e-37)      # NaN / a tiny normal f32
    assert np.frombuffer(bytes([byte] * 4), np.uint32)[0] == (0xFFFFFFFF if byte == 0xFF else 16843009)
    e = torch.ones(3, 256)
    assert bool((H.poison_(e, byte).view(torch.uint8) == byte).all())


# ------------------------------------------------------------------ part 3: the other batch
def test_other_batch_differs_in_every_prepared_field_and_in_content():
    named, g = H.chain_problem("a")
    other, g2 = H.chain_problem("c")
    assert g == g2
    for k in ("xc", "mc", "yc", "xn", "mn"):
        assert named[k].shape == other[k].shape and not np.array_equal(named[k], other[k]), k
    # the valid frames themselves differ, not only what lies under the padding
    both = ~named["mc"] & ~other["mc"]
    assert both.any() and not np.array_equal(named["xc"][both], other["xc"][both])
    both = ~named["mn"] & ~other["mn"]
    assert both.any() and not np.array_equal(named["xn"][both], other["xn"][both])
    # padded batches: the tensors behind _prep_key's pointers are distinct storages
    ta, tb = gh.batches(named)[:2], gh.batches(other)[:2]
    ptr = lambda bs: {"xc": bs[0]["net_input"]["feats"].data_ptr(), "mc": bs[0]["net_input"]["padding_mask"].data_ptr(),
                      "xn": bs[1]["net_input"]["feats"].data_ptr(), "mn": bs[1]["net_input"]["padding_mask"].data_ptr()}
    pa, pb = ptr(ta), ptr(tb)
    assert set(pa) == set(H.PADDED_FIELDS) and all(pa[k] != pb[k] for k in pa)
    assert set(H.PADDED_FIELDS) <= set(dadpkg.pkg().DADStep._PREP_BT)
    # store batches: each batch has stores of its own (xc, xn), and other rows and lengths in them
    for (fa, sa, oa, _), (fb, sb, ob, _) in zip(H.store_layouts(named, 0), H.store_layouts(other, 2)):
        assert fa is not fb and not np.array_equal(sa, sb) and not np.array_equal(oa, ob)
        assert all(o % 2 == 1 for o in list(oa) + list(ob))


@pytest.mark.parametrize("name", sorted(H.CHAIN_BATCHES))
def test_chain_batches_fill_their_geometry(name):
    """A store batch's padded length is its longest utterance: one utterance of each side has every frame, so the
    store batch has the padded batch's geometry; no utterance is empty; the operands stay on the grid."""
    inp, g = H.chain_problem(name)
    assert (~inp["mc"]).sum(1).max() == g["T"] and (~inp["mn"]).sum(1).max() == g["Tn"]
    assert (~inp["mc"]).sum(1).min() >= 1 and (~inp["mn"]).sum(1).min() >= 1
    for k in ("xc", "xn"):
        assert np.array_equal(inp[k] * 8, np.round(inp[k] * 8)) and np.abs(inp[k]).max() < 17


# ------------------------------------------------------------------ the problems' masks
ALL = pytest.mark.parametrize("g", X.GEOMS + [H.G65], ids=X.geom_id)


@ALL
def test_gates_are_open_and_the_mask_is_mixed(g):
    """test_exact_problem_cpu's conditions (G65 is not among its problems), and the one parts 1, 2 and 4 rely on:
    with Bn >= 7 the mask holds both values, so eflag, ge_ecda and the ecda scratch carry rows of either kind."""
    C.test_gates_are_open_and_mask_decisions_are_robust(g)
    inp, _, ref = X.case(g, 60)
    mask = np.asarray(ref["oracle"]["mask"])
    if g["Bn"] >= 7:
        assert mask.min() == 0 and mask.max() == 1, mask
    assert (~inp["mc"]).sum(1).max() == g["T"] and (~inp["mn"]).sum(1).max() == g["Tn"]
    assert (~inp["mc"]).sum(1).min() >= 1 and (~inp["mn"]).sum(1).min() >= 1


def test_g65_meets_the_exact_operand_conditions():
    """G65 is held to the float64 bound in part 1: its operands and pre-activations must be exact too."""
    C.test_operands_survive_fp16_and_bf16(H.G65)
    C.test_preactivations_are_exact_in_any_order_and_never_zero(H.G65)
    C.test_fp32_references_lie_inside_the_fp32_bound(H.G65, 60)
    assert X.tau_range(H.G65["Bn"]) == X.TAU_RANGE
