"""tests/data_path.py on the CPU: the coverage conditions of its cases, its references against torch's CPU conversions
and oracle/data_oracle.collate, and one wrong-answer control per reference (each control must change what the GPU
module compares)."""
import numpy as np
import pytest
import torch

import data_path as P
from oracle import data_oracle as do

ALL16 = np.arange(65536, dtype=np.uint32).astype(np.uint16)


def _t16(bits, dt):
    return torch.from_numpy(bits.view(np.int16).copy()).view(torch.float16 if dt == "f16" else torch.bfloat16)


def _bits16(t):
    return t.contiguous().view(torch.int16).numpy().view(np.uint16)


# ---- conditions of the cases ---------------------------------------------------------------------------------------------
def test_every_pattern_at_every_column_residue():
    bits = P.pattern_store()
    assert bits.shape == (1024, 768) and P.all_patterns_at_every_residue(bits)
    assert not P.all_patterns_at_every_residue(bits[:600])                  # (the condition can fail)
    sizes, offsets, batches = P.pattern_layout()
    assert sizes.sum() == 1024 and {1, 2, 33} <= set(sizes.tolist())
    assert sorted(i for b in batches for i in b) == list(range(len(sizes))) and max(map(len, batches)) <= 64
    assert P.is_nan16(ALL16, "f16").sum() == 2046 and P.is_subnormal16(ALL16, "f16").sum() == 2046
    assert P.is_nan16(ALL16, "bf16").sum() == 254 and P.is_subnormal16(ALL16, "bf16").sum() == 254


def probe_shares():
    """{store/precision: share of the 65,536 patterns the probe keeps}"""
    out = {}
    for dt in ("f16", "bf16"):
        for precision in ("fp32", "fp16", "bf16"):
            keep = P.finite32(P.widen(ALL16, dt)) & P.finite32(P.operand_bits(ALL16, dt, precision))
            out["%s/%s" % (dt, precision)] = float(keep.mean())
    return out


@pytest.mark.parametrize("precision", ["fp32", "fp16", "bf16"])
@pytest.mark.parametrize("dt", ["f16", "bf16"])
def test_probe_covers_every_finite_pattern_and_all_subnormals(dt, precision):
    bits, covered = P.probe_store(dt, precision)
    keep = P.finite32(P.widen(ALL16, dt)) & P.finite32(P.operand_bits(ALL16, dt, precision))
    assert keep[P.is_subnormal16(ALL16, dt)].all()                          # all subnormals are included
    masked = np.where(covered, bits, np.uint16(P.ONE[dt]))
    assert np.array_equal(masked, bits) and P.all_patterns_at_every_residue(bits, keep)
    assert P.finite32(P.operand_bits(bits, dt, precision)).all()
    share = probe_shares()["%s/%s" % (dt, precision)]
    print("probe %s store at %s: %.4f of the patterns covered" % (dt, precision, share))
    # finite patterns: 63,488 of fp16 (0.96875), 65,280 of bf16 (0.9961); bf16 beyond the fp16 range leaves at fp16
    want = {"f16": 63488 / 65536, "bf16": 65280 / 65536}[dt]
    assert share == want if (dt, precision) != ("bf16", "fp16") else 0.55 < share < 0.57
    # every read-out expectation is finite, and every covered column is read by exactly one (group, sign > 0) pair
    ops = P.operand_bits(bits, dt, precision)
    both = [P.readout_expected(ops, g, s) for g, s in P.READOUT]
    assert all(P.finite32(e).all() for e in both)
    for g in range(3):
        plus, minus = both[2 * g], both[2 * g + 1]
        x = ops[:, 256 * g:256 * (g + 1)]
        mag = x & np.uint32(0x7FFFFFFF)
        assert np.array_equal(np.maximum(plus, minus) & np.uint32(0x7FFFFFFF), mag)     # one of the two returns |x|


def test_edge_cases_hold_what_the_issue_lists():
    feats, sizes, offsets, labels = P.edge_store()
    assert {0, 1} <= set(sizes.tolist()) and offsets[-1] == feats.shape[0] and sizes[-1] == 0
    assert sizes[1] == 0 and sizes[0] > 0 and sizes[2] > 0 and {-1, 9} <= set(labels.tolist())
    assert np.array_equal(feats, np.round(feats)) and np.abs(feats).max() <= 125
    for dt in ("f16", "bf16"):                                              # exact in every store type
        t = torch.from_numpy(feats.copy()).to(torch.float16 if dt == "f16" else torch.bfloat16)
        assert torch.equal(t.float(), torch.from_numpy(feats.copy()))
    for B, T in P.COLLATE_SHAPES + P.INDEX_SHAPES:
        idx = P.edge_index(sizes, B, T)
        assert len(idx) == B and sizes[idx].max() <= T
        if B >= 3:
            assert len(set(idx.tolist())) < B
    assert sorted(B * T for B, T in P.INDEX_SHAPES)[:6] == [7, 255, 255, 256, 257, 257] and (19, 27) in P.INDEX_SHAPES
    assert (P.edge_index(sizes, 5, 7, cap=5).size, sizes[P.edge_index(sizes, 5, 7, cap=5)].max()) == (5, 5)
    ep = P.ref_collate_index_epoch(sizes, offsets, labels, P.edge_epoch())
    assert tuple(ep["T"][:5]) == P.EPOCH_TS and len(P.edge_epoch()[-1]) == 1
    assert sizes[P.edge_subset()].min() == 0 and len(set(P.edge_subset().tolist())) < len(P.edge_subset())
    bad = P.with_out_of_range([5, 3, 0], len(sizes))
    assert bad.tolist() == [5, -1, 3, len(sizes), 0, 2 ** 40, P.INT64_MIN]


# ---- the references against torch and the oracle ------------------------------------------------------------------------
def test_widening_references_equal_torch():
    for dt in ("f16", "bf16"):
        want = _t16(ALL16, dt).float().view(torch.int32).numpy().view(np.uint32)
        got = P.widen(ALL16, dt)
        nan = P.is_nan16(ALL16, dt)
        assert np.array_equal(got[~nan], want[~nan])
        assert np.isnan(got[nan].view(np.float32)).all() and np.isnan(want[nan].view(np.float32)).all()


def test_operand_rounding_references_equal_torch():
    for src, dst, fn in (("f16", torch.bfloat16, P.f32_to_bf16_bits), ("bf16", torch.float16, P.f32_to_f16_bits)):
        want = _bits16(_t16(ALL16, src).to(dst))
        got = fn(P.widen(ALL16, src))
        nan = P.is_nan16(ALL16, src)
        assert np.array_equal(got[~nan], want[~nan]), src
        assert P.is_nan16(got[nan], "bf16" if src == "f16" else "f16").all()
    rs = np.random.RandomState(5)
    u = rs.randint(0, 2 ** 32, size=1 << 20, dtype=np.uint64).astype(np.uint32)
    u = np.concatenate([u, P.widen_f16(ALL16) + np.uint32(0x1000), P.widen_f16(ALL16) + np.uint32(0x0FFF),
                        P.widen_f16(ALL16) + np.uint32(0x1001)])            # every fp16 tie and its two neighbours
    u = u[P.finite32(u)]
    x = torch.from_numpy(u.view(np.int32).copy()).view(torch.float32)
    assert np.array_equal(P.f32_to_f16_bits(u), _bits16(x.half()))
    assert np.array_equal(P.f32_to_bf16_bits(u), _bits16(x.bfloat16()))


@pytest.mark.parametrize("labelled", [True, False])
def test_ref_collate_agrees_with_the_oracle(labelled):
    feats, sizes, offsets, labels = P.edge_store()
    wide = feats.view(np.uint32)
    lab = labels if labelled else None
    n = 0
    for index in ([0], [3, 3, 5], [8, 1, 2, 0], [15, 13, 14, 16, 17], list(P.edge_subset())):
        want = do.collate(feats, sizes, offsets, lab, index)
        got = P.ref_collate(wide, sizes, offsets, lab, index, want["feats"].shape[1])
        assert np.array_equal(got["feats"], want["feats"].view(np.uint32))
        assert np.array_equal(got["pad"].astype(bool), want["padding_mask"])
        assert (got["labels"] is None and want["labels"] is None) or np.array_equal(got["labels"], want["labels"])
        idx = P.ref_collate_index(sizes, offsets, lab, index, want["feats"].shape[1])
        assert np.array_equal(idx["pad"], got["pad"]) and np.array_equal(idx["lens"], sizes[index])
        n += 1
    assert n == 5


def test_out_of_range_and_empty_rows_by_the_contract():
    feats, sizes, offsets, labels = P.edge_store()
    index = P.with_out_of_range([5, 3, 17], len(sizes))
    got = P.ref_collate(feats.view(np.uint32), sizes, offsets, labels, index, 9)
    idx = P.ref_collate_index(sizes, offsets, labels, index, 9)
    for b in (1, 3, 5, 6):
        assert got["pad"][b].all() and not got["feats"][b].any() and got["labels"][b] == -1
        assert idx["rows"][b] == 0 and idx["lens"][b] == 0 and idx["labels"][b] == -1
    assert got["pad"][4].all() and got["labels"][4] == labels[17] and idx["rows"][4] == 0     # empty, at the store's end
    assert got["labels"][0] == 9 and not got["pad"][0].any()


# ---- wrong-answer controls ------------------------------------------------------------------------------------------------
def test_control_pad_off_by_one_and_row_not_zeroed():
    _, sizes, offsets, labels = P.edge_store()
    for B, T in P.INDEX_SHAPES:
        idx = P.edge_index(sizes, B, T)
        right = P.ref_collate_index(sizes, offsets, labels, idx, T)
        wrong = P.ref_collate_index(sizes, offsets, labels, idx, T, mutate="pad_off_by_one")
        if (sizes[idx] < T).any():
            assert not np.array_equal(right["pad"], wrong["pad"]), (B, T)
    idx = np.array([0, 17, 1], np.int64)
    right = P.ref_collate_index(sizes, offsets, labels, idx, 3)
    wrong = P.ref_collate_index(sizes, offsets, labels, idx, 3, mutate="row_kept")
    assert right["rows"].tolist() == [offsets[0], 0, 0] and wrong["rows"][1] == offsets[17] != 0 and wrong["rows"][2] != 0
    right = P.ref_collate_index_epoch(sizes, offsets, labels, P.edge_epoch())
    wrong = P.ref_collate_index_epoch(sizes, offsets, labels, P.edge_epoch(), mutate="pad_off_by_one")
    assert not np.array_equal(right["pad"], wrong["pad"])
    cut = right["pad"].copy()                                              # the pad loop cut after its first trip
    for off, T in zip(right["pad_off"], right["pad_T"]):
        cut[off + 256:off + T] = P.PAD_SENTINEL
    assert not np.array_equal(cut, right["pad"])


def first_word_twice(wide):
    """The historical miscompile: of a lane's four elements (two words), the first word converted twice."""
    out = wide.reshape(wide.shape[0], -1, 4).copy()
    out[:, :, 2:] = out[:, :, :2]
    return out.reshape(wide.shape)


def test_control_first_word_twice():
    for dt in ("f16", "bf16"):
        right = P.widen(P.pattern_store(), dt)
        wrong = first_word_twice(right)
        assert (right != wrong).mean() > 0.49
        sizes, offsets, batches = P.pattern_layout()
        for b in batches:                                                   # every batch of the GPU test sees it
            T = int(sizes[b].max())
            assert not np.array_equal(P.ref_collate(right, sizes, offsets, None, b, T)["feats"],
                                      P.ref_collate(wrong, sizes, offsets, None, b, T)["feats"])


def test_control_truncation_and_flushed_subnormals():
    bits, _ = P.probe_store("bf16", "fp16")
    right = P.operand_bits(bits, "bf16", "fp16")
    assert not np.array_equal(right, P.operand_bits(bits, "bf16", "fp16", mode="trunc"))
    flushed = P.operand_bits(bits, "bf16", "fp16", mode="ftz")
    sub = P.is_subnormal16(P.f32_to_f16_bits(P.widen(bits, "bf16")), "f16")
    assert sub.sum() > 1000 and (right[sub] != flushed[sub]).all() and np.array_equal(right[~sub], flushed[~sub])
    bits, _ = P.probe_store("f16", "bf16")
    assert not np.array_equal(P.operand_bits(bits, "f16", "bf16"), P.operand_bits(bits, "f16", "bf16", mode="trunc"))
    assert P.subnormal_operand(right, "fp16").sum() == sub.sum() and not P.subnormal_operand(flushed, "fp16").any()
    # and the read-out sees each of them
    for g, s in P.READOUT:
        assert not np.array_equal(P.readout_expected(right, g, s), P.readout_expected(flushed, g, s))


@pytest.mark.parametrize("dt", ["f16", "f32"])
def test_control_wrapped_address(dt):
    sizes, offsets = P.big_layout(dt)
    fb = P.BIG[dt]["boundary"]
    assert (offsets + sizes <= fb).sum() == 2 and (offsets > fb).sum() == 2
    assert ((offsets <= fb) & (offsets + sizes > fb)).sum() == 1
    for k in range(len(sizes)):
        right, wrong = P.big_rows(dt, k), P.big_rows_wrapped(dt, k)
        assert np.array_equal(right * 8, np.round(right * 8)) and np.abs(right).max() <= 31.75
        if offsets[k] + sizes[k] <= fb:
            assert np.array_equal(right, wrong)
        else:                                                               # every row at or past the boundary differs
            rows = np.arange(offsets[k], offsets[k] + sizes[k]) >= fb
            assert (right[rows] != wrong[rows]).any(axis=1).all()
    csz, coff, frames = P.compact_layout(dt)
    assert np.array_equal(csz, sizes) and (coff + csz).max() < frames < 200


def test_train_probe_keeps_every_pattern_up_to_256():
    """The train step's probe (limit 256): every pattern of magnitude <= 256 at every c mod 8, all subnormals among
    them; the share of the 65,536 patterns is printed."""
    for dt in ("f16", "bf16"):
        for precision in ("fp32", "fp16", "bf16"):
            bits, covered = P.probe_store(dt, precision, limit=256.0)
            wide = P.widen(ALL16, dt)
            keep = P.finite32(wide) & (np.abs(wide.view(np.float32)) <= 256) & \
                (np.abs(P.operand_bits(ALL16, dt, precision).view(np.float32)) <= 256)
            assert keep[P.is_subnormal16(ALL16, dt)].all() and P.all_patterns_at_every_residue(bits, keep)
            assert np.abs(P.operand_bits(bits, dt, precision).view(np.float32)).max() == 256
            print("train probe %s store at %s: %.4f of the patterns covered" % (dt, precision, keep.mean()))
            assert keep.mean() > (0.7 if dt == "f16" else 0.5)
