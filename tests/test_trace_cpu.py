"""The device-side confirmation-bias log and DACP history (dad_trace_append, trace.TrainingTrace): the parts
that need no GPU.  The entry points and their argument checks, the reference's tracked-id draw, the bitmap,
the decoding of records into the reference's log entries, and the two files save() writes."""
import ctypes
import json
import os
import struct
import warnings

import numpy as np
import pytest

import dadpkg

PKG = dadpkg.pkg()
LIB = PKG._lib
TR = PKG.trace


def test_library_exports_the_trace_entry_points():
    L = LIB.lib()
    assert hasattr(L, "dad_trace_append") and hasattr(L, "dad_trace_bytes")
    assert "dad_trace_append" in LIB.EXPORTS and "dad_trace_bytes" in LIB.EXPORTS
    for c in (0, 1, 10, 2500, 2 ** 31 - 1):
        assert L.dad_trace_bytes(c) == (4 + 4 * c) * 4
    assert (LIB.TRACE_HDR_WORDS, LIB.TRACE_REC_WORDS, LIB.TRACE_MASKED_IN) == (4, 4, 0x100)
    hdr = open(os.path.join(dadpkg.ROOT, "include", "dad.h")).read()
    for name, v in (("HDR_WORDS", "4"), ("REC_WORDS", "4"), ("MASKED_IN", "0x100")):
        assert "#define DAD_TRACE_%s %s" % (name, v) in hdr
    assert PKG.TrainingTrace is TR.TrainingTrace


def test_argument_errors_come_before_any_launch():
    """No device is present here: every refusal below returns before the launch."""
    L = LIB.lib()
    p = ctypes.c_void_p(0x1000)           # never followed: the checks only test for NULL / alignment
    ok = dict(tail=p, Bn=8, ids=p, tracked=p, n=100, epoch=3, trace=p, cap=10)

    def call(**kw):
        a = dict(ok, **kw)
        return L.dad_trace_append(a["tail"], a["Bn"], a["ids"], a["tracked"], a["n"], a["epoch"], a["trace"], a["cap"],
                                  None)

    for name in ("tail", "ids", "tracked", "trace"):
        assert call(**{name: None}) == LIB.E_ARG, name
    assert call(trace=ctypes.c_void_p(0x1004)) == LIB.E_ARG        # records are 16-byte stores
    for kw in (dict(Bn=0), dict(Bn=-1), dict(Bn=1025), dict(n=0), dict(n=2 ** 31), dict(cap=-1), dict(cap=2 ** 31)):
        assert call(**kw) == LIB.E_SHAPE, kw


@pytest.mark.parametrize("n", [51, 5531])
@pytest.mark.parametrize("seed", [0, 1234])
def test_tracked_ids_are_the_references_draw(n, seed):
    """I/train.py:279-284: np.random.choice(total, 50, replace=False).tolist() from the global RNG."""
    np.random.seed(seed)
    want = np.random.choice(n, 50, replace=False).tolist()
    want_next = np.random.random()
    np.random.seed(seed)
    tr = TR.TrainingTrace(n, tracked=50, epochs=3, device="cpu")
    assert np.random.random() == want_next                          # the RNG is left where the bare call leaves it
    assert tr.tracked_sample_indices == want
    assert all(type(i) is int for i in tr.tracked_sample_indices)
    assert tr.active and tr.capacity == 150
    assert tr.buffer.numel() == 4 + 4 * 150 and int(tr.buffer.abs().sum()) == 0


def test_tracking_is_off_when_the_set_is_not_larger_than_k():
    np.random.seed(7)
    want_next = np.random.random()
    np.random.seed(7)
    tr = TR.TrainingTrace(50, tracked=50, epochs=3, device="cpu")
    assert np.random.random() == want_next                          # the reference draws nothing then
    assert tr.tracked_sample_indices == [] and not tr.active and tr.capacity == 0
    assert tr.bias_log() == [] and tr.dropped == 0


def test_tracked_given_or_all():
    tr = TR.TrainingTrace(100, tracked=[5, 99, 0], epochs=2, device="cpu")
    assert tr.tracked_sample_indices == [5, 99, 0] and tr.capacity == 6
    tr = TR.TrainingTrace(100, tracked="all", epochs=2, device="cpu")
    assert tr.tracked_sample_indices == list(range(100)) and tr.capacity == 200
    assert TR.TrainingTrace(100, tracked="all", capacity=7, device="cpu").capacity == 7
    with pytest.raises(ValueError):
        TR.TrainingTrace(100, tracked=[100], epochs=1, device="cpu")
    with pytest.raises(ValueError):
        TR.TrainingTrace(100, tracked=[1], device="cpu")             # neither epochs nor capacity

    class Loader:
        dataset = list(range(77))
    assert TR.TrainingTrace.for_loader(Loader(), tracked=[1, 2], epochs=5, device="cpu").n_samples == 77


@pytest.mark.parametrize("n", [33, 64, 65, 5000])
def test_bitmap_packing(n):
    ids = sorted({0, 31, 32, n - 1})
    want = np.zeros((n + 31) // 32, dtype=np.uint32)
    for i in ids:
        want[i >> 5] |= np.uint32(1) << np.uint32(i & 31)
    got = TR.pack_bitmap(ids, n)
    assert got.dtype == np.uint32 and got.shape == want.shape
    np.testing.assert_array_equal(got, want)
    assert TR.pack_bitmap([], n).sum() == 0
    tr = TR.TrainingTrace(n, tracked=ids, epochs=1, device="cpu")
    np.testing.assert_array_equal(tr.bitmap.numpy().view(np.uint32), want)


def _bits(x):
    return struct.unpack("<i", struct.pack("<f", x))[0]


def test_record_decoding():
    scores = [np.float32(0.1), np.float32(0.73456789), np.float32(1.0), np.float32(1e-7)]
    rec = np.array([[30, 17, 2 | 0x100, _bits(scores[0])],
                    [30, 4999, 3, _bits(scores[1])],
                    [31, 0, 0 | 0x100, _bits(scores[2])],
                    [99, 2 ** 31 - 2, 1, _bits(scores[3])]], dtype=np.int32)
    words = np.concatenate([np.array([4, 0, 0, 0], np.int32), rec.reshape(-1), np.full(8, -1, np.int32)])
    log, offered = TR.decode_records(words, capacity=6)
    assert offered == 4 and len(log) == 4
    want = [dict(epoch=30, sample_id=17, pseudo_label=2, certainty_score=float(scores[0]), is_masked_in=True),
            dict(epoch=30, sample_id=4999, pseudo_label=3, certainty_score=float(scores[1]), is_masked_in=False),
            dict(epoch=31, sample_id=0, pseudo_label=0, certainty_score=float(scores[2]), is_masked_in=True),
            dict(epoch=99, sample_id=2 ** 31 - 2, pseudo_label=1, certainty_score=float(scores[3]), is_masked_in=False)]
    assert log == want
    for e in log:       # the reference's keys (I/train.py:430-436), in its order, with its Python types
        assert list(e) == ["epoch", "sample_id", "pseudo_label", "certainty_score", "is_masked_in"]
        assert [type(v) for v in e.values()] == [int, int, int, float, bool]
    back = json.loads(json.dumps(log))
    for e, s in zip(back, scores):
        assert np.float32(e["certainty_score"]) == s and e["certainty_score"] == float(s)


def test_overflow_is_counted_and_warned_once():
    tr = TR.TrainingTrace(100, tracked=[1, 2, 3], capacity=2, device="cpu")
    w = tr.buffer.numpy()
    w[0] = 5                                  # five offered, two kept
    w[4:12] = [7, 1, 0x102, _bits(0.5), 7, 3, 1, _bits(0.25)]
    with pytest.warns(RuntimeWarning, match="3 of 5"):
        assert tr.dropped == 3
    with warnings.catch_warnings():
        warnings.simplefilter("error")        # once only
        log = tr.bias_log()
        assert tr.dropped == 3
    assert [e["sample_id"] for e in log] == [1, 3] and log[0]["is_masked_in"] and not log[1]["is_masked_in"]


def test_save_writes_the_files_the_analysis_scripts_read(tmp_path):
    import torch
    tr = TR.TrainingTrace(100, tracked=[1, 2], epochs=2, device="cpu")

    class Step:                               # what end_epoch reads of a DADStep
        class view:
            ECDA_CLASS_ATTENTION_LAMBDA = 1.5
        ema_thresholds = torch.tensor([0.5, 0.6, 0.7, 0.8])
        class_quality_scores = torch.tensor([0.4, 0.5, 0.6, 0.9])

    tr.end_epoch(Step)
    Step.class_quality_scores = torch.tensor([0.1, 0.2, 0.3, 0.4])
    tr.end_epoch(Step)
    tr.add_validation("Noisy", {"disagreement_rate": np.float64(0.25), "accuracy": 1.0})
    tr.add_validation("Clean", {"disagreement_rate": 0.125})
    tr.add_validation("Clean", {"accuracy": 1.0})            # no teacher pass: nothing appended
    paths = tr.save(str(tmp_path))
    hist_path = os.path.join(str(tmp_path), "reports", "training_history.json")
    assert paths == [hist_path]
    assert not os.path.exists(os.path.join(str(tmp_path), "reports", "confirmation_bias_log.json"))   # empty log
    h = json.load(open(hist_path))
    # analyze_dacp_evolution.py's required keys; analyze_disagreement.py's series
    assert set(h) == {"dacp_ema_thresholds", "dacp_class_quality", "ecda_class_attention", "disagreement_rate_noisy",
                      "disagreement_rate_clean"}
    assert h == tr.history()
    assert len(h["dacp_ema_thresholds"]) == len(h["dacp_class_quality"]) == len(h["ecda_class_attention"]) == 2
    assert all(len(r) == 4 for k in ("dacp_ema_thresholds", "dacp_class_quality", "ecda_class_attention") for r in h[k])
    assert h["disagreement_rate_noisy"] == [0.25] and h["disagreement_rate_clean"] == [0.125]
    q = torch.tensor([0.1, 0.2, 0.3, 0.4])
    np.testing.assert_allclose(h["ecda_class_attention"][1], torch.exp(1.5 * (q.mean() - q)).tolist(), rtol=1e-6)
    np.testing.assert_array_equal(np.float32(h["dacp_class_quality"][0]), np.float32([0.4, 0.5, 0.6, 0.9]))
    assert open(hist_path).read() == json.dumps(tr.history(), indent=4)           # the reference's layout

    w = tr.buffer.numpy()
    w[0] = 1
    w[4:8] = [40, 2, 0x103, _bits(0.75)]
    paths = tr.save(str(tmp_path))
    log_path = os.path.join(str(tmp_path), "reports", "confirmation_bias_log.json")
    assert paths == [hist_path, log_path]
    log = json.load(open(log_path))
    # analyze_confirmation_bias.py builds a DataFrame of these columns
    assert log == [{"epoch": 40, "sample_id": 2, "pseudo_label": 3, "certainty_score": 0.75, "is_masked_in": True}]
    assert open(log_path).read() == json.dumps(tr.bias_log(), indent=4)
