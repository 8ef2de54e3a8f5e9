"""Host side of the whole-split evaluator (evaluate.py: metrics_from_confusion, plan_host), no GPU:
the metrics derived from a confusion matrix against the scikit-learn calls of evaluate.validate, the
slab plan's coverage, and the ctypes mirror of dad_eval_args against the C layout."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import dadpkg

PKG = dadpkg.pkg()
E = PKG.evaluate


def _expand(cm):
    """Label / prediction arrays with exactly this confusion matrix."""
    y, p = [], []
    for i in range(cm.shape[0]):
        for j in range(cm.shape[1]):
            y += [i] * int(cm[i, j])
            p += [j] * int(cm[i, j])
    return np.asarray(y, np.int64), np.asarray(p, np.int64)


def _sklearn_metrics(labels, preds, num_classes=4):
    """The scikit-learn calls of evaluate.validate, verbatim."""
    from sklearn.metrics import (accuracy_score, balanced_accuracy_score, confusion_matrix, f1_score,
                                 precision_recall_fscore_support)
    labs = range(num_classes)
    cm = confusion_matrix(labels, preds, labels=labs)
    prec, rec, f1, sup = precision_recall_fscore_support(labels, preds, average=None, zero_division=0, labels=labs)
    return {
        "accuracy": accuracy_score(labels, preds) * 100,
        "weighted_accuracy": balanced_accuracy_score(labels, preds) * 100,
        "f1_weighted": f1_score(labels, preds, average="weighted", zero_division=0) * 100,
        "f1_macro": f1_score(labels, preds, average="macro", zero_division=0) * 100,
        "precision_per_class": prec.tolist(), "recall_per_class": rec.tolist(),
        "f1_per_class": f1.tolist(), "support_per_class": sup.tolist(), "confusion_matrix": cm,
    }


def _hand_made():
    z = lambda: np.zeros((4, 4), np.int64)
    out = {}
    a = np.array([[5, 1, 0, 2], [0, 0, 0, 0], [1, 2, 7, 0], [0, 3, 1, 4]])       # class 1 never a label
    out["absent_from_y_true"] = a
    b = np.array([[5, 0, 0, 2], [3, 0, 1, 1], [1, 0, 7, 0], [0, 0, 1, 4]])       # class 1 never predicted
    out["absent_from_y_pred"] = b
    c = np.array([[5, 0, 1, 2], [0, 0, 0, 0], [1, 0, 7, 0], [2, 0, 1, 4]])       # class 1 in neither
    out["absent_from_both"] = c
    d = z(); d[2, 2] = 9                                                          # one class, all right
    out["single_class"] = d
    e = z(); e[2, 0] = 4; e[2, 2] = 3; e[2, 3] = 1                                # one label class, mixed preds
    out["single_label_class"] = e
    f = z(); f[3, 3] = 1
    out["single_utterance_right"] = f
    g = z(); g[0, 2] = 1
    out["single_utterance_wrong"] = g
    return out


def _cases():
    rs = np.random.RandomState(20240611)
    cases = [("random%03d" % k, rs.randint(0, 31, size=(4, 4)).astype(np.int64)) for k in range(200)]
    return cases + list(_hand_made().items())


def test_metrics_from_confusion_match_sklearn():
    import warnings
    n = 0
    for name, cm in _cases():
        if cm.sum() == 0:
            continue
        y, p = _expand(cm)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")     # sklearn warns about classes in y_pred that y_true lacks
            want = _sklearn_metrics(y, p)
        got = E.metrics_from_confusion(cm)
        assert sorted(got) == sorted(want), name
        for k in ("accuracy", "weighted_accuracy", "f1_weighted", "f1_macro"):
            assert got[k] == pytest.approx(want[k], abs=1e-9), (name, k)
        for k in ("precision_per_class", "recall_per_class", "f1_per_class"):
            np.testing.assert_allclose(got[k], want[k], rtol=0, atol=1e-12, err_msg="%s %s" % (name, k))
        assert list(got["support_per_class"]) == list(want["support_per_class"]), name
        np.testing.assert_array_equal(got["confusion_matrix"], want["confusion_matrix"], err_msg=name)
        n += 1
    assert n >= 207


def test_metrics_from_confusion_rejects_an_empty_split():
    with pytest.raises(ValueError):
        E.metrics_from_confusion(np.zeros((4, 4), np.int64))


def _coverage(sizes, offsets):
    rows, lens, slab_off = E.plan_host(sizes, offsets)
    utt, chunk = E.slab_jobs(slab_off)
    seen = {}
    for u, c in zip(utt.tolist(), chunk.tolist()):
        assert 0 <= c and 32 * c < lens[u], (u, c)          # no job without a valid frame
        for t in range(32 * c, min(32 * c + 32, int(lens[u]))):
            key = (u, t)
            assert key not in seen
            seen[key] = int(rows[u]) + t
    return rows, lens, slab_off, seen


def test_plan_host_covers_every_valid_frame_once():
    sizes = np.array([0, 1, 31, 32, 33, 64, 65])
    offsets = np.concatenate([[0], np.cumsum(sizes)[:-1]])
    rows, lens, slab_off, seen = _coverage(sizes, offsets)
    assert rows.dtype == np.int64 and lens.dtype == np.int32 and slab_off.dtype == np.int32
    assert slab_off.tolist() == [0, 0, 1, 2, 3, 5, 7, 10]
    assert sorted(seen) == [(u, t) for u in range(len(sizes)) for t in range(int(sizes[u]))]
    # every valid frame maps to its own store row, and nothing else is touched
    assert sorted(seen.values()) == list(range(int(sizes.sum())))


def test_plan_host_handles_unsorted_repeated_and_trailing_empty_samples():
    sizes = np.array([40, 0, 7, 40, 0])
    offsets = np.array([100, 0, 3, 100, 50])        # sample 3 repeats sample 0's rows
    rows, lens, slab_off, seen = _coverage(sizes, offsets)
    assert slab_off.tolist() == [0, 2, 2, 3, 5, 5]
    assert rows.tolist() == [100, 0, 3, 100, 0]     # empty samples read nothing: row 0
    assert len(seen) == int(sizes.sum())
    assert [seen[(3, t)] for t in range(40)] == list(range(100, 140))


def test_plan_host_rejects_bad_sizes():
    with pytest.raises(ValueError):
        E.plan_host([3, -1], [0, 3])
    with pytest.raises(ValueError):
        E.plan_host([3, 4], [0])


def test_result_block_slots_mirror_the_header():
    L = PKG._lib
    hdr = open(os.path.join(dadpkg.ROOT, "include", "dad.h")).read()
    for py, c in (("EV_CONF_STUDENT", "DAD_EV_CONF_STUDENT"), ("EV_CONF_TEACHER", "DAD_EV_CONF_TEACHER"),
                  ("EV_DISAGREE", "DAD_EV_DISAGREE"), ("EV_N", "DAD_EV_N"), ("EV_N_LABELLED", "DAD_EV_N_LABELLED"),
                  ("EV_N_SKIPPED", "DAD_EV_N_SKIPPED"), ("EV_N_NONFINITE", "DAD_EV_N_NONFINITE"),
                  ("EV_COUNTS", "DAD_EV_COUNTS"), ("EV_MOMENTS", "DAD_EV_MOMENTS"), ("EV_M_COUNT", "DAD_EV_M_COUNT"),
                  ("EV_M_MEAN", "DAD_EV_M_MEAN"), ("EV_M_VAR", "DAD_EV_M_VAR")):
        assert "#define %s %d " % (c, getattr(L, py)) in hdr.replace("\n", " \n"), c


def test_eval_args_struct_matches_c_layout(tmp_path):
    cls = PKG._lib.DadEvalArgs
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "dad.h"', "int main(void){",
             'printf("size %zu\\n", sizeof(dad_eval_args));']
    for f in cls._fields_:
        lines.append('printf("%s %%zu\\n", offsetof(dad_eval_args, %s));' % (f[0], f[0]))
    lines.append("return 0;}")
    c = tmp_path / "probe.c"
    c.write_text("\n".join(lines))
    exe = tmp_path / "probe"
    subprocess.check_call(["gcc", "-I", os.path.join(dadpkg.ROOT, "include"), str(c), "-o", str(exe)])
    out = dict(l.split() for l in subprocess.check_output([str(exe)]).decode().splitlines())
    assert int(out["size"]) == ctypes.sizeof(cls)
    for f in cls._fields_:
        assert int(out[f[0]]) == getattr(cls, f[0]).offset, f[0]


def test_eval_split_host_validation():
    """Argument checks that return before any device call."""
    L = PKG.lib()
    A = PKG._lib.DadEvalArgs
    assert L.dad_eval_workspace_bytes(10, 30, PKG._lib.PREC_FP32, 0) > 0
    assert (L.dad_eval_workspace_bytes(10, 30, PKG._lib.PREC_FP16, 1)
            > L.dad_eval_workspace_bytes(10, 30, PKG._lib.PREC_FP32, 1)
            > L.dad_eval_workspace_bytes(10, 30, PKG._lib.PREC_FP32, 0))
    assert L.dad_eval_workspace_bytes(0, 0, PKG._lib.PREC_FP32, 0) == 0
    assert L.dad_eval_split(None, None, None) == 1001
    a = A()
    assert L.dad_eval_split(ctypes.byref(a), ctypes.c_void_p(256), None) == 1001      # null required pointers
    for f in ("store", "rows", "lens", "slab_off", "student", "counts", "moments"):
        setattr(a, f, 256)          # never dereferenced: every case below returns from the checks
    a.n, a.slabs = 0, 0
    assert L.dad_eval_split(ctypes.byref(a), ctypes.c_void_p(256), None) == 1002      # n < 1
    a.n, a.slabs = 4, -1
    assert L.dad_eval_split(ctypes.byref(a), ctypes.c_void_p(256), None) == 1002
    a.n, a.slabs = 4, 4 * (1 << 26) + 1
    assert L.dad_eval_split(ctypes.byref(a), ctypes.c_void_p(256), None) == 1002      # more slabs than n can hold
    a.n, a.slabs = 4, 8
    a.precision = PKG._lib.PREC_BF16
    assert L.dad_eval_split(ctypes.byref(a), ctypes.c_void_p(256), None) == 1004      # DAD_E_UNSUPPORTED
    a.precision = 7
    assert L.dad_eval_split(ctypes.byref(a), ctypes.c_void_p(256), None) == 1001
    a.precision = PKG._lib.PREC_FP32
    a.store_dtype = 9
    assert L.dad_eval_split(ctypes.byref(a), ctypes.c_void_p(256), None) == 1001
