"""The host-only parts of the k-NN entry points: dad_knn_plan, dad_knn_workspace_bytes, every DAD_E_SHAPE / DAD_E_ARG
path that is decided before a device call, the DAD_KNN_* / DAD_KV_* / DAD_TW_* defines of header and binding, and
neighbourhood_from_scores' arithmetic."""
import ctypes
import os
import re

import pytest

import dadpkg

PKG = dadpkg.pkg()
E = PKG.evaluate
L = PKG._lib
P = ctypes.c_void_p(256)        # never dereferenced: every call it goes to fails its checks first


@pytest.fixture(scope="module", autouse=True)
def _built():
    PKG.build(verbose=False)


@pytest.mark.parametrize("k", [1, 5, 16, 17, 32])
@pytest.mark.parametrize("n,cus", [(1, 256), (37, 256), (1100, 256), (5531, 256), (5531, 8), (65536, 256), (65536, 304)])
def test_plan_covers_every_column_tile_once(n, cus, k):
    fn = L.require("dad_knn_plan", "the plan")
    rt, ch, per = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    assert fn(n, k, cus, ctypes.byref(rt), ctypes.byref(ch), ctypes.byref(per)) == 0
    assert rt.value == -(-n // L.KNN_TILE)
    assert 1 <= ch.value <= min(rt.value, L.KNN_MAX_CHUNKS)
    assert (ch.value - 1) * per.value < rt.value <= ch.value * per.value        # every tile once, no empty chunk
    # the grid is resident at once: two workgroups a compute unit up to k = 16, one above
    assert ch.value == 1 or rt.value * ch.value <= (2 if k <= 16 else 1) * cus


def test_plan_refuses_what_the_calls_refuse():
    fn = L.require("dad_knn_plan", "the plan")
    v = [ctypes.c_int() for _ in range(3)]
    for n, k, cus in ((0, 5, 256), (L.KNN_MAX_N + 1, 5, 256), (100, 0, 256), (100, L.KNN_MAX_K + 1, 256), (100, 5, 0)):
        assert fn(n, k, cus, *v) == L.E_SHAPE
    assert fn(100, 5, 256, None, v[1], v[2]) == L.E_ARG


def test_workspace_bytes():
    fn = L.require("dad_knn_workspace_bytes", "the test")
    for n, k in ((0, 5), (-1, 5), (L.KNN_MAX_N + 1, 5), (100, 0), (100, L.KNN_MAX_K + 1)):
        assert fn(n, k) == 0
    assert 0 < fn(1, 1) < fn(1, 32) and fn(64, 5) < fn(65, 5) < fn(1100, 5) < fn(1100, 32)
    for n, k in ((37, 5), (1100, 32), (L.KNN_MAX_N, L.KNN_MAX_K)):
        rt = -(-n // L.KNN_TILE)
        lists = 8 * min(rt, L.KNN_MAX_CHUNKS) * rt * L.KNN_TILE * k          # the chunks' (d2, idx) lists
        assert lists < fn(n, k) < lists + 16 * rt * L.KNN_TILE * k + 4096 * rt + 16384
        assert fn(n, k) % 256 == 0


def test_knn_argument_errors_come_before_any_launch():
    for name, tail in (("dad_knn", (P, None)), ("dad_knn_chunked", (3, P, None))):
        fn = L.require(name, "the test")
        call = lambda emb=P, n=4, k=1, mode=L.KNN_ALL, idx=P, d2=P, tail=tail: fn(emb, None, n, k, mode, idx, d2, *tail)
        assert call(emb=None) == L.E_ARG and call(idx=None) == L.E_ARG and call(d2=None) == L.E_ARG
        assert call(tail=tail[:-2] + (None, None)) == L.E_ARG               # no workspace
        assert call(mode=3) == L.E_ARG and call(mode=-1) == L.E_ARG
        for k in (0, -1, L.KNN_MAX_K + 1):
            assert call(k=k) == L.E_SHAPE
        for n in (0, -3, L.KNN_MAX_N + 1):
            assert call(n=n) == L.E_SHAPE


def test_vote_argument_errors_come_before_any_launch():
    fn = L.require("dad_knn_vote", "the test")
    for args in ((None, P, None, 4, 1, P, P, None), (P, None, None, 4, 1, P, P, None), (P, P, None, 4, 1, None, P, None),
                 (P, P, None, 4, 1, P, None, None)):
        assert fn(*args) == L.E_ARG
    for n, k in ((0, 1), (L.KNN_MAX_N + 1, 1), (4, 0), (4, L.KNN_MAX_K + 1)):
        assert fn(P, P, None, n, k, P, P, None) == L.E_SHAPE


def test_trustworthiness_argument_errors_come_before_any_launch():
    for name, tail in (("dad_trustworthiness", (P, None)), ("dad_trustworthiness_chunked", (3, P, None))):
        fn = L.require(name, "the test")
        call = lambda emb=P, Y=P, n=100, k=5, out=P, tail=tail: fn(emb, Y, n, k, out, None, *tail)
        assert call(emb=None) == L.E_ARG and call(Y=None) == L.E_ARG and call(out=None) == L.E_ARG
        assert call(tail=tail[:-2] + (None, None)) == L.E_ARG
        for n, k in ((100, 0), (100, 33), (0, 5), (L.KNN_MAX_N + 1, 5), (10, 5), (11, 6), (2, 1), (64, 32), (1, 1)):
            assert call(n=n, k=k) == L.E_SHAPE, (n, k)            # scikit-learn: n_neighbors < n_samples / 2


def test_header_defines_equal_the_binding():
    hdr = open(os.path.join(dadpkg.ROOT, "include", "dad.h")).read()
    for prefix, names in (("KNN", {"ALL", "SAME", "OTHER", "MAX_K", "MAX_N", "TILE", "MAX_CHUNKS", "WS_NONFINITE"}),
                          ("KV", {"CONFUSION", "QUERIES", "NO_VOTE", "SLOTS"}),
                          ("TW", {"T", "PENALTY", "N", "K", "VALID", "NONFINITE", "SLOTS"})):
        defs = {k: int(v) for k, v in re.findall(r"^#define DAD_%s_([A-Z_]+) (\d+)" % prefix, hdr, flags=re.M)}
        assert set(defs) == names, prefix
        for k, v in defs.items():
            assert getattr(L, "%s_%s" % (prefix, k)) == v, (prefix, k)
    assert L.KNN_MAX_K == 32 and L.KNN_MAX_N == 65536 and L.KV_SLOTS >= L.KV_NO_VOTE + 2 and L.KV_QUERIES == 2 * 4 * 4


def test_neighbourhood_from_scores():
    keys = ("noisy_knn_accuracy", "noisy_to_clean_accuracy", "clean_to_noisy_accuracy")
    a = dict(zip(keys, (50.0, 40.0, 45.5)))
    b = dict(zip(keys, (62.5, 55.0, 44.0)))
    r = E.neighbourhood_from_scores(a, b)
    assert r["initial_weights"] == a and r["trained_weights"] == b
    assert r["improvement"] == {"noisy_knn_accuracy_change": 12.5, "noisy_to_clean_accuracy_change": 15.0,
                                "clean_to_noisy_accuracy_change": -1.5}
    assert all(type(v) is float for block in r.values() for v in block.values())
    assert PKG.knn is E.knn and PKG.trustworthiness is E.trustworthiness and PKG.knn_store is E.knn_store
