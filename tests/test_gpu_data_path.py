"""The device data path on the MI355X against tests/data_path.py: data.py (FeatureStore, StoreFeats, DeviceLoader), the
three kernels of csrc/collate.hip through the C ABI, and the in-place row loaders of the store-fed consumers, read
through a read-out network.  Every comparison is an equality of bit patterns.  Every output buffer handed to a kernel
is pre-filled with a sentinel (0xA5 pad bytes, -7 labels / rows / lens, the NaN 0x7FA5A5A5 for features) and carries
64 guard elements that must come back unchanged; a refusal must leave the whole buffer unchanged.

Store address arithmetic, read before section 4 was written (every store consumer; none is a 32-bit product):
  collate.hip:38,52,70      (size_t)frame * (DAD_D / 4) + lane on a 16-B / 8-B vector pointer, frame = offsets[s] + t
                            (long); collate.hip:108 (size_t)r * (DAD_D / 4) on the output
  dad_common.h:142-146      dad_src_row returns size_t: (size_t)(base[b] + min(t, max(len, 1) - 1)), base int64
  dad_prep.h:149-157        size_t srow (dad_src_row, or the readlane pair rebuilt as uint64); x + srow * DAD_D + 4 lane
  dad_prep.h:291-306        dad_clean_src_row returns size_t; a.xc + row * DAD_D + 4 lane
  wgrad_direct.h:275-277    size_t srow; the buffer resource is based at a.xc + srow * DAD_D (64-bit pointer), the
                            32-bit offsets behind it (wgrad_direct.h:421) stay inside one 8-row block
  wgrad_f32.hip:65          X[dad_src_row(...) * DAD_D + d]: size_t
  encode.hip:233            (a.xn | a.xc) + dad_src_row(...) * DAD_D: size_t
  eval_split.hip:87, eval_windows.hip:145, eval_noise.hip:99, input_grad.hip:143
                            size_t row = (size_t)(a.rows[u] + (int64_t)t); row * DAD_D + 8 kh | 4 kh: size_t
  eval_models.hip:181-191   size_t r0, r1 from a.rows[u] + (int64_t)t; r * DAD_D + 8 kh: size_t
  attribution.hip:241-247   int64_t row0 = a.rows[u] + (int64_t)c * DAD_SLAB; row * DAD_D: size_t; the 32-bit
                            at_store_elem index (attribution.hip:372) is relative to the slab's own pointer
  eval_rows.h:20-65         Raw4 / Raw8 ::load(base, size_t el): typed pointer + el

The module prints one JSON line of what it compared when it is done (profiles/data_path.json)."""
import ctypes
import functools
import gc
import json

import numpy as np
import pytest
import torch

import dadpkg
import data_path as P
import gpu_harness as gh
from oracle import dad_oracle
from oracle import data_oracle as do

pytestmark = pytest.mark.gpu
PKG = dadpkg.pkg()
D = PKG.data
E = PKG.evaluate
LIB = PKG._lib
TORCH_DT = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}
COUNTS = {}


def _count(key, n):
    COUNTS[key] = COUNTS.get(key, 0) + int(n)


# ---- sentinel buffers ----------------------------------------------------------------------------------------------------
class Out:
    """An output buffer of n elements and 64 guard elements, all set to the sentinel of its kind."""
    KINDS = {"pad": (torch.uint8, P.PAD_SENTINEL), "i64": (torch.int64, P.INT_SENTINEL),
             "i32": (torch.int32, P.INT_SENTINEL), "feats": (torch.int32, P.FEAT_SENTINEL)}

    def __init__(self, kind, n):
        dtype, self.fill = self.KINDS[kind]
        self.n = int(n)
        self.t = torch.full((self.n + P.GUARD,), self.fill, dtype=dtype, device="cuda")

    @property
    def ptr(self):
        return ctypes.c_void_p(self.t.data_ptr())

    def result(self):
        """The n elements (features as uint32 patterns); the guard must hold the sentinel."""
        torch.cuda.synchronize()
        a = self.t.cpu().numpy()
        assert (a[self.n:] == self.fill).all(), "guard overwritten"
        a = a[:self.n]
        return a.view(np.uint32) if a.dtype == np.int32 and self.fill == P.FEAT_SENTINEL else a

    def untouched(self):
        torch.cuda.synchronize()
        return bool((self.t == self.fill).all())


def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _dev(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dtype).cuda()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _collate(st, index, T, labelled=True, n_samples=None):
    """dad_collate through the C ABI into sentinel buffers: {'feats' uint32 [B][T][768], 'pad', 'labels'}."""
    index = np.asarray(index, np.int64)
    B = len(index)
    feats, pad = Out("feats", B * T * P.DIM), Out("pad", B * T)
    lab = Out("i64", B) if labelled else None
    idx = _dev(index, torch.int64)
    rc = LIB.lib().dad_collate(_p(st.feats), D.STORE_DTYPES[st.feats.dtype], _p(st.offsets_d), _p(st.sizes_d),
                               len(st) if n_samples is None else n_samples, _p(idx), B, T, feats.ptr, pad.ptr,
                               _p(st.labels_d) if labelled else None, lab.ptr if labelled else None, _stream())
    assert rc == 0
    return {"feats": feats.result().reshape(B, T, P.DIM), "pad": pad.result().reshape(B, T),
            "labels": lab.result() if labelled else None}


def _collate_index(st, index, T, labelled=True):
    index = np.asarray(index, np.int64)
    B = len(index)
    rows, lens, pad = Out("i64", B), Out("i32", B), Out("pad", B * T)
    lab = Out("i64", B) if labelled else None
    idx = _dev(index, torch.int64)
    rc = LIB.lib().dad_collate_index(_p(st.offsets_d), _p(st.sizes_d), len(st), _p(idx), B, T, rows.ptr, lens.ptr,
                                     pad.ptr, _p(st.labels_d) if labelled else None, lab.ptr if labelled else None,
                                     _stream())
    assert rc == 0
    return {"rows": rows.result(), "lens": lens.result(), "pad": pad.result().reshape(B, T),
            "labels": lab.result() if labelled else None}


def _same(got, want, what):
    assert set(got) == set(want), what
    for k in want:
        if want[k] is None:
            assert got[k] is None, (what, k)
        else:
            assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, (what, k)
            bad = np.flatnonzero(got[k].reshape(-1) != want[k].reshape(-1))
            assert bad.size == 0, "%s: %s differs at %d of %d, first at %d: got %s want %s" % (
                what, k, bad.size, want[k].size, bad[0], got[k].reshape(-1)[bad[0]], want[k].reshape(-1)[bad[0]])
            _count("edge_values_compared", want[k].size)


# ---- stores --------------------------------------------------------------------------------------------------------------
def _bits_tensor(bits, dt):
    """Store elements from their bit patterns, through a view (no float conversion touches them)."""
    if dt == "f32":
        return torch.from_numpy(np.ascontiguousarray(bits, np.uint32).view(np.int32).copy()).view(torch.float32)
    return torch.from_numpy(np.ascontiguousarray(bits, np.uint16).view(np.int16).copy()).view(TORCH_DT[dt])


def _check_upload(st, bits):
    w = torch.int32 if st.feats.dtype == torch.float32 else torch.int16
    assert np.array_equal(st.feats.view(w).cpu().numpy().view(bits.dtype), bits)


@functools.lru_cache(None)
def _pattern_store(dt):
    sizes, offsets, _ = P.pattern_layout()
    st = D.FeatureStore(_bits_tensor(P.pattern_store(), dt), sizes, offsets, np.arange(len(sizes)) % 4)
    assert st.feats.dtype == TORCH_DT[dt]
    _check_upload(st, P.pattern_store())
    return st


@functools.lru_cache(None)
def _edge(dt, variant="base"):
    feats, sizes, offsets, labels = P.edge_store()
    if variant == "base":
        return D.FeatureStore(feats.copy(), sizes, offsets, labels, dtype=TORCH_DT[dt])
    if variant == "unlabelled":
        return _edge(dt).subset(np.arange(len(sizes)), with_labels=False)
    return _edge(dt).subset(P.edge_subset())


def _edge_host(variant):
    feats, sizes, offsets, labels = P.edge_store()
    if variant == "subset":
        s = P.edge_subset()
        return feats.view(np.uint32), sizes[s], offsets[s], labels[s]
    return feats.view(np.uint32), sizes, offsets, (labels if variant == "base" else None)


@pytest.fixture(scope="module", autouse=True)
def _report_and_release():
    yield
    print("\ndata_path compared: " + json.dumps(COUNTS, sort_keys=True))
    torch.cuda.synchronize()
    for f in (_pattern_store, _edge, _probe_store, _readout_flats, _eval_readout, _models_readout, _train_readout):
        f.cache_clear()
    gc.collect()
    torch.cuda.empty_cache()
    torch.cuda.synchronize()


@pytest.fixture(autouse=True)
def _stop_at_a_fault():
    """A device error ends the module: nothing more is launched on a card that has reported one."""
    yield
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit("the device reported an error, nothing more is run on it: %s" % e, returncode=3)


# ---- 1. every 16-bit pattern through dad_collate ---------------------------------------------------------------------------
def _check_wide(got, want, dt, what):
    """bf16: every pattern bit-equal, NaNs included.  fp16: every non-NaN pattern bit-equal; a NaN pattern gives a NaN
    (payloads are not compared), and not the sentinel."""
    assert got.shape == want.shape and got.dtype == want.dtype == np.uint32
    nan = ~P.finite32(want) & (want & np.uint32(0x7FFFFF) != 0)
    if dt == "bf16":
        assert np.array_equal(got, want), what
    else:
        bad = np.flatnonzero((got != want) & ~nan)
        assert bad.size == 0, "%s: %d patterns differ, first at %d: got %08x want %08x" % (
            what, bad.size, bad[0], got.reshape(-1)[bad[0]], want.reshape(-1)[bad[0]])
        g = got[nan]
        assert (~P.finite32(g) & (g & np.uint32(0x7FFFFF) != 0)).all() and (g != P.FEAT_SENTINEL).all(), what
    _count("collate_elements_bit_equal_%s" % dt, (~nan).sum() if dt == "f16" else want.size)
    _count("collate_nan_elements_%s" % dt, nan.sum())


@pytest.mark.parametrize("dt", ["f16", "bf16"])
def test_every_pattern_through_collate(dt):
    st = _pattern_store(dt)
    sizes, offsets, batches = P.pattern_layout()
    wide = P.widen(P.pattern_store(), dt)
    seen = np.zeros(P.PATTERN_FRAMES, bool)
    for b in batches:
        T = int(sizes[b].max())
        want = P.ref_collate(wide, sizes, offsets, st.labels, b, T)
        got = _collate(st, b, T)
        _check_wide(got["feats"], want["feats"], dt, "batch %s" % b)
        assert np.array_equal(got["pad"], want["pad"]) and np.array_equal(got["labels"], want["labels"])
        for s in b:
            seen[offsets[s]:offsets[s] + sizes[s]] = True
    assert seen.all()


@pytest.mark.parametrize("dt", ["f16", "bf16"])
def test_every_pattern_through_materialize(dt):
    st = _pattern_store(dt)
    sizes, offsets, batches = P.pattern_layout()
    wide = P.widen(P.pattern_store(), dt)
    for b in batches:
        batch = st.batch_index(b)
        f = batch["net_input"]["feats"]
        assert isinstance(f, D.StoreFeats)
        x = f.materialize()
        assert x.dtype == torch.float32 and tuple(x.shape) == tuple(f.shape)
        got = x.view(torch.int32).cpu().numpy().view(np.uint32)
        _check_wide(got, P.ref_collate(wide, sizes, offsets, None, b, int(sizes[b].max()))["feats"], dt, "batch %s" % b)


# ---- 2. the three kernels at their edges -----------------------------------------------------------------------------------
VARIANTS = ("base", "unlabelled", "subset")


@pytest.mark.parametrize("B,T", P.COLLATE_SHAPES, ids=["%dx%d" % s for s in P.COLLATE_SHAPES])
@pytest.mark.parametrize("dt", P.STORES)
def test_collate_edges(dt, B, T):
    for variant in VARIANTS:
        wide, sizes, offsets, labels = _edge_host(variant)
        caps = (None, 5) if (B, T) == (5, 7) else (None, 7) if (B, T) == (2, 300) else (None,)
        for cap in caps:                                   # cap: T above the batch's longest sample
            index = P.edge_index(sizes, B, T, cap)
            want = P.ref_collate(wide, sizes, offsets, labels, index, T)
            got = _collate(_edge(dt, variant), index, T, labelled=labels is not None)
            _same(got, want, "%s %s %dx%d cap %s" % (dt, variant, B, T, cap))
    if T == 300:
        assert (_edge_host("base")[1][P.edge_index(_edge_host("base")[1], B, T)] == 300).any()


@pytest.mark.parametrize("dt", P.STORES)
def test_collate_out_of_range_indices(dt):
    wide, sizes, offsets, labels = _edge_host("base")
    index = P.with_out_of_range([5, 3, 17, 0, 2], len(sizes))
    assert {-1, len(sizes), 2 ** 40, P.INT64_MIN} <= set(index.tolist())
    for lab in (labels, None):
        st = _edge(dt, "base" if lab is not None else "unlabelled")
        _same(_collate(st, index, 9, labelled=lab is not None), P.ref_collate(wide, sizes, offsets, lab, index, 9),
              "%s out of range" % dt)


def _refusals(call, outs, good):
    """call(**args) with one argument of `good` replaced at a time: each must be refused with the given code and
    leave every output buffer as it was."""
    cases = [(k, None, LIB.E_ARG) for k, v in good.items() if isinstance(v, ctypes.c_void_p) and k not in
             ("labels_in", "labels_out", "stream")]
    cases += [("labels_in", None, LIB.E_ARG), ("labels_out", None, LIB.E_ARG)]
    for k in ("B", "T", "n", "n_samples"):
        if k in good:
            cases += [(k, 0, LIB.E_SHAPE), (k, -1, LIB.E_SHAPE)]
    if "dtype" in good:
        cases += [("dtype", 3, LIB.E_ARG), ("dtype", -1, LIB.E_ARG)]
    for k, v, code in cases:
        args = dict(good)
        args[k] = v
        assert call(*args.values()) == code, (k, v)
        assert all(o.untouched() for o in outs), (k, v)
    return len(cases)


def test_collate_refusals():
    st = _edge("f32")
    B, T = 3, 9
    idx = _dev([5, 3, 0], torch.int64)
    feats, pad, lab = Out("feats", B * T * P.DIM), Out("pad", B * T), Out("i64", B)
    good = dict(store=_p(st.feats), dtype=0, offsets=_p(st.offsets_d), sizes=_p(st.sizes_d), n_samples=len(st),
                index=_p(idx), B=B, T=T, feats=feats.ptr, pad=pad.ptr, labels_in=_p(st.labels_d), labels_out=lab.ptr,
                stream=_stream())
    assert _refusals(LIB.lib().dad_collate, (feats, pad, lab), good) == 6 + 2 + 6 + 2


@pytest.mark.parametrize("B,T", P.INDEX_SHAPES, ids=["%dx%d" % s for s in P.INDEX_SHAPES])
def test_collate_index_edges(B, T):
    for variant in VARIANTS:
        _, sizes, offsets, labels = _edge_host(variant)
        index = P.edge_index(sizes, B, T)
        want = P.ref_collate_index(sizes, offsets, labels, index, T)
        got = _collate_index(_edge("f32", variant), index, T, labelled=labels is not None)
        _same(got, want, "%s %dx%d" % (variant, B, T))


def test_collate_index_out_of_range_and_the_empty_sample_at_the_end():
    _, sizes, offsets, labels = _edge_host("base")
    index = P.with_out_of_range([5, 3, 17, 1, 2], len(sizes))
    for lab in (labels, None):
        st = _edge("f32", "base" if lab is not None else "unlabelled")
        got = _collate_index(st, index, 9, labelled=lab is not None)
        _same(got, P.ref_collate_index(sizes, offsets, lab, index, 9), "out of range")
        at_end = int(np.flatnonzero(index == 17)[0])
        assert offsets[17] == st.feats.shape[0] and got["rows"][at_end] == 0 and got["lens"][at_end] == 0


def test_collate_index_refusals():
    st = _edge("f32")
    B, T = 3, 9
    idx = _dev([5, 3, 0], torch.int64)
    rows, lens, pad, lab = Out("i64", B), Out("i32", B), Out("pad", B * T), Out("i64", B)
    good = dict(offsets=_p(st.offsets_d), sizes=_p(st.sizes_d), n_samples=len(st), index=_p(idx), B=B, T=T,
                rows=rows.ptr, lens=lens.ptr, pad=pad.ptr, labels_in=_p(st.labels_d), labels_out=lab.ptr,
                stream=_stream())
    assert _refusals(LIB.lib().dad_collate_index, (rows, lens, pad, lab), good) == 6 + 2 + 6


def _epoch_call(st, ep, labelled, n=None):
    n = len(ep["index"]) if n is None else n
    rows, lens, pad = Out("i64", len(ep["index"])), Out("i32", len(ep["index"])), Out("pad", int(ep["pad_T"].sum()))
    lab = Out("i64", len(ep["index"])) if labelled else None
    dev = [_dev(ep[k], torch.int64) for k in ("index", "pad_off", "pad_T")]
    rc = LIB.lib().dad_collate_index_epoch(_p(st.offsets_d), _p(st.sizes_d), len(st), _p(dev[0]), n, _p(dev[1]),
                                           _p(dev[2]), rows.ptr, lens.ptr, pad.ptr,
                                           _p(st.labels_d) if labelled else None, lab.ptr if labelled else None,
                                           _stream())
    return rc, (rows, lens, pad) + ((lab,) if labelled else ())


@pytest.mark.parametrize("labelled", [True, False])
def test_collate_index_epoch_c_abi(labelled):
    _, sizes, offsets, labels = _edge_host("base" if labelled else "unlabelled")
    st = _edge("f32", "base" if labelled else "unlabelled")
    for batches in (P.edge_epoch(), [[15]], [[17]], [[-1]]):               # the epoch; n = 1: long, empty, out of range
        ep = P.ref_collate_index_epoch(sizes, offsets, labels, batches, Ts=None if len(batches) > 1 else [513])
        rc, outs = _epoch_call(st, ep, labelled)
        assert rc == 0
        got = {"rows": outs[0].result(), "lens": outs[1].result(), "pad": outs[2].result(),
               "labels": outs[3].result() if labelled else None}
        _same(got, {k: ep[k] for k in got}, "epoch of %d batches" % len(batches))
    ep = P.ref_collate_index_epoch(sizes, offsets, labels, P.edge_epoch())
    assert tuple(ep["T"][:5]) == (1, 255, 256, 257, 513) and (ep["lens"][ep["pad_T"] > 0] == 0).any()
    for n in (0, -1, 2 ** 31 + 1):                                          # refusals: nothing is written
        rc, outs = _epoch_call(st, ep, labelled, n=n)
        assert rc == LIB.E_SHAPE and all(o.untouched() for o in outs), n


def test_collate_index_epoch_refusals():
    st = _edge("f32")
    _, sizes, offsets, labels = _edge_host("base")
    ep = P.ref_collate_index_epoch(sizes, offsets, labels, P.edge_epoch())
    n = len(ep["index"])
    dev = [_dev(ep[k], torch.int64) for k in ("index", "pad_off", "pad_T")]
    rows, lens, pad, lab = Out("i64", n), Out("i32", n), Out("pad", int(ep["pad_T"].sum())), Out("i64", n)
    good = dict(offsets=_p(st.offsets_d), sizes=_p(st.sizes_d), n_samples=len(st), index=_p(dev[0]), n=n,
                pad_off=_p(dev[1]), pad_T=_p(dev[2]), rows=rows.ptr, lens=lens.ptr, pad=pad.ptr,
                labels_in=_p(st.labels_d), labels_out=lab.ptr, stream=_stream())
    assert _refusals(LIB.lib().dad_collate_index_epoch, (rows, lens, pad, lab), good) == 8 + 2 + 4


@pytest.mark.parametrize("with_labels", [True, False])
@pytest.mark.parametrize("style", ["iemocap", "casia"])
@pytest.mark.parametrize("drop_last", [False, True])
def test_fused_loader_epochs_against_the_reference(drop_last, style, with_labels):
    """Two shuffled epochs of DeviceLoader(fused=True) over sizes that include 256, 257 and 513: every batch's rows,
    lens, pad, labels and ids against ref_collate_index on the batches torch's own DataLoader draws from the same
    generator seed (not against batch_index)."""
    sizes = np.array(P.LOADER_SIZES, np.int64)
    offsets = np.concatenate([[0], np.cumsum(sizes + 1)[:-1]]).astype(np.int64)
    labels = np.arange(len(sizes)) % 4
    feats = P.edge_values(np.arange(int(offsets[-1] + sizes[-1]))[:, None], np.arange(P.DIM)[None, :])
    st = D.FeatureStore(feats, sizes, offsets, labels)
    g, g_ref = torch.Generator(), torch.Generator()
    g.manual_seed(11)
    g_ref.manual_seed(11)
    loader = D.DeviceLoader(st, batch_size=4, shuffle=True, generator=g, drop_last=drop_last, style=style,
                            with_labels=with_labels, fused=True)
    ref_loader = torch.utils.data.DataLoader(range(len(sizes)), batch_size=4, shuffle=True, generator=g_ref,
                                             drop_last=drop_last, collate_fn=lambda b: b)
    lab = labels if with_labels else None
    orders = []
    for epoch in range(2):
        want_batches = [np.asarray(b, np.int64) for b in ref_loader]
        got_batches = list(loader)
        assert len(got_batches) == len(want_batches) == (2 if drop_last else 3)
        orders.append(np.concatenate(want_batches).tolist())
        for batch, index in zip(got_batches, want_batches):
            T = int(sizes[index].max())
            want = P.ref_collate_index(sizes, offsets, lab, index, T)
            f = batch["net_input"]["feats"]
            assert isinstance(f, D.StoreFeats) and tuple(f.shape) == (len(index), T, P.DIM)
            got = {"rows": f.rows.cpu().numpy(), "lens": f.lens.cpu().numpy(),
                   "pad": batch["net_input"]["padding_mask"].view(torch.uint8).cpu().numpy(),
                   "labels": batch["labels"].cpu().numpy() if batch.get("labels") is not None else None}
            _same(got, want, "epoch %d" % epoch)
            assert np.array_equal(f.index, index) and np.array_equal(f.index_d.cpu().numpy(), index)
            if style == "iemocap":
                assert np.array_equal(batch["id"].cpu().numpy(), index) and "labels" in batch
            else:
                assert "id" not in batch and ("labels" in batch) == with_labels
    assert orders[0] != orders[1]
    if not drop_last:
        assert sorted(orders[0]) == sorted(orders[1]) == list(range(len(sizes))) and {256, 257, 513} <= set(sizes.tolist())


# ---- 3. store rows as the consumers see them -------------------------------------------------------------------------------
PARTS = ("normal", "subnormal")


@functools.lru_cache(None)
def _probe_store(dt, precision, limit=None):
    """The probe store of (dt, precision): 1024 utterances of one frame, labels 0 .. 3."""
    bits, _, _ = P.probe(dt, precision, limit)
    n = P.PATTERN_FRAMES
    st = D.FeatureStore(_bits_tensor(bits, dt), np.ones(n, np.int64), np.arange(n), np.arange(n) % 4)
    _check_upload(st, bits)
    return st


@functools.lru_cache(None)
def _readout_flats():
    return tuple(torch.from_numpy(gh.flat(P.readout_params(g, s))).cuda() for g, s in P.READOUT)


def _readout_model(k_student, k_teacher):
    model = PKG.SSRLModel().cuda()
    with torch.no_grad():
        model.student_flat.copy_(_readout_flats()[k_student])
        model.teacher_flat.copy_(_readout_flats()[k_teacher])
    return model


def _bits_of(t):
    return t.detach().contiguous().view(torch.int32).cpu().numpy().view(np.uint32)


@functools.lru_cache(None)
def _eval_readout(dt, precision):
    """dad_eval_split's embeddings of the six read-out networks (student: sign +, teacher: sign -, per column group):
    uint32 [6][1024][256], and the logits."""
    st = _probe_store(dt, precision)
    emb, logits = [None] * 6, []
    for g in range(3):
        res = E.evaluate_store(_readout_model(2 * g, 2 * g + 1), st, use_teacher=True, precision=precision,
                               outputs=("emb", "t_emb", "logits", "t_logits"))
        emb[2 * g], emb[2 * g + 1] = _bits_of(res["emb"]), _bits_of(res["t_emb"])
        logits += [_bits_of(res["logits"]), _bits_of(res["t_logits"])]
        assert res["n_nonfinite"] == 0 and res["n"] == P.PATTERN_FRAMES
    return np.stack(emb), np.stack(logits)


@functools.lru_cache(None)
def _models_readout(dt, precision):
    """dad_eval_models: the six networks as six checkpoints in one pass."""
    res = E.evaluate_models_store(list(_readout_flats()), _probe_store(dt, precision), precision=precision,
                                  outputs=("emb", "logits"))
    assert not res["nonfinite"].any()
    return _bits_of(res["emb"]), _bits_of(res["logits"])


def _check_readout(got, logits, dt, precision, part, what, limit=None):
    """got uint32 [6][1024][256] against relu(+-operand), bit for bit, on the elements whose operand is (part
    'subnormal') or is not ('normal') subnormal in the GEMM's operand type; the logits are b2."""
    _, ops, covered = P.probe(dt, precision, limit)
    sub = P.subnormal_operand(ops, precision)
    n_bad, first, flushed = 0, None, 0
    for k, (g, s) in enumerate(P.READOUT):
        want = P.readout_expected(ops, g, s)
        sel = sub[:, 256 * g:256 * (g + 1)] == (part == "subnormal")
        bad = (got[k] != want) & sel
        n_bad += int(bad.sum())
        flushed += int((bad & (got[k] & np.uint32(0x7FFFFFFF) == 0)).sum())
        if first is None and bad.any():
            f, h = np.argwhere(bad)[0]
            first = "network %d frame %d unit %d: got %08x want %08x" % (k, f, h, got[k][f, h], want[f, h])
        _count("readout_%s_%s" % (what, part), sel.sum())
    print("%s %s store at %s, %s operands: %d differ (%d of them returned as +-0); %s" % (
        what, dt, precision, part, n_bad, flushed, first))
    assert n_bad == 0, "%d differ, %d of them +-0 for a subnormal operand; first: %s" % (n_bad, flushed, first)
    if logits is not None:
        b2 = np.asarray(P.readout_params(0, 1.0)[3], np.float32).view(np.uint32)
        assert (logits.reshape(-1, 4) == b2).all()
    assert covered.any()


@pytest.mark.parametrize("part", PARTS)
@pytest.mark.parametrize("dt", P.STORES)
@pytest.mark.parametrize("precision", ["fp32", "fp16"])
def test_eval_split_reads_every_pattern(precision, dt, part):
    emb, logits = _eval_readout(dt, precision)
    _check_readout(emb, logits, dt, precision, part, "eval_split")


@pytest.mark.parametrize("part", PARTS)
@pytest.mark.parametrize("dt", P.STORES)
@pytest.mark.parametrize("precision", ["fp32", "fp16"])
def test_eval_models_reads_every_pattern(precision, dt, part):
    emb, logits = _models_readout(dt, precision)
    _check_readout(emb, logits, dt, precision, part, "eval_models")
    assert np.array_equal(emb, _eval_readout(dt, precision)[0])            # each model's dad_eval_split outputs


TRAIN_B = 64
TRAIN_LIMIT = 256.0


@functools.lru_cache(None)
def _train_readout(dt, precision, ragged):
    """One train step past warm-up per batch of 64 one-frame utterances and per read-out pair (explicit draws: zero
    noise, u = 1, every dropout unit kept): the clean student embedding reads the clean rows, the teacher's embedding
    of the weak rows (x + 0) the noisy rows.  Student and teacher take opposite signs of one column group; the
    weights are reloaded before every step (the step updates them).  uint32 [2][6][1024][256]: clean, weak."""
    st = _probe_store(dt, precision, TRAIN_LIMIT)
    n, B = P.PATTERN_FRAMES, TRAIN_B
    cfg = dad_oracle.make_cfg("iemocap")
    model = PKG.SSRLModel().cuda()
    step = PKG.DADStep(model, PKG.ConfigView(cfg, flavor="iemocap"), precision=precision, rng="explicit", seed=3,
                       ragged=ragged)
    zeros = torch.zeros(B, 1, P.DIM, device="cuda")
    draws = {"nw": zeros, "ns": zeros, "u": torch.ones(P.DIM, device="cuda"),
             "start": torch.zeros(B, dtype=torch.int64, device="cuda"),
             "keep1": torch.ones(B, 256, dtype=torch.bool, device="cuda"),
             "keep2": torch.ones(B, 256, dtype=torch.bool, device="cuda")}
    out = np.zeros((2, 6, n, 256), np.uint32)
    flats = _readout_flats()
    for ks, kt in ((0, 1), (1, 0), (2, 3), (3, 2), (4, 5), (5, 4)):
        clean, weak = [], []
        for r0 in range(0, n, B):
            idx = np.arange(r0, r0 + B)
            with torch.no_grad():
                model.student_flat.copy_(flats[ks])
                model.teacher_flat.copy_(flats[kt])
            step.refresh_shadow()
            step.step(st.batch_index(idx), st.batch_index(idx, with_labels=False), 60, draws=draws)
            o = step.outputs(B, B)
            clean.append(o["e_clean"].clone())
            weak.append(o["e_teacher"].clone())
        out[0, ks] = _bits_of(torch.cat(clean))
        out[1, kt] = _bits_of(torch.cat(weak))
    torch.cuda.synchronize()
    return out


TRAIN_CASES = [(p, dt, rg) for p in ("fp32", "fp16", "bf16") for dt in P.STORES for rg in (False, True)
               if not (rg and p == "fp32")]


@pytest.mark.parametrize("part", PARTS)
@pytest.mark.parametrize("precision,dt,ragged", TRAIN_CASES,
                         ids=["%s-%s-%s" % (p, dt, "ragged" if rg else "dense") for p, dt, rg in TRAIN_CASES])
def test_train_step_reads_every_pattern(precision, dt, ragged, part):
    got = _train_readout(dt, precision, ragged)
    _check_readout(got[0], None, dt, precision, part, "train_clean", TRAIN_LIMIT)
    _check_readout(got[1], None, dt, precision, part, "train_weak", TRAIN_LIMIT)


# ---- 4. stores past 2^31 elements and 2^32 bytes ---------------------------------------------------------------------------
def _install(feats, sizes, offsets, labels):
    st = D.FeatureStore.__new__(D.FeatureStore)
    st.feats = feats
    st._init_index(D._device(None), np.asarray(sizes, np.int64), np.asarray(offsets, np.int64), labels)
    return st


def _big_pair(dt):
    """(big store, compact store): the same utterances at the layout's rows of a zeroed store past the boundary, and
    packed into a few rows."""
    sizes, offsets = P.big_layout(dt)
    csizes, coffsets, cframes = P.compact_layout(dt)
    labels = np.arange(len(sizes)) % 4
    big = torch.empty(P.BIG[dt]["frames"], P.DIM, dtype=TORCH_DT[dt], device="cuda")
    big.zero_()
    small = torch.zeros(cframes, P.DIM, dtype=TORCH_DT[dt], device="cuda")
    for k in range(len(sizes)):
        rows = torch.from_numpy(P.big_rows(dt, k)).to(TORCH_DT[dt]).cuda()
        big[int(offsets[k]):int(offsets[k] + sizes[k])] = rows
        small[int(coffsets[k]):int(coffsets[k] + sizes[k])] = rows
    assert (big.numel() if dt == "f16" else big.numel() * big.element_size()) > P.BIG[dt]["wrap"]
    return _install(big, sizes, offsets, labels), _install(small, csizes, coffsets, labels)


def _store_step(clean_st, noisy_st, ragged):
    from oracle import synth
    import test_gpu_store16 as T16
    cfg = dad_oracle.make_cfg("iemocap")
    step = PKG.DADStep(PKG.SSRLModel().cuda(), PKG.ConfigView(cfg, flavor="iemocap"), precision="fp16",
                       rng="counter", seed=9, ragged=ragged)
    gh.load_state(step, synth.make_state(40, 1))
    idx = np.arange(len(clean_st))
    losses = step.step(clean_st.batch_index(idx), noisy_st.batch_index(idx[::-1].copy(), with_labels=False), 60)
    return T16._snapshot(step, losses, len(idx), len(idx))


@pytest.mark.parametrize("dt", ["f16", "f32"])
def test_store_past_the_32_bit_boundary(dt):
    """dad_collate, dad_collate_index, dad_eval_split (fp32, fp16) and one store-fed fp16 train step (dense, ragged) on
    utterances below, across and above element 2^31 (fp16) / byte 2^32 (f32) of the store equal the same calls on a
    compact store of the same utterances, bit for bit; dad_collate equals the formula as well."""
    big, small = _big_pair(dt)
    try:
        sizes, offsets = P.big_layout(dt)
        index = np.array([4, 2, 0, 3, 1, 2], np.int64)
        T = int(sizes.max())
        a, b = _collate(big, index, T), _collate(small, index, T)
        _same(a, b, "collate")
        wide = np.zeros((int(small.feats.shape[0]), P.DIM), np.uint32)
        for k in range(len(sizes)):
            wide[small.offsets[k]:small.offsets[k] + sizes[k]] = P.big_rows(dt, k).view(np.uint32)
        _same(a, P.ref_collate(wide, small.sizes, small.offsets, small.labels, index, T), "collate against the formula")
        assert all(a["feats"][i, :sizes[s]].any(axis=1).all() for i, s in enumerate(index))
        ia, ib = _collate_index(big, index, T), _collate_index(small, index, T)
        assert np.array_equal(ia["rows"], offsets[index]) and ia["rows"].max() > P.BIG[dt]["boundary"]
        for k in ("lens", "pad", "labels"):
            assert np.array_equal(ia[k], ib[k]), k
        student, teacher = do.eval_weights(7)
        model = PKG.SSRLModel().cuda()
        with torch.no_grad():
            model.student_flat.copy_(torch.from_numpy(gh.flat(student)))
            model.teacher_flat.copy_(torch.from_numpy(gh.flat(teacher)))
        names = ("emb", "logits", "probs", "score", "pred", "t_emb", "t_logits", "t_pred")
        for precision in ("fp32", "fp16"):
            ra = E.evaluate_store(model, big, use_teacher=True, precision=precision, outputs=names)
            rb = E.evaluate_store(model, small, use_teacher=True, precision=precision, outputs=names)
            for k in names:
                assert torch.equal(ra[k].contiguous().view(torch.uint8), rb[k].contiguous().view(torch.uint8)), k
            assert ra["emb"].abs().sum(1).min() > 0
            _count("big_store_eval_outputs", len(names))
        for ragged in (False, True):
            sa, sb = _store_step(big, big, ragged), _store_step(small, small, ragged)
            assert set(sa) == set(sb)
            for k in sa:
                np.testing.assert_array_equal(sa[k], sb[k], err_msg="%s ragged=%s" % (k, ragged))
            _count("big_store_step_outputs", len(sa))
    finally:
        for st in (big, small):
            st.feats = None
            st._eval_plan = None
        del big, small
        gc.collect()
        torch.cuda.empty_cache()
