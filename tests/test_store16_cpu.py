"""fp16 / bf16 feature stores read in place by the 16-bit train step (ABI 10), the parts that need no
GPU: the two dtype fields of dad_batch, the host plan for a next batch on 16-bit stores (the same
launches as for f32 stores), and the step's predicate for handing a store through without a copy."""
import ctypes

import pytest
import torch

import dadpkg
from test_step_plan_cpu import _cfg, _next, _plan

PKG = dadpkg.pkg()
LIB = PKG._lib
S = PKG.step


def _store_next(cfg, xc_dtype, xn_dtype, **kw):
    ncfg, nbt = _next(cfg, store=True, **kw)
    nbt.xc_dtype, nbt.xn_dtype = xc_dtype, xn_dtype
    return ncfg, nbt


def test_dad_batch_has_the_dtype_fields():
    names = [n for n, _ in LIB.DadBatch._fields_]
    assert names[-3:] == ["lenn", "xc_dtype", "xn_dtype"]
    assert LIB.DadBatch.xc_dtype.size == LIB.DadBatch.xn_dtype.size == 4
    assert LIB.DadBatch.xn_dtype.offset == LIB.DadBatch.xc_dtype.offset + 4
    bt = LIB.DadBatch()
    assert (bt.xc_dtype, bt.xn_dtype) == (LIB.STORE_F32, LIB.STORE_F32)      # zero-initialised = an f32 batch
    assert (LIB.STORE_F32, LIB.STORE_F16, LIB.STORE_BF16) == tuple(PKG.data.STORE_DTYPES[t] for t in
                                                                   (torch.float32, torch.float16, torch.bfloat16))
    assert LIB.DAD_ABI_VERSION == LIB.lib().dad_abi_version() == 10


@pytest.mark.parametrize("shape", [dict(B=5, T=37, Bn=3, Tn=41), dict(B=64, T=300, Bn=64, Tn=300)])
@pytest.mark.parametrize("precision", ["fp16", "bf16"])
def test_plan_for_16bit_stores_equals_plan_for_f32_stores(shape, precision):
    c = _cfg(precision=precision, **shape)
    for defer in (0, 1, 2, 3):
        want = _plan(c, _next(c, store=True), defer=defer)
        assert want["prepped"] == 1 and want["pending"] == defer
        if defer == 0:
            assert want["wgrad_store"] == 1 and want["wgrad"].endswith("_cps") and want["tail_prep"] == 2
        for xc, xn in ((LIB.STORE_F16, LIB.STORE_F16), (LIB.STORE_BF16, LIB.STORE_BF16), (LIB.STORE_F16, LIB.STORE_BF16),
                       (LIB.STORE_F32, LIB.STORE_F16), (LIB.STORE_BF16, LIB.STORE_F32)):
            assert _plan(c, _store_next(c, xc, xn), defer=defer) == want, (xc, xn, defer)


def test_plan_refuses_what_the_step_refuses():
    L = LIB.lib()
    info = LIB.DadStepPlanInfo()
    plan = lambda c, nxt: L.dad_step_plan(c, nxt[0], nxt[1], 0, 256, ctypes.byref(info))
    for shape in (dict(B=5, T=37, Bn=3, Tn=41), dict(B=64, T=300, Bn=64, Tn=300)):
        c = _cfg(precision="fp32", **shape)
        assert plan(c, _next(c, store=True)) == 0                              # an f32 store: planned (not ahead)
        assert plan(c, _store_next(c, LIB.STORE_F16, LIB.STORE_F16)) == LIB.E_UNSUPPORTED
        assert plan(c, _store_next(c, LIB.STORE_F32, LIB.STORE_BF16)) == LIB.E_UNSUPPORTED
    c = _cfg()
    ncfg, nbt = _next(c)                                                       # a padded batch is f32
    nbt.xc_dtype = LIB.STORE_F16
    assert plan(c, (ncfg, nbt)) == LIB.E_ARG
    ncfg, nbt = _store_next(c, LIB.STORE_F16, 3)                               # not a DAD_STORE_* value
    assert plan(c, (ncfg, nbt)) == LIB.E_ARG
    ncfg, nbt = _store_next(c, LIB.STORE_F16, LIB.STORE_F32)
    nbt.rown = nbt.lenn = None                                                 # clean store, padded noisy batch
    assert plan(c, (ncfg, nbt)) == 0 and info.prepped == 1
    nbt.xn_dtype = LIB.STORE_F16
    assert plan(c, (ncfg, nbt)) == LIB.E_ARG


class _Store:
    def __init__(self, dtype, device):
        self.feats = torch.empty(4, 768, dtype=dtype, device=device)


def _store_batch(dtype, device=torch.device("cpu")):
    feats = S.StoreFeats.__new__(S.StoreFeats)
    feats.store = _Store(dtype, device)
    return {"net_input": {"feats": feats, "padding_mask": torch.zeros(2, 3, dtype=torch.bool, device=device)},
            "labels": torch.zeros(2, dtype=torch.int64, device=device)}


def test_store_in_place_predicate():
    for prec in (LIB.PREC_FP16, LIB.PREC_BF16):
        for dt in (torch.float32, torch.float16, torch.bfloat16):
            assert S._store_in_place(dt, prec)
        assert not S._store_in_place(torch.float64, prec)
    assert S._store_in_place(torch.float32, LIB.PREC_FP32)
    assert not S._store_in_place(torch.float16, LIB.PREC_FP32)
    assert not S._store_in_place(torch.bfloat16, LIB.PREC_FP32)


def test_16bit_store_batch_is_resident_for_16bit_precisions_only():
    cpu = torch.device("cpu")
    for dt in (torch.float16, torch.bfloat16):
        b = _store_batch(dt)
        assert S._resident(b, cpu, precision=LIB.PREC_FP16)
        assert S._resident(b, cpu, precision=LIB.PREC_BF16)
        assert S._resident(b, cpu, labels=False, precision=LIB.PREC_FP16)
        assert not S._resident(b, cpu, precision=LIB.PREC_FP32)
        assert not S._resident(b, cpu)                                          # (the default is the FP32 step's rule)
        assert not S._resident(b, torch.device("meta"), precision=LIB.PREC_FP16)   # another device: copied
    f = _store_batch(torch.float32)
    assert all(S._resident(f, cpu, precision=p) for p in (LIB.PREC_FP32, LIB.PREC_FP16, LIB.PREC_BF16))
