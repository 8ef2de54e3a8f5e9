"""The step's host plan (csrc/step_plan.h, C ABI dad_step_plan), checked without a GPU: which kernels
each step launches and with which grids.  The GPU tests of these paths assert bit-identical results
with and without preparation ahead, so only this file notices when a batch falls back to another
variant.  The expected values are literals, worked out by hand from the launch rules (dad.h,
DESIGN.md): a change of plan has to change them here."""
import ctypes
import os
import subprocess
import sys

import pytest

import dadpkg

CLEAN, NOISY = 1, 2
# the bench step (fp16, 64x300 / 64x300, 256 CUs, no next batch, rows not prepared ahead)
BENCH = dict(prep_grid=1024, encode="dad_encode_wp_f16", pool_grid=0, tail="dad_tail_ecda_w", tail_grid=29, tail_prep=0,
             tail_prep_clean_only=0, splits=21, max_splits=21, wgrad="dad_wgrad_direct_f16", wgrad_grid=256,
             wgrad_clean=0, wgrad_store=0, reduce="dad_reduce_w", reduce_grid=768, prepped=0, pending=0)
# ... with a padded next batch of the other counter parity
AHEAD = dict(BENCH, tail_grid=256, tail_prep=NOISY, wgrad="dad_wgrad_direct_f16_cp", wgrad_clean=1, prepped=1)


def _cfg(B=64, T=300, Bn=64, Tn=300, epoch=60, precision="fp16", view=None, **kw):
    p = dadpkg.pkg()
    prec = {"fp16": p._lib.PREC_FP16, "bf16": p._lib.PREC_BF16, "fp32": p._lib.PREC_FP32}[precision]
    return p.dad_config_for(p.ConfigView(flavor="iemocap", **(view or {})), B, T, Bn, Tn, epoch, 1, precision=prec, **kw)


def _next(cfg, step=1, store=False, **changes):
    """(next_cfg, next_batch): cfg at counter + step and a padded (or store) batch of made-up addresses."""
    lib = dadpkg.pkg()._lib
    ncfg = lib.DadConfig.from_buffer_copy(cfg)
    ncfg.counter = cfg.counter + step
    for k, v in changes.items():
        setattr(ncfg, k, v)
    nbt = lib.DadBatch()
    names = ("xc", "mc", "yc", "xn", "mn") + (("rowc", "lenc", "rown", "lenn") if store else ())
    for i, name in enumerate(names):
        setattr(nbt, name, 0x1000 * (i + 1))
    return ncfg, nbt


def _plan(cfg, nxt=(None, None), defer=0, cus=256):
    lib = dadpkg.pkg()._lib
    L = lib.lib()
    info = lib.DadStepPlanInfo()
    assert L.dad_step_plan(cfg, nxt[0], nxt[1], defer, cus, ctypes.byref(info)) == 0
    got = {n: getattr(info, n) for n, _ in info._fields_}
    for k in ("encode", "tail", "wgrad", "reduce"):
        got[k] = got[k].decode()
    nt, ns, mj = ctypes.c_int(0), ctypes.c_int(0), ctypes.c_int(0)
    if cfg.precision != lib.PREC_FP32:     # the 16-bit encoder's roles are dad_encoder_ws_plan's
        assert L.dad_encoder_ws_plan(cfg, cus, ctypes.byref(nt), ctypes.byref(ns), ctypes.byref(mj)) == 0
    assert (got.pop("ws_nt"), got.pop("ws_ns")) == (nt.value, ns.value)
    if cfg.precision != lib.PREC_FP32:
        assert got["encode_grid"] == nt.value + ns.value > 0
    return got


def _check(got, want):
    diff = {k: (got[k], v) for k, v in want.items() if got[k] != v}
    assert not diff, diff


def test_bench_step_without_a_next_batch():
    _check(_plan(_cfg()), BENCH)                                              # 1
    c = _cfg()
    c.prepped = 1
    _check(_plan(c), dict(BENCH, prep_grid=0))                                # 2


def test_preparation_ahead_variants():
    c = _cfg()
    _check(_plan(c, _next(c)), AHEAD)                                         # 3
    _check(_plan(c, _next(c, store=True)), dict(AHEAD, wgrad="dad_wgrad_direct_f16_cps", wgrad_store=1))    # 4
    b = _cfg(precision="bf16")
    _check(_plan(b, _next(b), defer=CLEAN),                                   # 5
           dict(AHEAD, encode="dad_encode_wp", wgrad="dad_wgrad_direct", wgrad_clean=0, pending=1))
    _check(_plan(c, _next(c), defer=NOISY), dict(AHEAD, tail_grid=29, tail_prep=0, pending=2))              # 6
    _check(_plan(c, _next(c), defer=CLEAN | NOISY),                           # 7
           dict(AHEAD, tail_grid=29, tail_prep=0, wgrad="dad_wgrad_direct_f16", wgrad_clean=0, pending=3))
    # 10: few CUs: the tail grid is not raised past its own blocks, the noisy rows still ride in it
    _check(_plan(c, _next(c), cus=8), dict(AHEAD, tail_grid=29, prep_grid=32))


def test_next_steps_that_do_not_qualify_are_not_prepared():
    c = _cfg()
    lib = dadpkg.pkg()._lib
    assert _plan(c, _next(c, step=2)) == _plan(c)                             # 8: the same set parity
    assert _plan(c, _next(c, T=301)) == _plan(c)                              # 9: other geometry,
    assert _plan(c, _next(c, precision=lib.PREC_BF16)) == _plan(c)            #    other precision,
    ncfg, nbt = _next(c)
    nbt.mn = 0
    assert _plan(c, (ncfg, nbt)) == _plan(c)                                  #    a missing pointer
    _check(_plan(c, (ncfg, nbt)), BENCH)


def test_other_geometries_and_modes():
    c = _cfg(16, 40, 12, 50)                                                  # 11
    _check(_plan(c), dict(splits=21, tail="dad_tail_ecda_w", tail_grid=10, wgrad_grid=256, prepped=0))
    _check(_plan(c, _next(c)), dict(splits=21, tail_grid=256, tail_prep=NOISY, wgrad_grid=256, prepped=1))
    c = _cfg(96, 300, 96, 300)                                                # 12: past the wave-centric tail
    _check(_plan(c, _next(c)), dict(pool_grid=288, tail="dad_tail_ecda", tail_grid=5, tail_prep=0, splits=30,
                                    wgrad="dad_wgrad_direct_f16", wgrad_grid=368, wgrad_clean=0, prepped=0, pending=0))
    c = _cfg(view=dict(USE_CLASS_AWARE_MMD=False))                            # 13: global MMD
    assert c.class_aware == 0
    _check(_plan(c), dict(BENCH, pool_grid=192, tail="dad_tail_ecda", tail_grid=5))
    c = _cfg(precision="fp32")                                                # 14
    _check(_plan(c, _next(c)), dict(encode="dad_encode_f32", encode_grid=320, prep_grid=0, pool_grid=0,
                                    tail="dad_tail_ecda_w", tail_grid=29, tail_prep=0, splits=42, wgrad="dad_wgrad_f32",
                                    wgrad_grid=252, reduce="dad_reduce", reduce_grid=784, prepped=0, pending=0))
    c = _cfg(64, 300, 0, 0, epoch=0)                                          # 15: warm-up
    assert c.warmup == 1
    _check(_plan(c), dict(BENCH, pool_grid=64, tail="dad_tail", tail_grid=1))
    c = _cfg(splits=5)                                                        # 16: raised to ceil(1280 / 64)
    _check(_plan(c), dict(BENCH, splits=20, max_splits=20, wgrad_grid=248))


@pytest.mark.parametrize("kw,want", [
    (dict(), 199898624), (dict(precision="bf16"), 199898624), (dict(B=16, T=40, Bn=12, Tn=50), 23654144),
    (dict(B=96, T=300, Bn=96, Tn=300), 298269696), (dict(view=dict(USE_CLASS_AWARE_MMD=False)), 199898624),
    (dict(precision="fp32"), 39466496), (dict(Bn=0, Tn=0, epoch=0), 78917632), (dict(splits=5), 199112192)])
def test_workspace_bytes_unchanged(kw, want):
    """dad_workspace_bytes of every config above, as the library reported them before the plan existed."""
    n = ctypes.c_size_t(0)
    assert dadpkg.pkg()._lib.lib().dad_workspace_bytes(_cfg(**kw), ctypes.byref(n)) == 0
    assert n.value == want


def test_error_returns():
    lib = dadpkg.pkg()._lib
    L = lib.lib()
    c, info = _cfg(), lib.DadStepPlanInfo()
    ncfg, nbt = _next(c)
    assert L.dad_step_plan(None, None, None, 0, 256, ctypes.byref(info)) == 1001
    bad = _cfg()
    bad.B = 0
    assert L.dad_step_plan(bad, None, None, 0, 256, ctypes.byref(info)) == 1002      # check_cfg's DAD_E_SHAPE
    bad = _cfg()
    bad.precision = 7
    assert L.dad_step_plan(bad, None, None, 0, 256, ctypes.byref(info)) == 1001
    assert L.dad_step_plan(c, None, None, 0, 1, ctypes.byref(info)) == 1001          # cus < 2
    assert L.dad_step_plan(c, None, None, 0, 256, None) == 1001
    assert L.dad_step_plan(c, ncfg, nbt, 4, 256, ctypes.byref(info)) == 1001         # defer outside DAD_PREP_*
    # a next step that does not qualify is no error: nothing is prepared
    ncfg.B = 0
    assert L.dad_step_plan(c, ncfg, nbt, 0, 256, ctypes.byref(info)) == 0 and info.prepped == 0
    assert L.dad_step_plan(c, ncfg, None, 0, 256, ctypes.byref(info)) == 0 and info.prepped == 0


# ---- the exact entry points (dad_step_plan_kernels): the `_s16` / `_rg` siblings the plan resolves, which
# dad_step_plan_info reports under their family names.  A wrong sibling reads rows with the wrong element size
# on a GPU; here it is a wrong string.
LAUNCHES = ("prep", "encode", "pool", "tail", "wgrad", "reduce")
EXACT = dict(prep="dad_prep", encode="dad_encode_wp_f16", pool=None, tail="dad_tail_ecda_w",
             wgrad="dad_wgrad_direct_f16", reduce="dad_reduce_w")                          # the bench step again
EXACT_RG = dict(prep="dad_prep_rg", encode="dad_encode_wp_f16_rg", pool=None, tail="dad_tail_ecda_w_rg",
                wgrad="dad_wgrad_direct_f16_rg", reduce="dad_reduce_w")
F32, F16, BF16 = 0, 1, 2
SMALL = dict(B=5, T=37, Bn=3, Tn=41)


def _batch(store=False, xc=F32, xn=F32):
    """This step's batch: made-up addresses, as _next's."""
    nbt = _next(_cfg(), store=store)[1]
    nbt.xc_dtype, nbt.xn_dtype = xc, xn
    return nbt


def _next16(cfg, xc, xn, **kw):
    ncfg, nbt = _next(cfg, store=True, **kw)
    nbt.xc_dtype, nbt.xn_dtype = xc, xn
    return ncfg, nbt


def _ragged(**kw):
    c = _cfg(**kw)
    c.ragged = 1
    return c


def _family(name):
    for suffix in ("_s16", "_rg"):
        if name.endswith(suffix):
            return name[:-len(suffix)]
    return name


def _kernels(cfg, batch=None, nxt=(None, None), defer=0, cus=256):
    lib = dadpkg.pkg()._lib
    out = (ctypes.c_char_p * lib.STEP_LAUNCHES)()
    assert lib.lib().dad_step_plan_kernels(cfg, batch, nxt[0], nxt[1], defer, cus, out) == 0
    got = {k: (v.decode() if v is not None else None) for k, v in zip(LAUNCHES, out)}
    # every name is its dad_step_plan_info string's sibling, and NULL exactly where the info's grid is 0
    info = _plan(cfg, nxt, defer, cus)
    info.update(prep="dad_prep", pool="dad_pool")
    for k, name in got.items():
        assert (name is None) == (info[k + "_grid"] == 0), (k, name, info[k + "_grid"])
        assert name is None or _family(name) == info[k], (k, name, info[k])
    return got


def test_exact_kernels_of_this_steps_own_launches():
    c = _cfg()
    assert _kernels(c) == EXACT                                               # 1
    p = _cfg()
    p.prepped = 1
    assert _kernels(p) == dict(EXACT, prep=None)                              # 2
    assert _kernels(c, _batch(store=True)) == EXACT                           # 3: an f32 store
    for shape in (dict(), SMALL):                                             # 4: a part of the set in a 16-bit store
        c = _cfg(**shape)
        for xc, xn in ((F16, F16), (BF16, F32), (F32, BF16)):
            assert _kernels(c, _batch(True, xc, xn)) == dict(EXACT, prep="dad_prep_s16"), (shape, xc, xn)
    c = _cfg(precision="fp32")                                                # 18
    assert _kernels(c) == dict(prep=None, encode="dad_encode_f32", pool=None, tail="dad_tail_ecda_w",
                               wgrad="dad_wgrad_f32", reduce="dad_reduce")
    c = _cfg(64, 300, 0, 0, epoch=0)                                          # 19: dense warm-up
    assert _kernels(c) == dict(EXACT, pool="dad_pool", tail="dad_tail")


def test_exact_kernels_that_prepare_the_next_batch():
    c = _cfg()
    assert _kernels(c, None, _next(c)) == dict(EXACT, wgrad="dad_wgrad_direct_f16_cp")                     # 5
    assert _kernels(c, None, _next(c, store=True)) == dict(EXACT, wgrad="dad_wgrad_direct_f16_cps")        # 6
    for shape in (dict(), SMALL):
        c = _cfg(**shape)
        assert _kernels(c, None, _next16(c, F16, F32)) == dict(EXACT, wgrad="dad_wgrad_direct_f16_cps_s16")   # 7
        assert _kernels(c, None, _next16(c, F32, BF16)) == dict(EXACT, wgrad="dad_wgrad_direct_f16_cps",      # 8
                                                                tail="dad_tail_ecda_w_s16")
    # the deferred part's rows are dad_step_prepare_rows': the launch that no longer reads them is the f32 kernel
    c = _cfg()
    nxt = _next16(c, F16, F16)
    assert _kernels(c, None, nxt, defer=CLEAN) == dict(EXACT, tail="dad_tail_ecda_w_s16")                  # 9
    assert _kernels(c, None, nxt, defer=NOISY) == dict(EXACT, wgrad="dad_wgrad_direct_f16_cps_s16")        # 10
    assert _kernels(c, None, nxt, defer=CLEAN | NOISY) == EXACT                                            # 11
    b = _cfg(precision="bf16")                                                                             # 12
    assert _kernels(b, None, _next16(b, BF16, BF16)) == dict(EXACT, encode="dad_encode_wp", tail="dad_tail_ecda_w_s16",
                                                            wgrad="dad_wgrad_direct_cps_s16")


def test_exact_kernels_of_ragged_steps():
    for shape in (dict(), SMALL):
        assert _kernels(_ragged(**shape), _batch(True, F16, F16)) == EXACT_RG                              # 13
    c = _ragged()
    nxt = _next16(c, F16, BF16)
    assert nxt[0].ragged == 1
    assert _kernels(c, _batch(True), nxt) == dict(EXACT_RG, wgrad="dad_wgrad_direct_f16_cps_rg")           # 14
    assert _kernels(c, _batch(True), nxt, defer=CLEAN) == EXACT_RG                                         # 15
    w = _ragged(B=64, T=300, Bn=0, Tn=0, epoch=0)                                                          # 16: warm-up
    assert w.warmup == 1
    assert _kernels(w, _batch(True)) == dict(EXACT_RG, pool="dad_pool_rg", tail="dad_tail")
    big = _ragged(B=96, T=300, Bn=96, Tn=300)                            # 17: the general tail has no ragged sibling
    assert _kernels(big, _batch(True)) == dict(EXACT_RG, pool="dad_pool_rg", tail="dad_tail_ecda")


def test_exact_kernels_error_returns():
    lib = dadpkg.pkg()._lib
    L = lib.lib()
    out = (ctypes.c_char_p * lib.STEP_LAUNCHES)()
    c = _cfg()
    assert L.dad_step_plan_kernels(c, _batch(False, F16, F32), None, None, 0, 256, out) == lib.E_ARG    # padded is f32
    assert L.dad_step_plan_kernels(_cfg(precision="fp32"), _batch(True, F16, F16), None, None, 0, 256, out) == lib.E_UNSUPPORTED
    assert L.dad_step_plan_kernels(c, None, None, None, 0, 256, None) == lib.E_ARG
    assert L.dad_step_plan_kernels(c, None, None, None, 0, 1, out) == lib.E_ARG                         # as dad_step_plan
    assert L.dad_step_plan_kernels(None, None, None, None, 0, 256, out) == lib.E_ARG


def test_tail_w_switch_selects_the_general_tail_of_a_ragged_step():
    """DAD_TAIL_W=0 in a child (below): row 14's step pools in dad_pool_rg and runs the general tail."""
    code = ("import test_step_plan_cpu as t; c = t._ragged(); "
            "g = t._kernels(c, t._batch(True), t._next16(c, t.F16, t.BF16)); print(g['pool'], g['tail'], g['wgrad'])")
    out = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, DAD_TAIL_W="0"),
                         cwd=os.path.dirname(os.path.abspath(__file__)), check=True, stdout=subprocess.PIPE, text=True)
    assert out.stdout.split() == ["dad_pool_rg", "dad_tail_ecda", "dad_wgrad_direct_f16_rg"]


def test_tail_w_switch_selects_the_general_tail():
    """DAD_TAIL_W=0 (read once per process, hence a child): the bench step pools separately and runs
    the general tail + ECDA launch."""
    code = ("import test_step_plan_cpu as t; g = t._plan(t._cfg()); "
            "print(g['pool_grid'], g['tail'], g['tail_grid'], g['prepped'])")
    out = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, DAD_TAIL_W="0"),
                         cwd=os.path.dirname(os.path.abspath(__file__)), check=True, stdout=subprocess.PIPE, text=True)
    assert out.stdout.split() == ["192", "dad_tail_ecda", "5", "0"]
