"""The supervised-contrastive term's host side, without a GPU: the weight schedule, the three dad_config fields that
took the reserved words' place, the argument checks that come before any launch, and the host-only queries."""
import ctypes
import os
import subprocess

import pytest

import dadpkg

P = dadpkg.pkg()
LIB = P._lib


def _cfg(epoch=60, flavor="casia", **kw):
    return P.dad_config_for(P.ConfigView(flavor=flavor, **kw), 8, 40, 8, 40, epoch, 1)


@pytest.mark.parametrize("flavor", ["iemocap", "casia", "emodb"])
def test_defaults_are_the_references(flavor):
    v = P.ConfigView(flavor=flavor)
    assert (v.TARGET_SCL_WEIGHT, v.SCL_START_EPOCH, v.SCL_TEMPERATURE) == (0.0, 5001, 0.1)
    assert all(v.scl_weight(e) == 0.0 for e in (0, 29, 30, 60, 5000, 5001, 10000))
    for k in ("TARGET_SCL_WEIGHT", "SCL_START_EPOCH", "SCL_TEMPERATURE"):
        assert k in P.config.CONFIG_KEYS


def test_scl_weight_over_the_epochs():
    v = P.ConfigView(flavor="casia", TARGET_SCL_WEIGHT=0.2, SCL_START_EPOCH=45)
    assert v.WARMUP_EPOCHS == 30
    assert [v.scl_weight(e) for e in (0, 29, 30, 44, 45, 46, 400)] == [0.0, 0.0, 0.0, 0.0, 0.2, 0.2, 0.2]   # no ramp
    early = P.ConfigView(flavor="casia", TARGET_SCL_WEIGHT=0.2, SCL_START_EPOCH=0)
    assert [early.scl_weight(e) for e in (0, 29, 30)] == [0.0, 0.0, 0.2]           # the warm-up is CE only
    # a config source that sets the reference's names is honoured (a dict as well as a module)
    assert P.ConfigView({"TARGET_SCL_WEIGHT": 0.3, "SCL_START_EPOCH": 31}, flavor="emodb").scl_weight(31) == 0.3


def test_dad_config_for_fills_the_three_fields():
    off = _cfg()
    assert (off.scl_on, off.w_scl, off.scl_tau) == (0, 0.0, 0.0)
    assert list(off.reserved) == [0, 0, 0]                   # exactly the reserved words of before
    on = _cfg(TARGET_SCL_WEIGHT=0.25, SCL_START_EPOCH=31, SCL_TEMPERATURE=0.07)
    assert on.scl_on == 1 and on.w_scl == 0.25 and on.scl_tau == ctypes.c_float(0.07).value
    assert list(_cfg(epoch=30, TARGET_SCL_WEIGHT=0.25, SCL_START_EPOCH=31).reserved) == [0, 0, 0]
    assert list(_cfg(epoch=10, TARGET_SCL_WEIGHT=0.25, SCL_START_EPOCH=0).reserved) == [0, 0, 0]     # warm-up
    # everything else is the config of the step without the term, byte for byte
    a, b = bytearray(bytes(on)), bytearray(bytes(off))
    lo = LIB.DadConfig.reserved.offset
    assert a[:lo] == b[:lo] and a[lo + 12:] == b[lo + 12:] and a[lo:lo + 12] != b[lo:lo + 12]
    # the cache hands out the same bytes as dad_config_for
    view = P.ConfigView(flavor="casia", TARGET_SCL_WEIGHT=0.25, SCL_START_EPOCH=31)
    cached = P.config.ConfigCache().config(view, 8, 40, 8, 40, 60, 1)
    assert bytes(cached) == bytes(P.dad_config_for(view, 8, 40, 8, 40, 60, 1))
    changed = P.ConfigView(flavor="casia", TARGET_SCL_WEIGHT=0.5, SCL_START_EPOCH=31)
    cache = P.config.ConfigCache()
    assert cache.config(view, 8, 40, 8, 40, 60, 1).w_scl == 0.25 and cache.config(changed, 8, 40, 8, 40, 60, 1).w_scl == 0.5


def test_fields_overlay_the_reserved_words_in_c(tmp_path):
    """scl_on / w_scl / scl_tau sit at reserved[0..2] in include/dad.h, and the struct keeps its size."""
    src = ['#include <stdio.h>', '#include <stddef.h>', '#include "dad.h"', "int main(void){",
           'printf("%zu %zu %zu %zu %zu\\n", sizeof(dad_config), offsetof(dad_config, reserved),',
           '       offsetof(dad_config, scl_on), offsetof(dad_config, w_scl), offsetof(dad_config, scl_tau));',
           "dad_config c = {0}; c.scl_on = 1; c.w_scl = 0.5f; c.scl_tau = 0.1f;",
           'printf("%d %d %d\\n", c.reserved[0], c.reserved[1], c.reserved[2]);', "return 0;}"]
    c = tmp_path / "probe.c"
    c.write_text("\n".join(src))
    exe = tmp_path / "probe"
    subprocess.check_call(["gcc", "-I", os.path.join(dadpkg.ROOT, "include"), str(c), "-o", str(exe)])
    sizes, words = subprocess.check_output([str(exe)]).decode().splitlines()
    lo = LIB.DadConfig.reserved.offset
    assert [int(x) for x in sizes.split()] == [ctypes.sizeof(LIB.DadConfig), lo, lo, lo + 4, lo + 8]
    py = LIB.DadConfig()
    py.scl_on, py.w_scl, py.scl_tau = 1, 0.5, 0.1
    assert [int(x) for x in words.split()] == list(py.reserved)


@pytest.mark.parametrize("tau", [0.0, -0.1, float("nan"), float("inf")])
def test_bad_temperature_is_an_argument_error(tau):
    L = P.lib()
    # dad_scl checks it before any device call: the pointers are never followed
    dummy = ctypes.c_void_p(256)
    assert L.dad_scl(dummy, dummy, dummy, 8, tau, dummy, None, dummy, None) == LIB.E_ARG
    assert L.dad_scl_chunked(dummy, dummy, dummy, 8, tau, dummy, None, 2, dummy, None) == LIB.E_ARG
    # and so does every entry point of the step, through the config check
    cfg = _cfg(TARGET_SCL_WEIGHT=1.0, SCL_START_EPOCH=0)
    n = ctypes.c_size_t(0)
    assert L.dad_workspace_bytes(cfg, ctypes.byref(n)) == 0
    cfg.scl_tau = tau
    assert L.dad_workspace_bytes(cfg, ctypes.byref(n)) == LIB.E_ARG
    info = LIB.DadStepPlanInfo()
    assert L.dad_step_plan(cfg, None, None, 0, 256, info) == LIB.E_ARG
    cfg.scl_on = 0                       # off: the other two words are not looked at
    assert L.dad_workspace_bytes(cfg, ctypes.byref(n)) == 0


def test_dad_scl_refuses_null_pointers_and_bad_sizes():
    L = P.lib()
    d = ctypes.c_void_p(256)
    assert L.dad_scl(None, d, d, 8, 0.1, d, None, d, None) == LIB.E_ARG
    assert L.dad_scl(d, None, d, 8, 0.1, d, None, d, None) == LIB.E_ARG
    assert L.dad_scl(d, d, None, 8, 0.1, d, None, d, None) == LIB.E_ARG
    assert L.dad_scl(d, d, d, 8, 0.1, None, None, d, None) == LIB.E_ARG
    assert L.dad_scl(d, d, d, 8, 0.1, d, None, None, None) == LIB.E_ARG
    assert L.dad_scl(d, d, d, 0, 0.1, d, None, d, None) == LIB.E_SHAPE
    assert L.dad_scl(d, d, d, LIB.SCL_MAX_N + 1, 0.1, d, None, d, None) == LIB.E_SHAPE


def test_workspace_bytes_and_plan():
    L = P.lib()
    assert LIB.SCL_MAX_N >= 2 * 1024                       # the step's largest batch: 2 * DAD_MAX_BATCH
    assert L.dad_scl_workspace_bytes(0) == 0 and L.dad_scl_workspace_bytes(-3) == 0
    assert L.dad_scl_workspace_bytes(LIB.SCL_MAX_N + 1) == 0
    sizes = [L.dad_scl_workspace_bytes(n) for n in (1, 64, 65, 128, 129, LIB.SCL_MAX_N)]
    assert sizes[0] == sizes[1] > 0 and sizes[2] == sizes[3] and sizes == sorted(sizes)
    rt, ch, per = ctypes.c_int(0), ctypes.c_int(0), ctypes.c_int(0)
    args = (ctypes.byref(rt), ctypes.byref(ch), ctypes.byref(per))
    assert L.dad_scl_plan(0, 256, *args) == LIB.E_SHAPE
    assert L.dad_scl_plan(LIB.SCL_MAX_N + 1, 256, *args) == LIB.E_SHAPE
    assert L.dad_scl_plan(64, 0, *args) == LIB.E_SHAPE
    assert L.dad_scl_plan(64, 256, None, ctypes.byref(ch), ctypes.byref(per)) == LIB.E_ARG
    for n, cus in ((1, 256), (64, 256), (65, 256), (128, 256), (130, 256), (2048, 256), (2048, 8), (700, 1)):
        assert L.dad_scl_plan(n, cus, *args) == 0
        tiles = (n + LIB.SCL_TILE - 1) // LIB.SCL_TILE
        assert rt.value == tiles and 1 <= ch.value <= min(tiles, LIB.SCL_MAX_CHUNKS)
        assert (ch.value - 1) * per.value < tiles <= ch.value * per.value      # no chunk is empty
        assert rt.value * ch.value <= max(cus, rt.value)                       # one workgroup per compute unit
    assert L.dad_scl_plan(128, 256, *args) == 0 and (rt.value, ch.value, per.value) == (2, 2, 1)


def test_workspace_grows_by_the_terms_only_when_it_is_on():
    L = P.lib()
    n_off, n_on = ctypes.c_size_t(0), ctypes.c_size_t(0)
    assert L.dad_workspace_bytes(_cfg(), ctypes.byref(n_off)) == 0
    assert L.dad_workspace_bytes(_cfg(TARGET_SCL_WEIGHT=1.0, SCL_START_EPOCH=0), ctypes.byref(n_on)) == 0
    assert n_on.value - n_off.value == L.dad_scl_workspace_bytes(16)


def test_default_step_plan_lists_the_same_six_launches():
    L = P.lib()
    names = (ctypes.c_char_p * LIB.STEP_LAUNCHES)()
    for flavor in ("iemocap", "casia", "emodb"):
        for prec in (LIB.PREC_FP32, LIB.PREC_FP16):
            off = P.dad_config_for(P.ConfigView(flavor=flavor), 64, 300, 64, 300, 60, 1, precision=prec)
            assert L.dad_step_plan_kernels(off, None, None, None, 0, 256, names) == 0
            base = list(names)
            on = P.dad_config_for(P.ConfigView(flavor=flavor, TARGET_SCL_WEIGHT=1.0, SCL_START_EPOCH=0), 64, 300, 64,
                                  300, 60, 1, precision=prec)
            assert L.dad_step_plan_kernels(on, None, None, None, 0, 256, names) == 0
            assert list(names) == base and len(base) == 6 and base[3] is not None
            assert not any(b"scl" in (x or b"") for x in base)
