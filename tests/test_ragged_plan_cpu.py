"""Ragged mode (dad_config.ragged) without a GPU: the ABI field, the refusals, and the host plan of the
live slabs (dad_step_ragged_plan, computed by the functions the `_rg` kernels call on the device lengths).

A slab (32 frames) of utterance b is live iff c < ceil(len_b / 32).  Teachers run the live weak slabs,
students the live clean slabs and then the live strong slabs; the weight gradient's splits share the
student list.  Every live slab must be run exactly once, no dead slab at all, and with every slab live
the shares must be the dense step's."""
import ctypes
import os
import random
import subprocess

import pytest

import dadpkg

ROOT = dadpkg.ROOT

GEOMS = [(64, 300, 64, 300, 256), (1024, 1280, 1024, 300, 256), (1024, 1280, 1024, 300, 8), (5, 37, 3, 41, 256)]
SETS = ("full", "ones", "one_full", "uniform", "zeros")


def _cfg(B, T, Bn, Tn, epoch=60, precision="fp16", ragged=1):
    p = dadpkg.pkg()
    prec = {"fp16": p._lib.PREC_FP16, "bf16": p._lib.PREC_BF16, "fp32": p._lib.PREC_FP32}[precision]
    cfg = p.dad_config_for(p.ConfigView(flavor="iemocap"), B, T, Bn, Tn, epoch, 1, precision=prec)
    cfg.ragged = ragged
    return cfg


def _lengths(kind, B, T, seed):
    rng = random.Random(seed)
    if kind == "full":
        return [T] * B
    if kind == "ones":
        return [1] * B
    if kind == "one_full":
        v = [1] * B
        v[rng.randrange(B)] = T
        return v
    if kind == "uniform":
        return [rng.randint(1, T) for _ in range(B)]
    v = [rng.randint(1, T) for _ in range(B)]      # "zeros": utterances without frames in the middle
    for i in range(1, B - 1, 2):
        v[i] = 0
    if B >= 5:
        v[B // 2] = v[B // 2 + 1] = 0              # (two in a row)
    return v


def _live(lens, T):
    nc = -(-T // 32)
    return [min(nc, -(-l // 32)) for l in lens]


@pytest.mark.parametrize("kind", SETS)
@pytest.mark.parametrize("B,T,Bn,Tn,cus", GEOMS)
def test_ragged_plan_runs_every_live_slab_once_and_no_dead_one(B, T, Bn, Tn, cus, kind):
    p = dadpkg.pkg()
    lib = p._lib
    L = lib.lib()
    cfg = _cfg(B, T, Bn, Tn)
    lenc, lenn = _lengths(kind, B, T, 11), _lengths(kind, Bn, Tn, 12)
    plan = lib.ragged_plan(cfg, lenc, lenn, cus)
    lc, ln = _live(lenc, T), _live(lenn, Tn)
    clean = [("c", b, c) for b in range(B) for c in range(lc[b])]
    noisy = [(b, c) for b in range(Bn) for c in range(ln[b])]
    weak = [("w", b, c) for b, c in noisy]
    student = clean + [("s", b, c) for b, c in noisy]
    assert (plan["live_clean"], plan["live_noisy"]) == (len(clean), len(noisy))
    # the grid is the dense step's: it does not depend on the lengths
    nt, ns, mj = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    assert L.dad_encoder_ws_plan(cfg, cus, ctypes.byref(nt), ctypes.byref(ns), ctypes.byref(mj)) == 0
    assert len(plan["enc"]) == nt.value + ns.value
    # encoder: contiguous shares in workgroup order, so "exactly once" = the shares tile the lists
    seen = {0: [], 1: []}
    for wg, (t, first, count) in enumerate(plan["enc"]):
        assert t == (1 if wg < nt.value else 0)
        assert 0 <= count <= 256
        seen[t] += list(range(first, first + count))
    assert seen[1] == list(range(len(weak)))          # every live weak slab once: no index past the live list
    assert seen[0] == list(range(len(student)))
    assert plan["max_enc_range"] == max(c for _, _, c in plan["enc"]) <= 256
    # weight gradient: the splits tile the student list; utterances per split within the LDS table
    info = lib.DadStepPlanInfo()
    assert L.dad_step_plan(cfg, None, None, 0, cus, ctypes.byref(info)) == 0
    assert len(plan["split"]) == info.splits
    got, most = [], 0
    for s0, s1 in plan["split"]:
        assert 0 <= s0 <= s1 <= len(student) and s1 - s0 <= 64
        got += list(range(s0, s1))
        most = max(most, len({student[k][:2] for k in range(s0, s1)}))
    assert got == list(range(len(student)))
    assert plan["max_split_utts"] == most <= 64
    if kind == "full":
        # the live lists are the dense lists: dad_encoder_ws_jobs' ranges and wg_range's shares
        need = 4 * (nt.value + ns.value)
        buf = (ctypes.c_int * need)()
        assert L.dad_encoder_ws_jobs(cfg, cus, buf, need) == nt.value + ns.value
        assert plan["enc"] == [(buf[4 * w], buf[4 * w + 1], buf[4 * w + 3]) for w in range(nt.value + ns.value)]
        total = len(student)
        per = -(-total // info.splits)
        assert plan["split"] == [(min(s * per, total), min(total, s * per + per)) for s in range(info.splits)]


def test_ragged_plan_warmup_has_no_noisy_list():
    lib = dadpkg.pkg()._lib
    cfg = _cfg(5, 37, 3, 41, epoch=0)
    plan = lib.ragged_plan(cfg, [37, 0, 1, 33, 32], None, 256)
    assert (plan["live_clean"], plan["live_noisy"]) == (2 + 0 + 1 + 2 + 1, 0)
    assert all(t == 0 for t, _, _ in plan["enc"])
    assert sum(c for _, _, c in plan["enc"]) == 6


def test_sorted_short_utterances_fall_back_to_an_even_split_by_jobs():
    """Many utterances of at most 16 frames sorted together hold one job per sub-slab: a share that is
    even by sub-slabs would exceed the encoder's 256-job table, so that role's jobs are split by count."""
    lib = dadpkg.pkg()._lib
    cfg = _cfg(1024, 1280, 1024, 300)
    lenc = [16] * 600 + [1280] * 424
    plan = lib.ragged_plan(cfg, lenc, [300] * 1024, 256)
    assert plan["max_enc_range"] <= 256
    first = 0
    for t, a0, n in plan["enc"]:
        if not t:
            assert a0 == first
            first += n
    assert first == plan["live_clean"] + plan["live_noisy"]


def test_config_layout_and_abi_version(tmp_path):
    """dad_config.ragged takes reserved[0]'s place (offset 204); the size (224) and every other offset stay,
    and the ABI version stays 10: a zero reserved[0] always meant dense."""
    p = dadpkg.pkg()
    C = p._lib.DadConfig
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "dad.h"', "int main(void){",
             'printf("size %zu\\n", sizeof(dad_config));']
    for f in C._fields_:
        lines.append('printf("%s %%zu\\n", offsetof(dad_config, %s));' % (f[0], f[0]))
    lines.append("return 0;}")
    c = tmp_path / "probe.c"
    c.write_text("\n".join(lines))
    exe = tmp_path / "probe"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(c), "-o", str(exe)])
    out = dict(l.split() for l in subprocess.check_output([str(exe)]).decode().splitlines())
    assert int(out["size"]) == ctypes.sizeof(C) == 224
    assert int(out["prepped"]) == 200
    assert int(out["ragged"]) == C.ragged.offset == 204
    assert int(out["reserved"]) == C.reserved.offset == 208 and C.reserved.size == 12
    for f in C._fields_:
        assert int(out[f[0]]) == getattr(C, f[0]).offset, f[0]
    assert p._lib.lib().dad_abi_version() == 10


def test_refusals():
    p = dadpkg.pkg()
    lib = p._lib
    L = lib.lib()
    info = lib.DadStepPlanInfo()
    assert L.dad_step_plan(_cfg(64, 300, 64, 300, precision="fp32"), None, None, 0, 256, ctypes.byref(info)) == 1004
    assert L.dad_step_plan(_cfg(64, 300, 64, 300, precision="fp32", ragged=0), None, None, 0, 256, ctypes.byref(info)) == 0
    n = ctypes.c_size_t(0)
    assert L.dad_workspace_bytes(_cfg(64, 300, 64, 300, precision="fp32"), ctypes.byref(n)) == 1004
    out = lib.DadRaggedPlan()
    lens = (ctypes.c_int32 * 64)(*([300] * 64))
    assert L.dad_step_ragged_plan(_cfg(64, 300, 64, 300, precision="fp32", ragged=0), lens, lens, 256, out) == 1004
    assert L.dad_step_ragged_plan(_cfg(64, 300, 64, 300), lens, None, 256, out) == 1001      # no noisy lengths
    assert L.dad_step_ragged_plan(_cfg(64, 300, 64, 300), lens, lens, 256, out) == 1001      # no room for the shares
    assert out.enc_grid == 256 and out.splits == 21                                          # ... but their sizes


def test_a_ragged_set_is_prepared_by_a_ragged_step_only():
    """can_prepare_ahead: next_cfg->ragged == cfg->ragged, and a ragged next batch is a store batch."""
    lib = dadpkg.pkg()._lib
    L = lib.lib()

    def prepped(ragged, next_ragged, store=True):
        cfg = _cfg(64, 300, 64, 300, ragged=ragged)
        ncfg = lib.DadConfig.from_buffer_copy(cfg)
        ncfg.counter = cfg.counter + 1
        ncfg.ragged = next_ragged
        nbt = lib.DadBatch()
        for i, name in enumerate(("xc", "mc", "yc", "xn", "mn") + (("rowc", "lenc", "rown", "lenn") if store else ())):
            setattr(nbt, name, 0x1000 * (i + 1))
        info = lib.DadStepPlanInfo()
        assert L.dad_step_plan(cfg, ncfg, nbt, 0, 256, ctypes.byref(info)) == 0
        return info.prepped, info.wgrad.decode()

    assert prepped(1, 1) == (1, "dad_wgrad_direct_f16_cps")
    assert prepped(0, 0) == (1, "dad_wgrad_direct_f16_cps")
    assert prepped(1, 0)[0] == 0 and prepped(0, 1)[0] == 0
    assert prepped(1, 1, store=False)[0] == 0


def test_stale_library_is_reported_when_ragged_is_asked_for(monkeypatch):
    """A library of ABI 10 built before the mode loads (the entry point is optional at load), and asking
    for the mode names the remedy."""
    p = dadpkg.pkg()
    lib = p._lib

    class Stale:
        def __getattr__(self, name):
            if name == "dad_step_ragged_plan":
                raise AttributeError(name)
            return getattr(lib._LIB_REAL, name)

    lib.lib()
    monkeypatch.setattr(lib, "_LIB_REAL", lib._LIB, raising=False)
    monkeypatch.setattr(lib, "_LIB", Stale())
    with pytest.raises(lib.DadError, match="rebuild"):
        lib.require("dad_step_ragged_plan", "ragged=True")
