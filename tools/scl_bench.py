"""What the supervised-contrastive term costs the store-fed fp16 train step (dad_config.scl_on: dad_scl's four
launches between the tail launch and the weight gradient, csrc/scl.hip).

One process, fp16, counter RNG, B = Bn = 64, T = 300, f32 device-resident stores of `bench.synthetic_store`'s
rows, eight resident batches, every step naming its next batch (checkpoint.train_epoch's loop).  Legs, each with
its own model and DADStep from the same seeds:

  off      the flavour's defaults (TARGET_SCL_WEIGHT = 0): no launch and no allocation added
  on       TARGET_SCL_WEIGHT = --weight, SCL_START_EPOCH = 0: n = 128 rows, two row tiles of two chunks

After a clock-settling run: `--rounds` rounds of off, on, each leg `--warmup` untimed then `--steps` timed steps,
wall clock with a device synchronise at each end.  The off leg's spread over the rounds is the noise floor the
difference is read against.

  python tools/scl_bench.py [--out profiles/scl_step.json] [--legs off,on] [--parent FILE]

`--legs off` uses nothing this feature added, so it also runs with an earlier build of the library
(tools/build_old.py <rev> parent; DAD_LIB_VARIANT=parent): `--parent FILE` embeds such a run's JSON, timed in a
process of its own, under "parent_library".
"""
import argparse
import ctypes
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import bench  # noqa: E402

PKG = bench.PKG


class Leg:
    def __init__(self, weight, a, dev):
        self.model = PKG.SSRLModel().to(dev)
        bench.init_model_weights(self.model, seed=0)
        view = bench.flavor_view(a)
        if weight:
            view.overrides.update(TARGET_SCL_WEIGHT=weight, SCL_START_EPOCH=0)
        self.step = PKG.DADStep(self.model, view, precision="fp16", rng="counter", seed=1000)
        self.epoch = a.epoch
        self.k = 0
        self.prepped = self.steps = 0
        self.losses = None

    def run(self, batches, n):
        nb = len(batches)
        for _ in range(n):
            cur, nxt = batches[self.k % nb], batches[(self.k + 1) % nb]
            self.losses = self.step.step(cur[0], cur[1], self.epoch, next_batch=nxt)
            self.prepped += bool(self.step.last_prepped)
            self.steps += 1
            self.k += 1


def alone_us(n, dev, reps=200, tau=0.1):
    """dad_scl on its own (its four launches, loss and gradient) for n post-ReLU-like rows: microseconds per call
    between two events around `reps` back-to-back calls, after 20 untimed ones."""
    L = PKG.lib()
    g = torch.Generator().manual_seed(5)
    emb = (0.6 + 0.25 * torch.randn(n, 256, generator=g)).clamp_(min=0).to(dev)
    lab = torch.randint(0, 4, (n,), generator=g).to(dev)
    mem = torch.ones(n, dtype=torch.uint8, device=dev)
    out = torch.empty(PKG._lib.SCL_SLOTS, device=dev)
    grad = torch.empty(n, 256, device=dev)
    ws = torch.empty(int(L.dad_scl_workspace_bytes(n)), dtype=torch.uint8, device=dev)
    stream = torch.cuda.current_stream(dev).cuda_stream
    call = lambda: PKG._lib.check(L.dad_scl(emb.data_ptr(), lab.data_ptr(), mem.data_ptr(), n, tau, out.data_ptr(),
                                            grad.data_ptr(), ws.data_ptr(), stream), "dad_scl")
    for _ in range(20):
        call()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        call()
    e1.record()
    torch.cuda.synchronize(dev)
    return e0.elapsed_time(e1) / reps * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--frames", type=int, default=300)
    ap.add_argument("--batches", type=int, default=8)
    ap.add_argument("--epoch", type=int, default=60)
    ap.add_argument("--flavor", default="iemocap")
    ap.add_argument("--force-ecda", action="store_true")
    ap.add_argument("--weight", type=float, default=0.2)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--settle-steps", type=int, default=400)
    ap.add_argument("--legs", default="off,on")
    ap.add_argument("--parent", default=None, help="JSON of a `--legs off` run with the parent commit's library")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("scl_bench needs the MI355X")
    if a.rounds < 3 or a.steps < 200:
        sys.exit("at least 3 rounds of at least 200 timed steps")
    PKG.lib()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    B, T, n = a.batch, a.frames, a.batch * a.batches
    P = bench.init_model_weights(PKG.SSRLModel().to(dev), seed=0)
    cs, ns = (bench.synthetic_store(P, n, T, dev, seed=3 + k, noisy=bool(k)) for k in range(2))
    batches = [(cs.batch_index(np.arange(k * B, k * B + B), T=T),
                ns.batch_index(np.arange(k * B, k * B + B), T=T, with_labels=False)) for k in range(a.batches)]
    names = a.legs.split(",")
    weight = {"off": 0.0, "on": a.weight}
    legs = {m: Leg(weight[m], a, dev) for m in names}
    sync = lambda: torch.cuda.synchronize(dev)

    for _ in range(max(1, a.settle_steps // 100)):       # clocks settle under the load they will be timed at
        for leg in legs.values():
            leg.run(batches, 100 // len(legs) + 1)
    sync()
    for leg in legs.values():
        leg.prepped = leg.steps = 0
    wall = {m: [] for m in names}
    for _ in range(a.rounds):
        for m, leg in legs.items():
            leg.run(batches, a.warmup)
            sync()
            t0 = time.perf_counter()
            leg.run(batches, a.steps)
            sync()
            wall[m].append((time.perf_counter() - t0) / a.steps * 1e3)
    out = {
        "what": "store-fed fp16 step, B=Bn=%d T=%d, %d resident batches, next batch named; ms per step over %d timed "
                "steps per leg and round, legs alternating (%s) in one process" % (B, T, a.batches, a.steps, ", ".join(names)),
        "device": torch.cuda.get_device_name(dev), "abi": PKG._lib.DAD_ABI_VERSION,
        "library": os.environ.get("DAD_LIB_VARIANT") or "working tree",
        "steps_per_leg": a.steps, "warmup_steps_per_leg": a.warmup, "rounds": a.rounds,
        "ms_per_step": wall, "mean_ms": {m: float(np.mean(v)) for m, v in wall.items()},
        "fraction_of_timed_steps_prepared_ahead": {m: leg.prepped / max(leg.steps, 1) for m, leg in legs.items()},
        "off_leg": "TARGET_SCL_WEIGHT = 0: no launch and no allocation added (tests/test_gpu_scl.py for the term's "
                   "results, bench.py --dump-outputs against the parent commit's library for the step without it)",
    }
    if "off" in wall:
        off = wall["off"]
        out["off_spread_ms"] = float(max(off) - min(off))
        out["minus_off_ms"] = {m: float(np.mean(v) - np.mean(off)) for m, v in wall.items() if m != "off"}
    if "on" in legs:
        c_rt, c_ch, c_per = ctypes.c_int(0), ctypes.c_int(0), ctypes.c_int(0)
        cus = torch.cuda.get_device_properties(dev).multi_processor_count
        PKG._lib.check(PKG.lib().dad_scl_plan(2 * B, cus, ctypes.byref(c_rt), ctypes.byref(c_ch), ctypes.byref(c_per)),
                       "dad_scl_plan")
        out["on_leg"] = {"weight": a.weight, "rows": 2 * B, "row_tiles": c_rt.value, "chunks": c_ch.value,
                         "launches_added": 4,
                         "dad_scl_alone_us_per_call": {str(m): alone_us(m, dev) for m in (16, 2 * B, 512, 2048)},
                         "last_step_losses": {k: float(v) for k, v in legs["on"].losses.items()}}
    for leg in legs.values():
        if int(leg.step.range_flag()) != 0:
            sys.exit("a step raised the range flag")
    if a.parent:
        with open(a.parent) as f:
            p = json.load(f)
        out["parent_library"] = {"note": "the parent commit's library, `--legs off`, timed in a process of its own "
                                         "(not alternating with the legs above)",
                                 "ms_per_step": p["ms_per_step"]["off"], "mean_ms": p["mean_ms"]["off"],
                                 "off_spread_ms": p.get("off_spread_ms")}
    else:
        out["parent_library"] = "not measured against the parent"
    txt = json.dumps(out, indent=1, sort_keys=True)
    print(txt)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()
