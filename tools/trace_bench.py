"""What the confirmation-bias log costs the store-fed fp16 train step (DADStep(trace=TrainingTrace),
dad_trace_append: one small launch per step behind the tail launch).

One process, fp16, counter RNG, B = Bn = 64, T = 300, f32 device-resident stores of `bench.synthetic_store`'s
rows, eight resident batches, every step naming its next batch (checkpoint.train_epoch's loop).  The noisy
store is indexed as 5,531 samples (IEMOCAP's count) over those rows, and each batch's 'id' comes from a seeded
permutation of them.  Legs, each with its own model and DADStep from the same seeds:

  off      no trace attached: by construction the parent commit's step (no launch, no allocation added)
  k50      the reference's 50 tracked samples (np.random.choice, seeded)
  all      tracked="all": every row of every step is appended

After a clock-settling run: `--rounds` rounds of off, k50, all, each leg `--warmup` untimed then `--steps` timed
steps, wall clock with a device synchronise at each end.  The off leg's spread over the rounds is the noise
floor the differences are read against.

  python tools/trace_bench.py [--out profiles/trace_step.json] [--legs off,k50,all] [--parent FILE]

`--legs off` uses nothing this feature added, so it also runs with an earlier build of the library
(tools/build_old.py <rev> parent; DAD_LIB_VARIANT=parent): `--parent FILE` embeds such a run's JSON, timed in a
process of its own, under "parent_library".
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import bench  # noqa: E402

PKG = bench.PKG
N_SAMPLES = 5531


def indexed_as(base, n_samples, T, labels=True):
    """`base`'s rows as a store of n_samples full-length samples: sample s is base utterance s mod len(base)."""
    st = PKG.data.FeatureStore.__new__(PKG.data.FeatureStore)
    st.feats = base.feats                            # (shared rows: FeatureStore.subset's construction)
    s = np.arange(n_samples, dtype=np.int64) % len(base)
    st._init_index(base.device, np.full(n_samples, T, np.int64), base.offsets[s], base.labels[s] if labels else None)
    return st


class Leg:
    def __init__(self, tracked, a, dev, capacity):
        self.model = PKG.SSRLModel().to(dev)
        bench.init_model_weights(self.model, seed=0)
        self.step = PKG.DADStep(self.model, bench.flavor_view(a), precision="fp16", rng="counter", seed=1000)
        self.trace = None
        if tracked is not None:
            np.random.seed(0)
            self.trace = self.step.trace = PKG.TrainingTrace(N_SAMPLES, tracked=tracked, capacity=capacity, device=dev)
        self.epoch = a.epoch
        self.k = 0
        self.prepped = self.steps = 0

    def run(self, batches, n):
        nb = len(batches)
        for _ in range(n):
            cur, nxt = batches[self.k % nb], batches[(self.k + 1) % nb]
            self.step.step(cur[0], cur[1], self.epoch, next_batch=nxt)
            self.prepped += bool(self.step.last_prepped)
            self.steps += 1
            self.k += 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--frames", type=int, default=300)
    ap.add_argument("--batches", type=int, default=8)
    ap.add_argument("--epoch", type=int, default=60)
    ap.add_argument("--flavor", default="iemocap")
    ap.add_argument("--force-ecda", action="store_true")
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--settle-steps", type=int, default=400)
    ap.add_argument("--legs", default="off,k50,all")
    ap.add_argument("--parent", default=None, help="JSON of a `--legs off` run with the parent commit's library")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("trace_bench needs the MI355X")
    if a.rounds < 3 or a.steps < 200:
        sys.exit("at least 3 rounds of at least 200 timed steps")
    PKG.lib()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    B, T, n = a.batch, a.frames, a.batch * a.batches
    P = bench.init_model_weights(PKG.SSRLModel().to(dev), seed=0)
    base = [bench.synthetic_store(P, n, T, dev, seed=3 + k, noisy=bool(k)) for k in range(2)]
    cs, ns = base[0], indexed_as(base[1], N_SAMPLES, T, labels=False)
    ids = np.random.RandomState(11).permutation(N_SAMPLES)[:n]
    batches = [(cs.batch_index(np.arange(k * B, k * B + B), T=T),
                ns.batch_index(ids[k * B:k * B + B], T=T, with_labels=False)) for k in range(a.batches)]
    assert all(nb["id"].shape[0] == B for _, nb in batches)
    names = a.legs.split(",")
    tracked = {"off": None, "k50": 50, "all": "all"}
    total = a.settle_steps + a.rounds * (a.warmup + a.steps) + 16
    legs = {m: Leg(tracked[m], a, dev, capacity=total * B) for m in names}
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
        "what": "store-fed fp16 step, B=Bn=%d T=%d, %d resident batches, next batch named, noisy ids from %d samples; "
                "ms per step over %d timed steps per leg and round, legs alternating (%s) in one process"
                % (B, T, a.batches, N_SAMPLES, a.steps, ", ".join(names)),
        "device": torch.cuda.get_device_name(dev), "abi": PKG._lib.DAD_ABI_VERSION,
        "library": os.environ.get("DAD_LIB_VARIANT") or "working tree",
        "steps_per_leg": a.steps, "warmup_steps_per_leg": a.warmup, "rounds": a.rounds,
        "ms_per_step": wall, "mean_ms": {m: float(np.mean(v)) for m, v in wall.items()},
        "fraction_of_timed_steps_prepared_ahead": {m: leg.prepped / max(leg.steps, 1) for m, leg in legs.items()},
        "off_leg": "no trace attached: no launch and no allocation added, the parent commit's step by construction "
                   "(tests/test_gpu_trace.py::test_a_trace_changes_nothing_in_the_step for its results)",
    }
    if "off" in wall:
        off = wall["off"]
        out["off_spread_ms"] = float(max(off) - min(off))
        out["minus_off_ms"] = {m: float(np.mean(v) - np.mean(off)) for m, v in wall.items() if m != "off"}
    traces = {}
    for m, leg in legs.items():
        if int(leg.step.range_flag()) != 0:
            sys.exit("a step raised the range flag")
        if leg.trace is not None:
            log = leg.trace.bias_log()
            traces[m] = {"tracked": len(leg.trace.tracked_sample_indices), "records_offered": leg.trace.offered,
                         "records_per_step": leg.trace.offered / max(leg.k, 1), "dropped": leg.trace.dropped,
                         "records_kept": len(log)}
    out["traces"] = traces
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
