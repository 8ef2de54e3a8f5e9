"""The store-fed fp16 train step, dense against ragged (DADStep(ragged=True), dad_config.ragged), on batches
whose utterances differ in length.

One process, fp16, counter RNG, B = Bn = 64, T = 300, device-resident stores of `bench.synthetic_store`'s
rows, eight resident batches per case, every step naming its next batch (checkpoint.train_epoch's loop).
Cases (every batch keeps one utterance at T, so the padded length is T in all of them):

  full     all lengths 300
  synth    oracle/synth's ragged rule: lengths uniform in [150, 300]
  wide     lengths uniform in [30, 300]

Each case's batches index one store; the cases differ in the per-utterance sizes only.  The dense and the
ragged step have their own model and DADStep from the same seeds.  After a clock-settling run, per case:
dense, ragged, dense, ragged legs of `--warmup` untimed then `--steps` timed steps each, wall clock with a
device synchronise at each end.  The dense legs' spread is the noise floor: `full`'s difference is what the
mode costs with nothing to skip, `synth` and `wide` against the floor what it gains.  Then one pass per
(case, mode) with the library's per-kernel events (dad_timing_*).

  python tools/ragged_bench.py [--out profiles/ragged_step.json]
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
CASES = {"full": (300, 300), "synth": (150, 300), "wide": (30, 300)}   # lengths uniform in [lo, hi], one at T


def case_store(base, lo, hi, T, batch, rs):
    """`base`'s rows under other per-utterance sizes: uniform in [lo, hi], one utterance per batch at T."""
    n = len(base)
    sizes = rs.randint(lo, hi + 1, size=n).astype(np.int64)
    sizes = np.minimum(sizes, T)
    for b0 in range(0, n, batch):
        sizes[b0 + rs.randint(0, min(batch, n - b0))] = T
    st = PKG.data.FeatureStore.__new__(PKG.data.FeatureStore)
    st.feats = base.feats                            # (shared rows: FeatureStore.subset's construction)
    st._init_index(base.device, sizes, base.offsets, base.labels)
    return st


class Leg:
    def __init__(self, ragged, a, dev):
        self.model = PKG.SSRLModel().to(dev)
        bench.init_model_weights(self.model, seed=0)
        self.step = PKG.DADStep(self.model, bench.flavor_view(a), precision="fp16", rng="counter", seed=1000,
                                ragged=ragged)
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
    ap.add_argument("--settle-steps", type=int, default=400)
    ap.add_argument("--kernel-steps", type=int, default=64)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("ragged_bench needs the MI355X")
    PKG.lib()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    B, T, n = a.batch, a.frames, a.batch * a.batches
    P = bench.init_model_weights(PKG.SSRLModel().to(dev), seed=0)
    base = [bench.synthetic_store(P, n, T, dev, seed=3 + k, noisy=bool(k)) for k in range(2)]
    rs = np.random.RandomState(7)
    data, live = {}, {}
    for name, (lo, hi) in CASES.items():
        cs, ns = (case_store(s, min(lo, T), min(hi, T), T, B, rs) for s in base)
        ns = ns.subset(np.arange(n), with_labels=False)
        data[name] = [(cs.batch_index(np.arange(k * B, k * B + B), T=T),
                       ns.batch_index(np.arange(k * B, k * B + B), T=T, with_labels=False)) for k in range(a.batches)]
        nc = -(-T // 32)
        live[name] = {side: float(np.sum(-(-s.sizes // 32)) / (n * nc)) for side, s in (("clean", cs), ("noisy", ns))}
    legs = {"dense": Leg(False, a, dev), "ragged": Leg(True, a, dev)}
    sync = lambda: torch.cuda.synchronize(dev)

    for _ in range(max(1, a.settle_steps // 100)):       # clocks settle under the load they will be timed at
        for leg in legs.values():
            leg.run(data["full"], 100)
    sync()
    out_cases = {}
    for name, batches in data.items():
        wall = {"dense": [], "ragged": []}
        for leg in legs.values():
            leg.prepped = leg.steps = 0
        for _ in range(2):
            for mode, leg in legs.items():
                leg.run(batches, a.warmup)
                sync()
                t0 = time.perf_counter()
                leg.run(batches, a.steps)
                sync()
                wall[mode].append((time.perf_counter() - t0) / a.steps * 1e3)
        kernels = {}
        for mode, leg in legs.items():
            leg.run(batches, 8)
            sync()
            t = PKG._lib.KernelTimer(every=4, max_steps=a.kernel_steps)
            leg.run(batches, a.kernel_steps)
            sync()
            kernels[mode] = {k: {"mean_us": v[0] * 1e3, "steps": v[1]} for k, v in t.stop().items()}
        d, r = wall["dense"], wall["ragged"]
        out_cases[name] = {
            "lengths": "uniform in [%d, %d], one per batch at %d" % (min(CASES[name][0], T), min(CASES[name][1], T), T),
            "live_share": live[name],
            "dense_ms": d, "ragged_ms": r,
            "dense_spread_ms": abs(d[0] - d[1]), "ragged_spread_ms": abs(r[0] - r[1]),
            "ragged_minus_dense_ms": float(np.mean(r) - np.mean(d)),
            "ragged_over_dense": float(np.mean(r) / np.mean(d)),
            "kernels_us": kernels,
            "fraction_of_timed_steps_prepared_ahead": {m: leg.prepped / max(leg.steps, 1) for m, leg in legs.items()},
        }
    out = {
        "what": "store-fed fp16 step, B=Bn=%d T=%d, %d resident batches per case, next batch named; ms per step over "
                "%d timed steps per leg (dense, ragged, dense, ragged); live_share = sum ceil(len/32) / (B ceil(T/32))"
                % (B, T, a.batches, a.steps),
        "device": torch.cuda.get_device_name(dev), "abi": PKG._lib.DAD_ABI_VERSION,
        "steps_per_leg": a.steps, "warmup_steps_per_leg": a.warmup, "cases": out_cases,
    }
    for leg in legs.values():
        if int(leg.step.range_flag()) != 0:
            sys.exit("a step raised the range flag")
    txt = json.dumps(out, indent=1, sort_keys=True)
    print(txt)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()
