"""The store-fed fp16 train step from f32 stores, from fp16 stores read in place, and from fp16 stores
through the widening fallback.

Two `bench.synthetic_store` stores (clean, noisy) of n utterances x T frames, the headline batches'
distribution; B = 64, T = 300 by default.  Fused DeviceLoaders, batches drawn one ahead and every step
naming its next batch, as checkpoint.train_epoch does.  Three legs, interleaved in one process so all
see the same clock state:

  f32            the f32 stores, read in place (the path before ABI 10 and since)
  fp16_in_place  the same rows as fp16 stores, read in place by the row preparation (ABI 10)
  fp16_fallback  the fp16 stores through StoreFeats.materialize(): two dad_collate launches per step,
                 a padded f32 copy per batch, no preparation ahead (what a 16-bit store cost before)

Each leg has its own model and DADStep from the same seeds.  After a clock-settling run (bench.py's
--settle-ms) every repetition is `--warmup` untimed then `--steps` timed steps per leg, wall clock with
a device synchronise at each end; median / min / max over `--reps` repetitions.  Then one pass per leg
with the library's per-kernel events (dad_timing_*).  The fallback adds launches and copies, so the
in-place leg's maximum must lie below the fallback leg's minimum: the tool exits non-zero otherwise.

  python tools/store16_bench.py [--legs f32,fp16_in_place,fp16_fallback] [--out profiles/store16.json]

`--legs f32` runs on any earlier commit too (it uses nothing ABI 10 added): the f32 leg of a parent
checkout against this one, alternating on one box, shows whether the f32 path was disturbed.
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
LEGS = ("f32", "fp16_in_place", "fp16_fallback")


def stats(xs):
    xs = np.asarray(xs) * 1e3
    return {"median_ms": float(np.median(xs)), "min_ms": float(xs.min()), "max_ms": float(xs.max()), "reps": len(xs),
            "all_ms": [float(x) for x in xs]}


class Leg:
    def __init__(self, name, clean, noisy, a, dev):
        self.name = name
        self.model = PKG.SSRLModel().to(dev)
        bench.init_model_weights(self.model, seed=0)
        self.step = PKG.DADStep(self.model, bench.flavor_view(a), precision="fp16", rng="counter", seed=1000)
        g1, g2 = torch.Generator().manual_seed(1), torch.Generator().manual_seed(2)
        cl = PKG.data.DeviceLoader(clean, batch_size=a.batch, shuffle=True, generator=g1, fused=True)
        nl = PKG.data.DeviceLoader(noisy.subset(np.arange(len(noisy)), with_labels=False), batch_size=a.batch,
                                   shuffle=True, generator=g2, fused=True)
        self.ci, self.ni = self._epochs(cl), self._epochs(nl)
        self.nxt = (next(self.ci), next(self.ni))
        self.epoch = a.epoch
        self.prepped = self.steps = 0

    @staticmethod
    def _epochs(loader):        # a new epoch (a new shuffle) whenever one runs out
        while True:
            yield from loader

    def run(self, n):
        S = PKG.step
        rule = S._store_in_place if hasattr(S, "_store_in_place") else None
        if self.name == "fp16_fallback":      # the rule before ABI 10: only f32 stores are read in place
            S._store_in_place = lambda dtype, precision: dtype == torch.float32
        try:
            for _ in range(n):
                cur, self.nxt = self.nxt, (next(self.ci), next(self.ni))
                self.step.step(cur[0], cur[1], self.epoch, next_batch=self.nxt)
                self.prepped += bool(self.step.last_prepped)
                self.steps += 1
        finally:
            if rule is not None:
                S._store_in_place = rule


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--legs", default=",".join(LEGS))
    ap.add_argument("--n-utt", type=int, default=1024)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--frames", type=int, default=300)
    ap.add_argument("--epoch", type=int, default=60)
    ap.add_argument("--flavor", default="iemocap")
    ap.add_argument("--force-ecda", action="store_true")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--settle-steps", type=int, default=400)
    ap.add_argument("--kernel-steps", type=int, default=64)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    legs = [x for x in a.legs.split(",") if x]
    if not legs or any(x not in LEGS for x in legs) or a.reps < 1:
        ap.error("--legs takes %s; --reps at least 1" % ",".join(LEGS))
    if not torch.cuda.is_available():
        sys.exit("store16_bench needs the MI355X")
    PKG.lib()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    P = bench.init_model_weights(PKG.SSRLModel().to(dev), seed=0)
    f32 = [bench.synthetic_store(P, a.n_utt, a.frames, dev, seed=3 + k, noisy=bool(k)) for k in range(2)]
    stores = {"f32": f32}
    if any(x != "f32" for x in legs):
        stores["fp16"] = [PKG.data.FeatureStore(s.feats, s.sizes, s.offsets, s.labels, device=dev, dtype=torch.float16)
                          for s in f32]
    L = {x: Leg(x, *stores["f32" if x == "f32" else "fp16"], a, dev) for x in legs}
    sync = lambda: torch.cuda.synchronize(dev)

    for _ in range(max(1, a.settle_steps // 100)):       # clocks settle under the load they will be timed at
        for leg in L.values():
            leg.run(100)
    sync()
    for leg in L.values():
        leg.prepped = leg.steps = 0
    wall = {x: [] for x in legs}
    for _ in range(a.reps):
        for x, leg in L.items():
            leg.run(a.warmup)
            sync()
            t0 = time.perf_counter()
            leg.run(a.steps)
            sync()
            wall[x].append((time.perf_counter() - t0) / a.steps)

    kernels = {}
    for x, leg in L.items():
        leg.run(8)
        sync()
        t = PKG._lib.KernelTimer(every=4, max_steps=a.kernel_steps)
        leg.run(a.kernel_steps)
        sync()
        kernels[x] = {k: {"mean_us": v[0] * 1e3, "steps": v[1]} for k, v in t.stop().items()}

    rows = a.batch * a.frames
    out = {
        "what": "store-fed fp16 step, B=%d T=%d, fused loaders, next batch named (train_epoch's loop); ms per step"
                % (a.batch, a.frames),
        "device": torch.cuda.get_device_name(dev), "abi": PKG._lib.DAD_ABI_VERSION,
        "stores": "%d utterances x %d frames per store; %.2f GB (f32), %.2f GB (fp16)"
                  % (a.n_utt, a.frames, a.n_utt * a.frames * 3072 / 1e9, a.n_utt * a.frames * 1536 / 1e9),
        "steps_per_rep": a.steps, "warmup_steps_per_rep": a.warmup,
        "wall": {x: stats(v) for x, v in wall.items()},
        "kernels_us": kernels,
        "fraction_of_timed_steps_prepared_ahead": {x: leg.prepped / max(leg.steps, 1) for x, leg in L.items()},
        # what the row preparation of one step moves (dad_prep.h): source rows read once + prepared rows written
        "prep_bytes_per_step": {"f32": 2 * rows * 3072 + 3 * rows * 1536, "fp16": 2 * rows * 1536 + 3 * rows * 1536},
    }
    ok = True
    if "fp16_in_place" in wall and "fp16_fallback" in wall:
        w = out["wall"]
        ok = w["fp16_in_place"]["max_ms"] < w["fp16_fallback"]["min_ms"]
        out["in_place_max_below_fallback_min"] = ok
    if "fp16_in_place" in wall and "f32" in wall:
        out["in_place_over_f32_at_median"] = out["wall"]["fp16_in_place"]["median_ms"] / out["wall"]["f32"]["median_ms"]
    txt = json.dumps(out, indent=1, sort_keys=True)
    print(txt)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(txt + "\n")
    if not ok:
        sys.exit("the in-place leg is not faster than the fallback: a bug")


if __name__ == "__main__":
    main()
