"""What time-resolved inference costs: dad_eval_windows against dad_eval_split on the same split.

Synthetic stores of IEMOCAP size (tools/eval_bench.make_store: lengths uniform in [100, 350], seeded), 1,100 and
5,531 utterances.  Every leg is the GPU time of one enqueue-only call between two HIP events (no copy, no host
work in between), student network, no per-window output requested:

  split            enqueue_eval_split: one embedding per utterance (the same GEMM and row traffic)
  prefix_25        PREFIX  (hop 25, span 1)
  sliding_25x2     SLIDING (hop 25, span 2)
  prefix_1         PREFIX  (hop 1): one window per frame, the worst case of the segmented epilogue
  sliding_1        SLIDING (hop 1, span 1)
  crops_25         the host alternative to prefix_25: one enqueue_eval_split per prefix length over a store whose
                   utterances are cropped to it (the stores are built before the clock starts)

Three rounds; in each round every leg runs `--reps` times, the legs alternating (all see the same clock state).
Reported per leg: the median over all repetitions, the median of each round and their spread, the ratio to
`split`, and for the fp32 legs the fraction of the exact-f32 MFMA floor (2 * 768 * 256 * frames flops at 157.3
TFLOP/s).  Results are compared before anything is timed: the last prefix of prefix_25 against the split
evaluator's predictions, and crops_25's predictions against prefix_25's windows.

  python tools/windows_bench.py [--n 1100 5531] [--reps 5] [--out profiles/eval_windows.json]
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import __graft_entry__ as entry  # noqa: E402
from tools.eval_bench import F32_MFMA_PEAK, make_model, make_store  # noqa: E402

HOP = 25


def cropped_stores(store, hop):
    """[(j, store of the utterances with more than j prefixes, cropped to (j + 1) * hop frames)]: shares the rows."""
    out = []
    for j in range(-(-int(store.sizes.max()) // hop)):
        idx = np.nonzero(store.sizes > j * hop)[0]
        sub = store.subset(idx)
        sub._init_index(store.device, np.minimum(sub.sizes, (j + 1) * hop), sub.offsets, sub.labels)
        out.append((j, idx, sub))
    return out


def bench(PKG, dev, n, precision, reps, rounds, seed):
    E = PKG.evaluate
    store = make_store(PKG, dev, n, seed)
    model = make_model(PKG, dev, seed)
    model.eval()
    plan = E.EvalPlan.of(store)
    crops = cropped_stores(store, HOP)
    crop_plans = [E.EvalPlan.of(s) for _, _, s in crops]

    def crops_leg():
        for p in crop_plans:
            E.enqueue_eval_split(model, p, precision=precision)

    legs = {
        "split": lambda: E.enqueue_eval_split(model, plan, precision=precision),
        "prefix_25": lambda: E.enqueue_eval_windows(model, plan, HOP, 1, "prefix", precision=precision),
        "sliding_25x2": lambda: E.enqueue_eval_windows(model, plan, HOP, 2, "sliding", precision=precision),
        "prefix_1": lambda: E.enqueue_eval_windows(model, plan, 1, 1, "prefix", precision=precision),
        "sliding_1": lambda: E.enqueue_eval_windows(model, plan, 1, 1, "sliding", precision=precision),
        "crops_25": crops_leg,
    }

    # results first
    whole = E.evaluate_store(model, store, precision=precision, outputs=("pred",))["pred"]
    pre = E.evaluate_windows_store(model, store, HOP, 1, "prefix", precision=precision, outputs=("w_pred", "last_pred"))
    off = torch.from_numpy(pre["win_off"].astype(np.int64)).to(dev)
    checks = {"last_prefix_differs_from_split": int((pre["last_pred"] != whole).sum())}
    differ = 0
    for (j, idx, sub), p in zip(crops, crop_plans):
        got = E.evaluate_store(model, p, precision=precision, outputs=("pred",))["pred"]
        differ += int((got != pre["w_pred"][off[torch.from_numpy(idx).to(dev)] + j]).sum())
    checks["crop_predictions_differing_from_windows"] = differ
    checks["windows"] = {k: int(plan.window_buffers(*a)["windows"]) for k, a in
                         (("prefix_25", (HOP, 1, "prefix")), ("sliding_25x2", (HOP, 2, "sliding")),
                          ("prefix_1", (1, 1, "prefix")))}
    checks["pieces"] = {k: int(plan.window_buffers(*a)["pieces"]) for k, a in
                        (("hop_25", (HOP, 1, "prefix")), ("hop_1", (1, 1, "prefix")))}

    for fn in legs.values():
        fn()
    torch.cuda.synchronize(dev)
    times = {k: [[] for _ in range(rounds)] for k in legs}
    for r in range(rounds):
        for _ in range(reps):
            for k, fn in legs.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize(dev)
                e0.record()
                fn()
                e1.record()
                torch.cuda.synchronize(dev)
                times[k][r].append(e0.elapsed_time(e1))
    res = {}
    flops = 2.0 * 768 * 256 * plan.frames
    for k, per_round in times.items():
        allv = np.concatenate(per_round)
        med = [float(np.median(v)) for v in per_round]
        s = {"median_ms": float(np.median(allv)), "min_ms": float(allv.min()), "max_ms": float(allv.max()),
             "round_medians_ms": med, "round_spread": (max(med) - min(med)) / float(np.median(med)),
             "reps": int(len(allv))}
        work = flops if k != "crops_25" else 2.0 * 768 * 256 * sum(p.frames for p in crop_plans)
        s["flops"] = work
        if precision == "fp32":
            s["mfma_floor_ms"] = work / F32_MFMA_PEAK * 1e3
            s["fraction_of_mfma_floor_at_median"] = s["mfma_floor_ms"] / s["median_ms"]
        res[k] = s
    for k in res:
        res[k]["ratio_to_split_at_median"] = res[k]["median_ms"] / res["split"]["median_ms"]
    return {"n_utterances": n, "frames": plan.frames, "slabs": plan.slabs, "precision": precision, "checks": checks,
            "crop_calls": len(crop_plans), "legs": res}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, nargs="+", default=[1100, 5531])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--seed", type=int, default=5)
    ap.add_argument("--precisions", nargs="+", default=["fp32", "fp16"])
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("windows_bench needs the MI355X")
    PKG = entry._pkg()
    PKG.lib()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    out = {"what": "GPU time of one enqueue-only call, student network: dad_eval_windows against dad_eval_split",
           "device": torch.cuda.get_device_name(dev), "hop": HOP, "rounds": a.rounds, "reps_per_round": a.reps,
           "runs": [bench(PKG, dev, n, prec, a.reps, a.rounds, a.seed) for n in a.n for prec in a.precisions]}
    txt = json.dumps(out, indent=1, sort_keys=True)
    print(txt)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()
