"""What evaluating K checkpoints on one split costs on the device: (a) one dad_eval_models call (the slab-pair
kernel: one W1 fragment load feeds two slabs), beside what a user does without it, (b) K student-only dad_eval_split
calls and (c) ceil(K / 2) teacher-paired dad_eval_split calls (two networks per row read, W1 streamed once per slab
and network).  dad_eval_split is the unchanged evaluator of the same library.

On tools/eval_bench.py's synthetic stores (lengths uniform in [100, 350]) at n = 1,100 (IEMOCAP validation size)
and n = 5,531 (all of IEMOCAP), fp32 and fp16 operands, K = 1, 2, 4, 8.  Every figure is GPU time between two HIP
events around enqueue-only calls (no copy, no host read inside).  One process measures one size: `--rounds` rounds of
the legs in turn (alternating), each leg `--warmup` untimed then `--reps` timed calls; a leg's figure is the median of
its round medians and its spread the range of the round medians over that figure.  w1_bytes_read is what the waves
of a leg load of W1 (a: ceil(slabs / 2) K copies; b, c: slabs K copies), w1_gbps_at_median that over the leg's time,
as profiles/eval_split.json records it.  Each size runs under its own time limit, then the parts are merged:

  timeout -k 10 300 python tools/models_bench.py --n 1100 --part out/models_n1100.json && \
  timeout -k 10 420 python tools/models_bench.py --n 5531 --part out/models_n5531.json && \
  python tools/models_bench.py --merge out/models_n1100.json out/models_n5531.json --out profiles/eval_models.json

The one condition on the slab-pair kernel: at K = 8, leg (a) is not slower than leg (c) by more than the spread of
(c)'s rounds, at both sizes and in both precisions (`condition_met`).
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np  # noqa: E402

KS = (1, 2, 4, 8)
W1_ELEMS = 256 * 768


def timed(fn, sync, warmup, reps):
    """Median GPU ms of fn's launches between two events."""
    import torch
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    times = []
    for i in range(warmup + reps):
        ev[0].record()
        fn()
        ev[1].record()
        sync()
        if i >= warmup:
            times.append(ev[0].elapsed_time(ev[1]))
    return float(np.median(times))


def summarise(rounds, w1_bytes):
    med = float(np.median(rounds))
    return {"ms": med, "by_round_ms": [float(v) for v in rounds], "spread": float((max(rounds) - min(rounds)) / med),
            "w1_bytes_read": int(w1_bytes), "w1_gbps_at_median": w1_bytes / (med * 1e-3) / 1e9}


class Pair:
    """The two attributes enqueue_eval_split reads of a model."""

    def __init__(self, student, teacher):
        self.student_flat, self.teacher_flat = student, teacher


def measure(a):
    import torch
    import __graft_entry__ as entry
    from eval_bench import make_model, make_store
    if not torch.cuda.is_available():
        sys.exit("models_bench needs the MI355X")
    PKG = entry._pkg()
    PKG.lib()
    E, L = PKG.evaluate, PKG._lib
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    sync = lambda: torch.cuda.synchronize(dev)
    store = make_store(PKG, dev, a.n, a.seed)
    plan = E.EvalPlan.of(store)
    flats = []
    for k in range(max(KS) // 2):           # 8 different networks: the students and teachers of 4 seeded models
        m = make_model(PKG, dev, a.seed + k)
        flats += [m.student_flat.detach().clone(), m.teacher_flat.detach().clone()]
    res = {"n": a.n, "frames": plan.frames, "slabs": plan.slabs, "device": torch.cuda.get_device_name(dev),
           "store_bytes": int(store.feats.numel() * store.feats.element_size()), "cases": {}}
    for precision in ("fp32", "fp16"):
        prec = E._PRECISIONS[precision]
        wb = W1_ELEMS * (4 if precision == "fp32" else 2)
        for K in KS:
            nets = flats[:K]
            singles = [Pair(f, f) for f in nets]
            pairs = [Pair(nets[i], nets[i + 1] if i + 1 < K else None) for i in range(0, K, 2)]
            legs = {
                "models": lambda: E.enqueue_eval_models(nets, plan, precision=precision),
                "k_split_calls": lambda: [E.enqueue_eval_split(p, plan, False, True, precision) for p in singles],
                "paired_split_calls": lambda: [E.enqueue_eval_split(p, plan, p.teacher_flat is not None, True,
                                                                    precision) for p in pairs],
            }
            w1 = {"models": (plan.slabs + 1) // 2 * K * wb, "k_split_calls": plan.slabs * K * wb,
                  "paired_split_calls": plan.slabs * K * wb}
            rounds = {name: [] for name in legs}
            for _ in range(a.rounds):
                for name, fn in legs.items():
                    rounds[name].append(timed(fn, sync, a.warmup, a.reps))
            out = {name: summarise(v, w1[name]) for name, v in rounds.items()}
            c = out["paired_split_calls"]
            res["cases"]["%s_K%d" % (precision, K)] = {
                "legs": out,
                "models_over_k_split_calls": out["models"]["ms"] / out["k_split_calls"]["ms"],
                "models_over_paired_split_calls": out["models"]["ms"] / c["ms"],
                "condition_met": bool(out["models"]["ms"] <= c["ms"] * (1.0 + c["spread"])),
                "workspace_bytes": int(L.lib().dad_eval_models_workspace_bytes(plan.n, plan.slabs, K, prec)),
                "split_workspace_bytes": int(L.lib().dad_eval_workspace_bytes(plan.n, plan.slabs, prec, 1))}
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--n", type=int, default=1100)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--seed", type=int, default=5)
    ap.add_argument("--part", default=None, help="write this size's measurements here")
    ap.add_argument("--merge", nargs="+", default=None, help="parts to merge into --out")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.merge:
        parts = [json.load(open(p)) for p in a.merge]
        out = {"what": "K checkpoints on one split: (models) one dad_eval_models call, the slab-pair kernel; "
                       "(k_split_calls) K student-only dad_eval_split calls; (paired_split_calls) ceil(K / 2) "
                       "teacher-paired dad_eval_split calls; GPU ms between events of enqueue-only calls, the median of "
                       "alternating rounds' medians, spread = the range of the round medians over it; no kernel trace "
                       "was taken",
               "condition": "at K = 8, models <= paired_split_calls * (1 + spread of paired_split_calls)",
               "condition_met_at_K8": {"n%d" % p["n"]: {pr: p["cases"]["%s_K8" % pr]["condition_met"]
                                                       for pr in ("fp32", "fp16")} for p in parts},
               "sizes": {"n%d" % p["n"]: p for p in parts}}
    else:
        if a.rounds < 3:
            sys.exit("at least 3 rounds")
        out = measure(a)
    txt = json.dumps(out, indent=1, sort_keys=True)
    print(txt)
    path = a.out if a.merge else a.part
    if path:
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()
