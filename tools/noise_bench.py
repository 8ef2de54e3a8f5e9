"""What the noise response of a split (dad_eval_noise: K noise levels of one draw in one store pass) costs on the
device, beside (a) dad_eval_split with a teacher on the same split, which runs the same number of MFMAs per row read
(the ratio prices the in-register noise generation and the K-level epilogue and head), and (b) what a user does
without it: K materialised perturbed stores x + sigma_k n and K dad_eval_split calls (the materialisation timed
separately).

On tools/eval_bench.py's synthetic stores (lengths uniform in [100, 350]) at n = 1,100 (IEMOCAP validation size)
and n = 5,531 (all of IEMOCAP), fp32 and fp16 operands, K = 3 (0, WEAK_NOISE_STD, STRONG_NOISE_STD) and K = 8.
Every figure is GPU time between two HIP events around enqueue-only calls (no copy, no host read inside).  One
process measures one size: `--rounds` rounds of the legs in turn (alternating), each leg `--warmup` untimed then
`--reps` timed calls; a leg's figure is the median of its round medians and its spread the range of the round
medians over that figure.  Each size runs under its own time limit, then the parts are merged:

  timeout -k 10 300 python tools/noise_bench.py --n 1100 --part out/noise_n1100.json && \
  timeout -k 10 420 python tools/noise_bench.py --n 5531 --part out/noise_n5531.json && \
  python tools/noise_bench.py --merge out/noise_n1100.json out/noise_n5531.json --out profiles/eval_noise.json
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np  # noqa: E402

LEVELS = {3: (0.0, 0.01, 0.05), 8: (0.0, 0.01, 0.02, 0.05, 0.1, 0.25, 0.5, 1.0)}


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


def summarise(rounds):
    med = float(np.median(rounds))
    return {"ms": med, "by_round_ms": [float(v) for v in rounds], "spread": float((max(rounds) - min(rounds)) / med)}


def measure(a):
    import torch
    import __graft_entry__ as entry
    from eval_bench import make_model, make_store
    if not torch.cuda.is_available():
        sys.exit("noise_bench needs the MI355X")
    PKG = entry._pkg()
    PKG.lib()
    E, L, D = PKG.evaluate, PKG._lib, PKG.data
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    sync = lambda: torch.cuda.synchronize(dev)
    store = make_store(PKG, dev, a.n, a.seed)
    model = make_model(PKG, dev, a.seed)
    model.eval()
    plan = E.EvalPlan.of(store)
    res = {"n": a.n, "frames": plan.frames, "slabs": plan.slabs, "device": torch.cuda.get_device_name(dev),
           "store_bytes": int(store.feats.numel() * store.feats.element_size()), "cases": {}}
    gen = torch.Generator(device=dev)
    gen.manual_seed(a.seed + 7)

    def materialise(sigmas):
        """K perturbed stores x + sigma_k n of one draw n: the user's route without dad_eval_noise."""
        n_ = torch.randn(store.feats.shape, device=dev, generator=gen)
        return [D.FeatureStore(store.feats + s * n_, store.sizes, store.offsets, store.labels, device=dev)
                for s in sigmas]

    for K, sigmas in LEVELS.items():
        stores = materialise(sigmas)
        plans = [E.EvalPlan.of(s) for s in stores]
        mat_rounds = []
        for precision in ("fp32", "fp16"):
            prec = E._PRECISIONS[precision]
            legs = {
                "noise": lambda: E.enqueue_eval_noise(model, plan, sigmas, seed=a.seed, precision=precision),
                "split_teacher": lambda: E.enqueue_eval_split(model, plan, True, True, precision),
                "k_split_calls": lambda: [E.enqueue_eval_split(model, p, False, True, precision) for p in plans],
            }
            rounds = {name: [] for name in legs}
            for _ in range(a.rounds):
                for name, fn in legs.items():
                    rounds[name].append(timed(fn, sync, a.warmup, a.reps))
                if precision == "fp32":
                    mat_rounds.append(timed(lambda: materialise(sigmas), sync, 1, 2))
            legs_out = {name: summarise(v) for name, v in rounds.items()}
            case = {"levels": list(sigmas), "legs": legs_out,
                    "noise_over_split_teacher": legs_out["noise"]["ms"] / legs_out["split_teacher"]["ms"],
                    "k_split_calls_over_noise": legs_out["k_split_calls"]["ms"] / legs_out["noise"]["ms"],
                    "workspace_bytes": int(L.lib().dad_eval_noise_workspace_bytes(plan.n, plan.slabs, K, prec)),
                    "split_workspace_bytes": int(L.lib().dad_eval_workspace_bytes(plan.n, plan.slabs, prec, 1))}
            res["cases"]["%s_K%d" % (precision, K)] = case
        mat = summarise(mat_rounds)
        mat["bytes_written"] = K * res["store_bytes"]
        for precision in ("fp32", "fp16"):
            c = res["cases"]["%s_K%d" % (precision, K)]
            c["materialise_k_stores"] = mat
            c["k_stores_and_calls_over_noise"] = (mat["ms"] + c["legs"]["k_split_calls"]["ms"]) / c["legs"]["noise"]["ms"]
        del stores, plans
        torch.cuda.empty_cache()
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
        out = {"what": "dad_eval_noise (K noise levels of one draw in one store pass) against (a) dad_eval_split with a "
                       "teacher on the same split and (b) K materialised perturbed stores and K dad_eval_split calls; "
                       "GPU ms between events of enqueue-only calls, the median of alternating rounds' medians, spread "
                       "= the range of the round medians over it",
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
