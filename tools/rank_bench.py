"""What ranking a split by certainty costs (dad_rank_eval_columns + dad_rank_metrics, csrc/rank.hip): alone beside
dad_cluster_metrics, as the opt-in part of a validation pass, against the host route without the operator, and at the
size limit.

On tools/eval_bench.py's synthetic stores (n utterances, lengths uniform in [100, 350]) at n = 1,100 and n = 5,531,
m = 10 columns.  GPU time between two HIP events around enqueue-only calls; `--rounds` rounds of the legs in turn,
each leg `--warmup` untimed then `--reps` timed calls; a leg's figure is the median of its round medians, its spread
the range of them.  Legs:

  rank           dad_rank_eval_columns + dad_rank_metrics (2 quantiles, 20 bins) on the split's score / probs / pred
  cluster        dad_cluster_metrics on the same split's embeddings, the same session
  validate       the enqueue part of validate_store: dad_eval_split
  validate_rank  the enqueue part of validate_store(ranking=True): dad_eval_split with its score / probs / pred
                 written, dad_rank_eval_columns, dad_rank_metrics (no quantiles, no bins)
  host           the route without the operator, wall clock, `--host-threads` threads: scikit-learn's roc_auc_score
                 (binary and one-vs-rest), average_precision_score, a NumPy sort per column and torch.quantile per class
  host_copy      score / probs / pred to the host, wall clock, named apart from `host`
  limit          dad_rank_metrics at n = 65,536, m = 16 on random keys, with its workspace bytes

  python tools/rank_bench.py [--out profiles/rank_metrics.json]
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import __graft_entry__ as entry  # noqa: E402
from eval_bench import make_model, make_store  # noqa: E402


def _events(fn, a, sync):
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    times = []
    for i in range(a.warmup + a.reps):
        ev[0].record()
        fn()
        ev[1].record()
        sync()
        if i >= a.warmup:
            times.append(ev[0].elapsed_time(ev[1]))
    return float(np.median(times))


def _wall(fn, a, sync):
    fn()
    sync()
    t0 = time.perf_counter()
    for _ in range(a.host_reps):
        fn()
    sync()
    return (time.perf_counter() - t0) / a.host_reps * 1e3


def _rounds(legs, a, sync):
    by_round = {k: [] for k in legs}
    for _ in range(a.rounds):
        for k, (fn, how) in legs.items():
            by_round[k].append(how(fn, a, sync))
    return {k: {"by_round_ms": v, "ms": float(np.median(v)), "spread_ms": float(max(v) - min(v))}
            for k, v in by_round.items()}


def _enqueue_columns_and_rank(PKG, out, plan, b):
    L = PKG._lib
    L.check(L.lib().dad_rank_eval_columns(L.ptr(out["score"]), L.ptr(out["probs"]), L.ptr(out["pred"]),
                                          L.ptr(plan.labels_d), plan.n, L.ptr(b["key"]), L.ptr(b["flags"]),
                                          torch.cuda.current_stream(plan.device).cuda_stream), "dad_rank_eval_columns")
    PKG.evaluate._enqueue_rank(b["key"], b["flags"], b)


def measure(PKG, dev, n, a):
    E, L = PKG.evaluate, PKG._lib
    store = make_store(PKG, dev, n, a.seed)
    model = make_model(PKG, dev, a.seed)
    model.eval()
    plan = E.EvalPlan.of(store)
    sync = lambda: torch.cuda.synchronize(dev)
    r = E.certainty_ranking_store(model, store, outputs=("emb",))
    out = {k: r[k] for k in ("score", "probs", "pred", "emb")}
    full, bare = E._ranking_buffers(plan, 2, 20), E._ranking_buffers(plan, 0, 0)
    full["gammas"].copy_(torch.tensor([0.4, 0.8]))
    cws, cblock, _ = plan.cluster_buffers()

    def validate_rank():
        o = E.enqueue_eval_split(model, plan, False, True, "fp32", ("score", "probs", "pred"))
        _enqueue_columns_and_rank(PKG, o, plan, bare)

    def host_copy():
        return [out[k].cpu().numpy() for k in ("score", "probs", "pred")]

    score_h, probs_h, pred_h = host_copy()
    labels_h = store.labels

    def host():
        from sklearn.metrics import average_precision_score, roc_auc_score
        right = pred_h == labels_h
        res = [roc_auc_score(right, score_h), roc_auc_score(right, probs_h.max(axis=1)),
               roc_auc_score(labels_h, probs_h.astype(np.float64), multi_class="ovr")]
        for c in range(4):
            sel = pred_h == c
            if 0 < (labels_h[sel] == c).sum() < sel.sum():
                res.append(roc_auc_score(labels_h[sel] == c, score_h[sel]))
            res.append(average_precision_score(labels_h == c, probs_h[:, c]))
            if sel.any():
                res.append(torch.quantile(torch.from_numpy(score_h[sel]), torch.tensor([0.4, 0.8])))
        keys = np.concatenate([np.broadcast_to(score_h, (5, n)), probs_h.max(axis=1)[None], probs_h.T])
        for j in range(10):
            np.sort(keys[j], kind="stable")
        return res

    legs = {"rank": (lambda: _enqueue_columns_and_rank(PKG, out, plan, full), _events),
            "cluster": (lambda: E._enqueue_cluster(out["emb"], plan.labels_d, cblock, None, cws), _events),
            "validate": (lambda: E.enqueue_eval_split(model, plan, False, True, "fp32", ()), _events),
            "validate_rank": (validate_rank, _events),
            "host_copy": (host_copy, _wall)}
    try:
        import sklearn  # noqa: F401
        legs["host"] = (host, _wall)
    except ImportError:
        pass
    base, on = E.validate_store(model, store), E.validate_store(model, store, ranking=True)
    if any(np.any(on[k] != v) for k, v in base.items()):
        sys.exit("ranking=True changed a key of validate_store")
    res = {"n": n, "m": L.RK_EVAL_COLUMNS, "frames": plan.frames, "legs": _rounds(legs, a, sync),
           "rank_workspace_bytes": int(full["ws"].numel()),
           "selective": r["selective"]["overall"], "auroc_ovr_macro": r["ovr"]["auroc_macro"]}
    ms = {k: v["ms"] for k, v in res["legs"].items()}
    res["added_ms_per_validation"] = ms["validate_rank"] - ms["validate"]
    res["added_over_validation"] = res["added_ms_per_validation"] / ms["validate"]
    res["rank_over_cluster"] = ms["rank"] / ms["cluster"]
    if "host" in ms:
        res["host_over_rank"] = ms["host"] / ms["rank"]
    return res


def limit(PKG, dev, a):
    E, L = PKG.evaluate, PKG._lib
    n, m = L.RK_MAX_N, L.RK_MAX_M
    g = torch.Generator(device=dev).manual_seed(a.seed)
    key = torch.rand(m, n, device=dev, generator=g)
    flags = torch.randint(0, 4, (m, n), device=dev, generator=g, dtype=torch.uint8) | 1
    b = E._rank_buffers(n, m, 2, 20, False, dev)
    b["gammas"].copy_(torch.tensor([0.4, 0.8]))
    sync = lambda: torch.cuda.synchronize(dev)
    a1 = argparse.Namespace(**dict(vars(a), warmup=1, reps=3))
    legs = _rounds({"rank_metrics": (lambda: E._enqueue_rank(key, flags, b), _events)}, a1, sync)
    ms = legs["rank_metrics"]["ms"]
    return {"n": n, "m": m, "legs": legs, "workspace_bytes": int(b["ws"].numel()), "compares": m * n * n,
            "compares_per_second": m * n * n / (ms * 1e-3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1100,5531")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--host-threads", type=int, default=16)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--seed", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("rank_bench needs the MI355X")
    if a.rounds < 3:
        sys.exit("at least 3 rounds")
    torch.set_num_threads(a.host_threads)
    PKG = entry._pkg()
    PKG.lib()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    out = {
        "what": "GPU ms between events of enqueue-only calls (host legs: wall ms), %d alternating rounds, the median "
                "of the round medians and their range; %d timed calls per leg and round" % (a.rounds, a.reps),
        "device": torch.cuda.get_device_name(dev), "abi": PKG._lib.DAD_ABI_VERSION, "host_threads": a.host_threads,
        "sizes": {"n%d" % n: measure(PKG, dev, n, a) for n in [int(v) for v in a.sizes.split(",")]},
        "limit": limit(PKG, dev, a),
        "not_measured": "no kernel trace: the split of a call between its counting, scatter and finishing launches",
    }
    txt = json.dumps(out, indent=1, sort_keys=True)
    print(txt)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()
