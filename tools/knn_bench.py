"""What the exact k-NN of a split's embeddings and the trustworthiness of a map cost on the device, beside
cluster_metrics (one Gram walk like dad_knn: the difference is the price of the selection) and beside scikit-learn.

On tools/eval_bench.py's synthetic stores, at n = 1,100 (IEMOCAP validation size) and n = 5,531 (all of IEMOCAP), for
k = 5 and k = 32, on the clean split's embeddings, already on the device, and their PCA map.  Legs, in one process:

  knn        evaluate.knn (launches + the read of the non-finite word: the lists stay on the device)
  knn_copy   evaluate.knn and the copy of idx and d2 to the host
  trust      evaluate.trustworthiness (launches + the copy of the block)
  cluster    evaluate.cluster_metrics on the same rows (launches + the copy of the block)
  sk_knn     NearestNeighbors(algorithm='brute').fit(emb).kneighbors() on the host, the copy not counted
  sk_trust   sklearn.manifold.trustworthiness(emb, Y) on the host
             (both skipped, with a note, where scikit-learn is not importable)

`--rounds` rounds of the legs in turn, each leg `--warmup` untimed then `--reps` timed calls (scikit-learn: one
untimed, `--sk-reps` timed), wall clock with a device synchronise at each end; the spread of a leg's round means is
the noise the differences are read against.  The GPU-only times (the launches of one call between two HIP events) of
dad_knn, dad_trustworthiness and dad_cluster_metrics are set against the walk's MFMA floor, 2 * 256 * (64 *
ceil(n / 64))^2 flops at the exact-f32 MFMA peak.

  python tools/knn_bench.py [--out profiles/knn.json]
"""
import argparse
import ctypes
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import __graft_entry__ as entry  # noqa: E402
from eval_bench import F32_MFMA_PEAK, make_model, make_store  # noqa: E402


def gpu_only(fn, sync, warmup, reps):
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    times = []
    for i in range(warmup + reps):
        ev[0].record()
        fn()
        ev[1].record()
        sync()
        if i >= warmup:
            times.append(ev[0].elapsed_time(ev[1]))
    return {"median_ms": float(np.median(times)), "min_ms": float(min(times)), "max_ms": float(max(times))}


def measure(PKG, dev, n, k, a):
    E, L = PKG.evaluate, PKG._lib
    clean = make_store(PKG, dev, n, a.seed)
    model = make_model(PKG, dev, a.seed)
    sync = lambda: torch.cuda.synchronize(dev)
    emb = E.embed_store(model, clean)
    labels_d = clean.labels_d
    Y = E.tsne_pca_init(emb)
    Y = (Y / Y.abs().max()).contiguous()
    emb_h, Y_h = emb.cpu().numpy(), Y.cpu().numpy()

    def knn_copy():
        idx, d2 = E.knn(emb, k)
        return idx.cpu(), d2.cpu()

    legs = {"knn": (lambda: E.knn(emb, k), a.warmup, a.reps),
            "knn_copy": (knn_copy, a.warmup, a.reps),
            "trust": (lambda: E.trustworthiness(emb, Y, k), a.warmup, a.reps),
            "cluster": (lambda: E.cluster_metrics(emb, labels_d), a.warmup, a.reps)}
    idx, d2 = knn_copy()
    tw = E.trustworthiness(emb, Y, k)
    acc = E.knn_accuracy(emb, labels_d, k)
    plan = [ctypes.c_int() for _ in range(3)]
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    L.check(L.require("dad_knn_plan", "knn")(n, k, cus, *plan), "dad_knn_plan")
    res = {"n": n, "k": k, "compute_units": cus,
           "plan": {"row_tiles": plan[0].value, "chunks": plan[1].value, "tiles_per_chunk": plan[2].value},
           "device": {"trustworthiness": tw["trustworthiness"], "penalty_sum": tw["penalty_sum"],
                      "knn_accuracy": acc["accuracy"]}}
    try:
        from sklearn.manifold import trustworthiness
        from sklearn.neighbors import NearestNeighbors
    except ImportError:
        res["sklearn"] = "scikit-learn is not importable on this machine: legs skipped"
    else:
        sk_knn = lambda: NearestNeighbors(n_neighbors=k, algorithm="brute").fit(emb_h).kneighbors()
        sk_tw = lambda: float(trustworthiness(emb_h, Y_h, n_neighbors=k))
        legs["sk_knn"] = (sk_knn, 1, a.sk_reps)
        legs["sk_trust"] = (sk_tw, 1, a.sk_reps)
        _, sk_idx = sk_knn()
        res["sklearn_values"] = {"trustworthiness": sk_tw(),
                                 "rows_with_the_same_list": int((sk_idx == idx.numpy()).all(1).sum())}
        res["device_minus_sklearn_trustworthiness"] = tw["trustworthiness"] - res["sklearn_values"]["trustworthiness"]

    wall = {name: [] for name in legs}
    for _ in range(a.rounds):
        for name, (fn, warm, reps) in legs.items():
            for _ in range(warm):
                fn()
            sync()
            t0 = time.perf_counter()
            for _ in range(reps):
                fn()
            sync()
            wall[name].append((time.perf_counter() - t0) / reps * 1e3)
    res["ms_per_call_by_round"] = wall
    res["mean_ms"] = {name: float(np.mean(v)) for name, v in wall.items()}
    res["median_ms"] = {name: float(np.median(v)) for name, v in wall.items()}
    res["spread_ms"] = {name: float(max(v) - min(v)) for name, v in wall.items()}
    if "sk_knn" in wall:
        res["sklearn_over_device"] = {"knn": res["mean_ms"]["sk_knn"] / res["mean_ms"]["knn_copy"],
                                      "trustworthiness": res["mean_ms"]["sk_trust"] / res["mean_ms"]["trust"]}

    # GPU-only: the launches of one call between two events
    ws = E._knn_workspace(n, k, dev)
    idx_d = torch.empty(n, k, dtype=torch.int32, device=dev)
    d2_d = torch.empty(n, k, dtype=torch.float32, device=dev)
    out = torch.empty(L.TW_SLOTS, dtype=torch.float64, device=dev)
    cws = E._cluster_workspace(n, dev)
    block = torch.empty(L.CM_SLOTS, dtype=torch.float64, device=dev)
    npad = 64 * (-(-n // 64))
    flops = 2.0 * 256 * npad * npad
    floor_ms = flops / F32_MFMA_PEAK * 1e3
    g = {"knn": gpu_only(lambda: E._enqueue_knn(emb, None, k, L.KNN_ALL, idx_d, d2_d, ws), sync, a.warmup, a.reps),
         "trust": gpu_only(lambda: E._enqueue_trustworthiness(emb, Y, k, out, None, ws), sync, a.warmup, a.reps),
         "cluster": gpu_only(lambda: E._enqueue_cluster(emb, labels_d, block, None, cws), sync, a.warmup, a.reps)}
    for v in g.values():
        v["fraction_of_f32_mfma_peak"] = floor_ms / v["median_ms"]
    res["gpu_only"] = dict(g, walk_gflop=flops / 1e9, mfma_floor_ms=floor_ms, knn_workspace_bytes=int(ws.numel()),
                           knn_over_cluster=g["knn"]["median_ms"] / g["cluster"]["median_ms"])
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1100,5531")
    ap.add_argument("--ks", default="5,32")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--sk-reps", type=int, default=2)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--seed", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("knn_bench needs the MI355X")
    if a.rounds < 3:
        sys.exit("at least 3 rounds")
    PKG = entry._pkg()
    PKG.lib()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    out = {
        "what": "knn, trustworthiness and cluster_metrics on a synthetic split's embeddings, and scikit-learn's "
                "NearestNeighbors(brute) and trustworthiness on the same rows; ms per call, %d rounds of the legs in "
                "turn, %d timed calls per leg and round (scikit-learn %d)" % (a.rounds, a.reps, a.sk_reps),
        "device": torch.cuda.get_device_name(dev), "abi": PKG._lib.DAD_ABI_VERSION,
        "host_threads": os.environ.get("OMP_NUM_THREADS", "unset"),
        "cases": {"n%d_k%d" % (n, k): measure(PKG, dev, n, k, a)
                  for n in [int(v) for v in a.sizes.split(",")] for k in [int(v) for v in a.ks.split(",")]},
    }
    txt = json.dumps(out, indent=1, sort_keys=True)
    print(txt)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()
