"""What the class-separation scores cost a validation pass (evaluate.validate_store(cluster_metrics=True),
dad_cluster_metrics behind dad_eval_split), and what they cost alone against scikit-learn.

On tools/eval_bench.py's synthetic stores (n utterances each, lengths uniform in [100, 350], one "clean", one
"noisy"), at n = 1,100 (IEMOCAP validation size) and n = 5,531 (all of IEMOCAP).  Legs, in one process:

  validate     validate_store(clean) + validate_store(noisy, teacher_disagreement=True): one epoch's validation
  validate_cm  the same two calls with cluster_metrics=True
  cluster      evaluate.cluster_metrics on the clean split's embeddings, already on the device (launches + the
               copy of the block)
  sklearn      silhouette_score + calinski_harabasz_score on the same embeddings on the host, the copy not
               counted (calculate_cluster_metrics, I/iemocap_plot_tsne.py:390-398); skipped, with a note, where
               scikit-learn is not importable

`--rounds` rounds of the legs in turn, each leg `--warmup` untimed then `--reps` timed calls (scikit-learn: one
untimed, `--sk-reps` timed), wall clock with a device synchronise at each end; the spread of a leg's round means
is the noise the differences are read against.  The GPU-only time of dad_cluster_metrics (its launches between
two HIP events) is set against the pair kernel's MFMA floor, 2 * 256 * (64 * ceil(n / 64))^2 flops at the
exact-f32 MFMA peak.

  python tools/cluster_bench.py [--out profiles/cluster_metrics.json]
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
from eval_bench import F32_MFMA_PEAK, make_model, make_store  # noqa: E402


def measure(PKG, dev, n, a):
    E = PKG.evaluate
    clean = make_store(PKG, dev, n, a.seed)
    noisy = make_store(PKG, dev, n, a.seed + 1, base=clean)
    model = make_model(PKG, dev, a.seed)
    sync = lambda: torch.cuda.synchronize(dev)
    emb = E.embed_store(model, clean)
    labels_d = clean.labels_d
    emb_h, labels_h = emb.cpu().numpy(), clean.labels

    def validate(cm):
        return (E.validate_store(model, clean, cluster_metrics=cm),
                E.validate_store(model, noisy, teacher_disagreement=True, cluster_metrics=cm))

    legs = {"validate": (lambda: validate(False), a.warmup, a.reps),
            "validate_cm": (lambda: validate(True), a.warmup, a.reps),
            "cluster": (lambda: E.cluster_metrics(emb, labels_d), a.warmup, a.reps)}
    got = E.cluster_metrics(emb, labels_d)
    res = {"n": n, "frames_clean": E.EvalPlan.of(clean).frames,
           "device_scores": {k: got[k] for k in ("silhouette_score", "calinski_harabasz_score", "class_counts")}}
    try:
        from sklearn.metrics import calinski_harabasz_score, silhouette_score
    except ImportError:
        res["sklearn"] = "scikit-learn is not importable on this machine: leg skipped"
    else:
        def sk():
            return float(silhouette_score(emb_h, labels_h)), float(calinski_harabasz_score(emb_h, labels_h))
        legs["sklearn"] = (sk, 1, a.sk_reps)
        s, c = sk()
        res["sklearn_scores"] = {"silhouette_score": s, "calinski_harabasz_score": c}
        res["device_minus_sklearn"] = {"silhouette_score": got["silhouette_score"] - s,
                                       "calinski_harabasz_relative": got["calinski_harabasz_score"] / c - 1.0}
    base, with_cm = validate(False), validate(True)
    for b, w in zip(base, with_cm):
        if any(np.any(w[k] != v) for k, v in b.items()):
            sys.exit("cluster_metrics=True changed a key of validate_store")

    wall = {k: [] for k in legs}
    for _ in range(a.rounds):
        for k, (fn, warm, reps) in legs.items():
            for _ in range(warm):
                fn()
            sync()
            t0 = time.perf_counter()
            for _ in range(reps):
                fn()
            sync()
            wall[k].append((time.perf_counter() - t0) / reps * 1e3)
    res["ms_per_call_by_round"] = wall
    res["mean_ms"] = {k: float(np.mean(v)) for k, v in wall.items()}
    res["spread_ms"] = {k: float(max(v) - min(v)) for k, v in wall.items()}
    res["added_ms_per_validation_epoch"] = res["mean_ms"]["validate_cm"] - res["mean_ms"]["validate"]
    res["added_ms_by_round"] = [c - v for c, v in zip(wall["validate_cm"], wall["validate"])]
    if "sklearn" in wall:
        res["sklearn_over_cluster"] = [s / c for s, c in zip(wall["sklearn"], wall["cluster"])]

    # GPU-only: the launches of one dad_cluster_metrics between two events
    ws = E._cluster_workspace(n, dev)
    block = torch.empty(PKG._lib.CM_SLOTS, dtype=torch.float64, device=dev)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    times = []
    for i in range(a.warmup + a.reps):
        ev[0].record()
        E._enqueue_cluster(emb, labels_d, block, None, ws)
        ev[1].record()
        sync()
        if i >= a.warmup:
            times.append(ev[0].elapsed_time(ev[1]))
    npad = 64 * (-(-n // 64))
    flops = 2.0 * 256 * npad * npad
    floor_ms = flops / F32_MFMA_PEAK * 1e3
    med = float(np.median(times))
    res["gpu_only"] = {"median_ms": med, "min_ms": float(min(times)), "max_ms": float(max(times)),
                       "pair_gflop": flops / 1e9, "mfma_floor_ms": floor_ms, "fraction_of_f32_mfma_peak": floor_ms / med,
                       "workspace_bytes": int(ws.numel())}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1100,5531")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--sk-reps", type=int, default=2)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--seed", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("cluster_bench needs the MI355X")
    if a.rounds < 3:
        sys.exit("at least 3 rounds")
    PKG = entry._pkg()
    PKG.lib()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    out = {
        "what": "validate_store on two synthetic splits (clean; noisy with the teacher) with and without "
                "cluster_metrics=True, cluster_metrics alone and scikit-learn on the clean split's embeddings; ms per "
                "call, %d rounds of the legs in turn, %d timed calls per leg and round (scikit-learn %d)"
                % (a.rounds, a.reps, a.sk_reps),
        "device": torch.cuda.get_device_name(dev), "abi": PKG._lib.DAD_ABI_VERSION,
        "host_threads": os.environ.get("OMP_NUM_THREADS", "unset"),
        "sizes": {str(n): measure(PKG, dev, n, a) for n in [int(v) for v in a.sizes.split(",")]},
    }
    txt = json.dumps(out, indent=1, sort_keys=True)
    print(txt)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()
