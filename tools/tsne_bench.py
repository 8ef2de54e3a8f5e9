"""What the exact t-SNE of a split's embeddings costs on the device (evaluate.tsne*, csrc/tsne.hip), stage by stage,
and what scikit-learn's costs on the host.

On the embed_store embeddings of tools/eval_bench.py's synthetic stores (n utterances, lengths uniform in
[100, 350]), at n = 1,100 (IEMOCAP validation size) and n = 5,531 (all of IEMOCAP).  Legs, in one process:

  affinities   evaluate.tsne_affinities (the joint distribution P; launches + the copy of the non-finite count)
  run          evaluate.tsne from a fixed random start on a given P: the 1,000-iteration descent (2,001 launches + the
               copy of the result block)
  tsne         evaluate.tsne(init='pca'): affinities, the PCA start and the run
  iteration    one force + one step launch of the run between two HIP events (mean over a 200-iteration run with
               the stop rules off), against the bytes of P at 6.3 TB/s (the HBM copy rate of MI355X_MICROARCH.md),
               15 n^2 VALU operations at 78.6 T/s (256 CUs x 128 lanes x 2.4 GHz) and two kernel boundaries of 1.5 us
  sklearn_bh   TSNE(n_components=2, perplexity=30, max_iter=1000, init='pca', learning_rate='auto',
               random_state=42) as run_tsne makes it (I/iemocap_plot_tsne.py:310-323: Barnes-Hut), the host copy
               not counted
  sklearn_exact  the same with method='exact', at n = 1,100 only
               (both skipped, with a note, where scikit-learn is not importable; one timed call each)

`--rounds` rounds of the device legs in turn, each leg `--warmup` untimed then `--reps` timed calls, wall clock with
a device synchronise at each end; the spread of a leg's round means is the noise the figures are read against.

  python tools/tsne_bench.py [--out profiles/tsne.json]
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
from eval_bench import make_model, make_store  # noqa: E402

HBM_RATE = 6.3e12          # bytes / s, float4 copy
VALU_RATE = 78.6e12        # fp32 operations / s
BOUNDARY_US = 1.5          # dependent kernel boundary on one stream


def measure(PKG, dev, n, a):
    E, L = PKG.evaluate, PKG._lib
    store = make_store(PKG, dev, n, a.seed)
    model = make_model(PKG, dev, a.seed)
    sync = lambda: torch.cuda.synchronize(dev)
    emb = E.embed_store(model, store)
    emb_h = emb.cpu().numpy()
    P = E.tsne_affinities(emb, a.perplexity)
    y0 = (1e-4 * torch.randn(n, 2, generator=torch.Generator().manual_seed(a.seed))).to(dev)

    legs = {"affinities": lambda: E.tsne_affinities(emb, a.perplexity),
            "run": lambda: E.tsne(emb, a.perplexity, init=y0, _P=P),
            "tsne": lambda: E.tsne(emb, a.perplexity)}
    got = E.tsne(emb, a.perplexity)
    res = {"n": n, "perplexity": a.perplexity, "p_bytes": int(P.numel() * 4),
           "device": {"kl_divergence": got["kl_divergence"], "n_iter": got["n_iter"]}}
    plan = [ctypes.c_int() for _ in range(3)]
    L.require("dad_tsne_plan", "tsne")(n, torch.cuda.get_device_properties(dev).multi_processor_count,
                                       *[ctypes.byref(v) for v in plan])
    res["plan"] = {"row_tiles": plan[0].value, "chunks": plan[1].value, "tiles_per_chunk": plan[2].value}

    wall = {k: [] for k in legs}
    for _ in range(a.rounds):
        for k, fn in legs.items():
            for _ in range(a.warmup):
                fn()
            sync()
            t0 = time.perf_counter()
            for _ in range(a.reps):
                fn()
            sync()
            wall[k].append((time.perf_counter() - t0) / a.reps * 1e3)
    res["ms_per_call_by_round"] = wall
    res["mean_ms"] = {k: float(np.mean(v)) for k, v in wall.items()}
    res["spread_ms"] = {k: float(max(v) - min(v)) for k, v in wall.items()}

    # GPU-only: a 200-iteration run that cannot stop, between two events
    iters = 200
    ws = E._tsne_workspace(n, dev)
    hist, out = E.tsne_run_buffers(n, iters, dev)
    Y = torch.empty_like(y0)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    times = []
    for i in range(a.warmup + a.reps):
        Y.copy_(y0)
        ev[0].record()
        E.enqueue_tsne_run(P, Y, hist, out, ws, max_iter=iters, min_grad_norm=0.0, n_iter_without_progress=10 ** 6)
        ev[1].record()
        sync()
        if i >= a.warmup:
            times.append(ev[0].elapsed_time(ev[1]) / iters * 1e3)
    assert int(out[L.TS_N_ITER]) == iters - 1
    floors = {"p_bytes_us": res["p_bytes"] / HBM_RATE * 1e6, "valu_us": 15.0 * n * n / VALU_RATE * 1e6,
              "boundaries_us": 2 * BOUNDARY_US}
    med = float(np.median(times))
    res["iteration"] = {"median_us": med, "min_us": float(min(times)), "max_us": float(max(times)), "floors": floors,
                        "p_bytes_floor_fraction": floors["p_bytes_us"] / med, "p_read_TBps": res["p_bytes"] / med / 1e6,
                        "workspace_bytes": int(ws.numel())}

    try:
        from sklearn.manifold import TSNE
    except ImportError:
        res["sklearn"] = "scikit-learn is not importable on this machine: legs skipped"
        return res
    sk = {}
    for name, kw in (("sklearn_bh", {}), ("sklearn_exact", {"method": "exact"})):
        if name == "sklearn_exact" and n > a.exact_max_n:
            continue
        ts = TSNE(n_components=2, perplexity=a.perplexity, max_iter=1000, init="pca", learning_rate="auto",
                  random_state=42, **kw)
        t0 = time.perf_counter()
        ts.fit_transform(emb_h)
        sk[name] = {"ms": (time.perf_counter() - t0) * 1e3, "kl_divergence": float(ts.kl_divergence_),
                    "n_iter": int(ts.n_iter_)}
    res["sklearn"] = sk
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1100,5531")
    ap.add_argument("--perplexity", type=float, default=30.0)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--exact-max-n", type=int, default=1100)
    ap.add_argument("--seed", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("tsne_bench needs the MI355X")
    if a.rounds < 3:
        sys.exit("at least 3 rounds")
    PKG = entry._pkg()
    PKG.lib()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    out = {
        "what": "exact t-SNE of a synthetic split's embeddings on the device: affinities, the 1,000-iteration run, both "
                "with the PCA start, one iteration between events against its floors; scikit-learn's Barnes-Hut and exact "
                "calls on the host (one timed call each); ms per call, %d rounds of the device legs in turn, %d timed "
                "calls per leg and round" % (a.rounds, a.reps),
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
