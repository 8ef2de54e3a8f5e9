"""What the clean-noisy domain gap costs (evaluate.domain_gap / domain_gap_store, dad_domain_gap), alone, behind a
validation pass, and against the host.

On tools/eval_bench.py's synthetic stores (n utterances each, lengths uniform in [100, 350], one "clean", one
"noisy"), at n = 1,100 + 1,100 (IEMOCAP validation size) and 5,531 + 5,531 (all of IEMOCAP).  Legs, in one process:

  validate      validate_store(clean) + validate_store(noisy, teacher_disagreement=True): one epoch's validation
  validate_gap  the same two calls followed by domain_gap_store(clean, noisy)
  gap           evaluate.domain_gap on the two splits' embeddings, already on the device (the concatenation, the
                launches and the copy of the block)
  cluster       evaluate.cluster_metrics on the same 2 n rows: one walk where the gap takes two and up to ten
                exponentials per pair

and, once, tests/domain_gap_ref.py (float64 NumPy, row-chunked) on the same embeddings on the host, the copy not
counted, only up to --host-max rows per split (it is O(n^2 256) on one thread).

`--rounds` rounds of the legs in turn, each leg `--warmup` untimed then `--reps` timed calls, wall clock with a device
synchronise at each end; the spread of a leg's round means is the noise the differences are read against.  The GPU-only time of dad_domain_gap (its launches between two HIP events) is set against the two
walks' MFMA floor, 2 * 2 * 256 * (64 * ceil(2 n / 64))^2 flops at the exact-f32 MFMA peak.

  python tools/domain_gap_bench.py [--out profiles/domain_gap.json]

`--reference DIR` (no GPU needed) instead times the reference's own ECDALoss.forward (DIR = its IEMOCAP trainer
directory) on the CPU on embeddings of the same recipe and sizes, float32 as the trainer runs it, and prints one JSON
object to merge under "host_reference"; its [m, m, 256] temporaries need 3 * 4 * 256 * m^2 bytes per class.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402


def synthetic(n, seed):
    """Post-ReLU-like embeddings of two domains (the recipe of tests/golden/gen_domain_gap_golden.py)."""
    rs = np.random.RandomState(seed)
    lc, ln = rs.randint(0, 4, n), rs.randint(0, 4, n)
    offsets, shift = 0.08 * rs.standard_normal((4, 256)), 0.03 * rs.standard_normal((4, 256))
    ec = (0.5 + 0.1 * np.abs(rs.standard_normal((n, 256))) + offsets[lc]).astype(np.float32)
    en = (0.5 + 0.13 * np.abs(rs.standard_normal((n, 256))) + offsets[ln] + shift[ln]).astype(np.float32)
    return ec, lc.astype(np.int64), en, ln.astype(np.int64)


def time_reference(a):
    sys.path.insert(0, os.path.abspath(a.reference))
    import utils as ref_utils
    torch.set_num_threads(a.threads)
    loss = ref_utils.ECDALoss()
    out = {"what": "the reference's ECDALoss.forward on the CPU, float32, %d threads, unit scores and class weights; "
                   "seconds per call" % a.threads, "sizes": {}}
    for n in [int(v) for v in a.sizes.split(",")]:
        need = 3 * 4 * 256 * (2 * n / 4 * 1.1) ** 2
        if need > a.host_bytes:
            out["sizes"][str(n)] = "skipped: a class of ~%d rows needs ~%.0f GB of [m, m, 256] temporaries" % (
                2 * n // 4, need / 1e9)
            continue
        ec, lc, en, ln = synthetic(n, a.seed)
        args = (torch.from_numpy(ec), torch.from_numpy(en), torch.from_numpy(lc), torch.from_numpy(ln),
                torch.ones(n, dtype=torch.bool), torch.ones(n), torch.ones(4))
        times = []
        for _ in range(1 + a.host_reps):
            t0 = time.perf_counter()
            v = float(loss(*args))
            times.append(time.perf_counter() - t0)
        out["sizes"][str(n)] = {"seconds_by_call": times[1:], "mean_s": float(np.mean(times[1:])), "ecda_loss": v}
    print(json.dumps(out, indent=1, sort_keys=True))


def measure(PKG, dev, n, a):
    from domain_gap_ref import domain_gap_ref
    from eval_bench import F32_MFMA_PEAK, make_model, make_store
    E = PKG.evaluate
    clean = make_store(PKG, dev, n, a.seed)
    noisy = make_store(PKG, dev, n, a.seed + 1, base=clean)
    model = make_model(PKG, dev, a.seed)
    sync = lambda: torch.cuda.synchronize(dev)
    emb_c, emb_n = E.embed_store(model, clean), E.embed_store(model, noisy)
    lab_c, lab_n = clean.labels_d, noisy.labels_d
    both, lab_both = torch.cat([emb_c, emb_n]), torch.cat([lab_c, lab_n])

    def validate(gap):
        r = (E.validate_store(model, clean), E.validate_store(model, noisy, teacher_disagreement=True))
        return r + ((E.domain_gap_store(model, clean, noisy),) if gap else ())

    legs = {"validate": (lambda: validate(False), a.warmup, a.reps),
            "validate_gap": (lambda: validate(True), a.warmup, a.reps),
            "gap": (lambda: E.domain_gap(emb_c, lab_c, emb_n, lab_n), a.warmup, a.reps),
            "cluster": (lambda: E.cluster_metrics(both, lab_both), a.warmup, a.reps)}
    got = E.domain_gap(emb_c, lab_c, emb_n, lab_n)
    res = {"n_per_split": n, "rows": 2 * n,
           "device": {"mmd_global": got["global"]["mmd"], "mmd_class_mean": got["mmd_class_mean"],
                      "ecda_loss": got["ecda_loss"], "gates": got["per_class"]["gate"]}}
    if n <= a.host_max:
        x = both.cpu().numpy()
        y = lab_both.cpu().numpy()
        dom = np.concatenate([np.zeros(n, np.uint8), np.ones(n, np.uint8)])
        t0 = time.perf_counter()
        ref = domain_gap_ref(x, y, dom)
        res["host_ref_ms"] = (time.perf_counter() - t0) * 1e3
        res["device_minus_host_ref"] = {"mmd_global": got["global"]["mmd"] - ref["global"]["mmd"],
                                        "ecda_loss": got["ecda_loss"] - ref["ecda_loss"]}
    else:
        res["host_ref"] = "skipped above %d rows per split (O(n^2 256) NumPy on one thread)" % a.host_max
    base, with_gap = validate(False), validate(True)
    for b, w in zip(base, with_gap):
        if any(np.any(w[k] != v) for k, v in b.items()):
            sys.exit("a following domain_gap_store changed a key of validate_store")

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
    res["added_ms_per_validation_epoch"] = res["mean_ms"]["validate_gap"] - res["mean_ms"]["validate"]
    res["added_ms_by_round"] = [g - v for g, v in zip(wall["validate_gap"], wall["validate"])]
    res["gap_over_cluster"] = [g / c for g, c in zip(wall["gap"], wall["cluster"])]
    if "host_ref_ms" in res:
        res["host_ref_over_gap"] = res["host_ref_ms"] / res["mean_ms"]["gap"]

    # GPU-only: the launches of one dad_domain_gap between two events
    rows = 2 * n
    ws = E._domain_gap_workspace(rows, dev)
    block = torch.empty(PKG._lib.DG_SLOTS, dtype=torch.float64, device=dev)
    domain = torch.cat([torch.zeros(n, dtype=torch.uint8, device=dev), torch.ones(n, dtype=torch.uint8, device=dev)])
    args = E._domain_gap_args(None, None)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    times = []
    for i in range(a.warmup + a.reps):
        ev[0].record()
        E._enqueue_domain_gap(both, lab_both, domain, None, args, block, ws)
        ev[1].record()
        sync()
        if i >= a.warmup:
            times.append(ev[0].elapsed_time(ev[1]))
    npad = 64 * (-(-rows // 64))
    flops = 2 * 2.0 * 256 * npad * npad
    floor_ms = flops / F32_MFMA_PEAK * 1e3
    med = float(np.median(times))
    res["gpu_only"] = {"median_ms": med, "min_ms": float(min(times)), "max_ms": float(max(times)),
                       "walks_gflop": flops / 1e9, "mfma_floor_ms": floor_ms, "fraction_of_f32_mfma_peak": floor_ms / med,
                       "workspace_bytes": int(ws.numel())}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1100,5531")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--seed", type=int, default=5)
    ap.add_argument("--host-max", type=int, default=1100)
    ap.add_argument("--reference", default=None)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--host-reps", type=int, default=2)
    ap.add_argument("--host-bytes", type=float, default=32e9)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.reference:
        return time_reference(a)
    if not torch.cuda.is_available():
        sys.exit("domain_gap_bench needs the MI355X")
    if a.rounds < 3:
        sys.exit("at least 3 rounds")
    import __graft_entry__ as entry
    PKG = entry._pkg()
    PKG.lib()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    out = {
        "what": "validate_store on two synthetic splits (clean; noisy with the teacher) with and without a following "
                "domain_gap_store, domain_gap alone, cluster_metrics on the same rows (and the float64 host restatement, once); "
                "ms per call, %d rounds of the legs in turn, %d timed calls per leg and round"
                % (a.rounds, a.reps),
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
