"""Bit identity of the pairwise evaluators (cluster, t-SNE, domain gap, k-NN) and of their planners between two builds
of the library, for a refactor of csrc/pairwise.h and the units on it.

  DAD_LIB_VARIANT=parent python tools/pairwise_identity.py dump  parent.npz     (on the MI355X, a process per library)
  python tools/pairwise_identity.py dump  new.npz
  DAD_LIB_VARIANT=parent python tools/pairwise_identity.py plans parent_plans.npz     (host only)
  python tools/pairwise_identity.py plans new_plans.npz
  python tools/pairwise_identity.py compare parent.npz new.npz [--json out.json]

`dump` writes every output of the four evaluators on seeded synthetic inputs for the library DAD_LIB_VARIANT names
(tools/build_old.py builds a commit's): n = 65, 129, 257 and 1,100 rows of post-ReLU-like embeddings in 4 classes and
two domains, non-uniform weights, one exact duplicate row, a few rows with label -1 (group -1); chunks the planner's
(c0), 1 and 3.  Per n and chunk count: the DAD_CM_* block and silhouette_samples; tsne_gradient's block and grad; the
DAD_DG_* block; knn idx and d2 in the three modes at k = 5 and 17; trustworthiness' block and penalties at k = 5 and
17.  Per n: P and beta, the vote's block and pred.  `plans` writes the answers and return codes of the five planners
over a grid of (n, compute units), range edges and NULL pointers included, dad_knn_plan at k = 1, 16, 17, 32.
`compare` reads two such files and counts the bytes that differ, array by array (names, shapes and dtypes must agree);
exit status 1 unless that count is 0.
"""
import argparse
import ctypes
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

SIZES = (65, 129, 257, 1100)
CHUNKS = (0, 1, 3)
KS = (5, 17)


def inputs(n, seed):
    rs = np.random.RandomState(seed)
    labels = rs.randint(0, 4, n).astype(np.int64)
    labels[rs.permutation(n)[:3]] = -1
    domain = (rs.rand(n) < 0.45).astype(np.int64)
    offsets = 0.08 * rs.standard_normal((4, 256))
    emb = np.maximum(0.5 + 0.12 * rs.standard_normal((n, 256)) + offsets[np.maximum(labels, 0)] +
                     0.03 * domain[:, None], 0.0).astype(np.float32)
    emb[n - 2] = emb[5]                                    # an exact duplicate, across a tile edge for n > 64
    labels[n - 2], labels[5] = 1, 1
    weights = (0.3 + 0.7 * rs.rand(n)).astype(np.float32)
    Y = rs.standard_normal((n, 2)).astype(np.float32)
    return emb, labels, domain, weights, Y


def dump(path):
    import torch

    import __graft_entry__ as entry
    PKG = entry._pkg()
    PKG.lib()
    E = PKG.evaluate
    dev = torch.device("cuda", 0)
    out = {}
    host = lambda t: t.detach().cpu().numpy()
    for n in SIZES:
        emb_h, labels_h, domain_h, weights_h, Y_h = inputs(n, 400 + n)
        emb, labels, Y = (torch.from_numpy(v).to(dev) for v in (emb_h, labels_h, Y_h))
        domain = torch.from_numpy(domain_h).to(dev)
        group = E._knn_group(labels, domain)
        order = np.argsort(domain_h, kind="stable")       # domain_gap takes the clean rows first
        nc = int((domain_h == 0).sum())
        dg = [torch.from_numpy(v[order]).to(dev) for v in (emb_h, labels_h, weights_h)]
        key = lambda name: "n%d_%s" % (n, name)
        P, beta = E.tsne_affinities(emb, perplexity=30.0, beta=True)
        out[key("ts_P")], out[key("ts_beta")] = host(P), host(beta)
        vote = E.knn_accuracy(emb, labels, k=5, domain=domain, mode="other")
        vote = vote[0] if vote[0] is not None else vote[1]
        out[key("kv_block")], out[key("kv_pred")] = np.asarray(vote["block"]), host(vote["pred"])
        for c in CHUNKS:
            ck = lambda name: key("%s_c%d" % (name, c))
            r = E.cluster_metrics(emb, labels, samples=True, _chunks=c)
            out[ck("cm_block")], out[ck("cm_sil")] = np.asarray(r["block"]), host(r["silhouette_samples"])
            r = E.tsne_gradient(P, Y, exaggeration=12.0, _chunks=c)
            out[ck("ts_block")] = np.array([r["kl_divergence"], r["z"], r["grad_norm"]], dtype=np.float64)
            out[ck("ts_grad")] = host(r["grad"])
            r = E.domain_gap(dg[0][:nc], dg[1][:nc], dg[0][nc:], dg[1][nc:], weights_noisy=dg[2][nc:],
                             class_weights=[0.7, 1.0, 1.3, 0.9], _chunks=c)
            out[ck("dg_block")] = np.asarray(r["block"])
            for k in KS:
                for mode in ("all", "same", "other"):
                    idx, d2 = E.knn(emb, k=k, group=group, mode=mode, _chunks=c)
                    out[ck("knn_%s_k%d_idx" % (mode, k))], out[ck("knn_%s_k%d_d2" % (mode, k))] = host(idx), host(d2)
                r = E.trustworthiness(emb, Y, k=k, samples=True, _chunks=c)
                out[ck("tw_k%d_block" % k)], out[ck("tw_k%d_penalty" % k)] = np.asarray(r["block"]), host(r["penalty"])
    np.savez(path, **out)
    print("%s: %d arrays, %d bytes, library %s" % (path, len(out), sum(v.nbytes for v in out.values()),
                                                   os.environ.get("DAD_LIB_VARIANT") or "(the tree's)"))


def plans(path):
    import __graft_entry__ as entry
    L = entry._pkg()._lib
    lib = L.lib()
    ns = sorted(set(range(-1, 4300)) | {64 * t + d for t in range(1, 1025) for d in (-1, 0, 1)} | {16384, 16385, 65537})
    cus = (0, 1, 8, 32, 64, 104, 228, 256, 304)
    v = [ctypes.c_int() for _ in range(3)]
    ref = [ctypes.byref(x) for x in v]
    planners = [(name, getattr(lib, name), ()) for name in ("dad_cluster_plan", "dad_tsne_plan", "dad_domain_gap_plan",
                                                            "dad_scl_plan")]
    planners += [("dad_knn_plan_k%d" % k, lib.dad_knn_plan, (k,)) for k in (0, 1, 16, 17, 32, 33)]
    out = {"grid_n": np.array(ns, dtype=np.int64), "grid_cus": np.array(cus, dtype=np.int64)}
    for name, fn, pre in planners:
        a = np.empty((len(ns), len(cus), 4), dtype=np.int32)
        for i, n in enumerate(ns):
            for j, c in enumerate(cus):
                for x in v:
                    x.value = -7
                rc = fn(n, *pre, c, *ref)
                a[i, j] = (rc, v[0].value, v[1].value, v[2].value)
        out[name] = a
        out[name + "_null"] = np.array([fn(1100, *pre, 256, *(ref[:q] + [None] + ref[q + 1:])) for q in range(3)],
                                       dtype=np.int32)
    np.savez(path, **out)
    print("%s: %d planners x %d (n, compute units) pairs" % (path, len(planners), len(ns) * len(cus)))


def compare(a_path, b_path, json_path):
    a, b = np.load(a_path), np.load(b_path)
    names = sorted(set(a.files) | set(b.files))
    res = {"arrays_compared": 0, "bytes_compared": 0, "mismatching_bytes": 0, "mismatches": [], "arrays": names}
    for name in names:
        if name not in a.files or name not in b.files:
            res["mismatches"].append({"array": name, "why": "in one file only"})
            continue
        x, y = a[name], b[name]
        if x.shape != y.shape or x.dtype != y.dtype:
            res["mismatches"].append({"array": name, "why": "%s %s against %s %s" % (x.dtype, x.shape, y.dtype, y.shape)})
            continue
        bad = int((np.frombuffer(x.tobytes(), np.uint8) != np.frombuffer(y.tobytes(), np.uint8)).sum())
        res["arrays_compared"] += 1
        res["bytes_compared"] += x.nbytes
        res["mismatching_bytes"] += bad
        if bad:
            res["mismatches"].append({"array": name, "mismatching_bytes": bad})
    ok = not res["mismatches"]
    print("%d arrays, %d bytes compared, %d mismatching bytes%s" % (
        res["arrays_compared"], res["bytes_compared"], res["mismatching_bytes"],
        "" if ok else ": " + ", ".join(m["array"] for m in res["mismatches"][:20])))
    if json_path:
        with open(json_path, "w") as f:
            f.write(json.dumps(res, indent=1, sort_keys=True) + "\n")
    return 0 if ok else 1


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("what", choices=("dump", "plans", "compare"))
    ap.add_argument("paths", nargs="+")
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    if args.what == "compare":
        if len(args.paths) != 2:
            ap.error("compare takes two files")
        return compare(args.paths[0], args.paths[1], args.json)
    if len(args.paths) != 1:
        ap.error("%s takes one file" % args.what)
    (dump if args.what == "dump" else plans)(args.paths[0])
    return 0


if __name__ == "__main__":
    sys.exit(main())
