"""Writes tests/golden/eval_domain_gap.npz: the reference's ECDALoss (I/utils.py:510-652) on three seeded pairs of
embedding sets, in float64 and in float32, for tests/test_domain_gap_ref_cpu.py and tests/test_gpu_domain_gap.py.

Each case (n_clean, n_noisy) = (37, 29), (65, 64), (129, 140): embeddings by gen_cluster_golden.py's recipe (0.5 +
0.1 |N(0, 1)| plus a class offset), the noisy domain with a wider spread (0.13) and a per-class shift of 0.03 N(0, 1);
all four classes among the clean rows; one class with a single noisy member (its gate is closed, its centroid still
counts for the repulsion); two noisy rows labelled -1 (masked out); one noisy row an exact copy of a clean row of its
class; noisy weights uniform in [0.3, 1], class weights uniform in [0.5, 1.5] (both float32, so the float64 run
sees the values the device sees).  Stored per case (prefix c<n_clean>_), the results under f64_ and f32_:

  emb_clean, labels_clean, emb_noisy, labels_noisy, weights_noisy, class_weights, dup (clean row, noisy row), single
  class_terms [4][3]    _gaussian_kernel's (term_ss, term_tt, term_st) of each class with an open gate, zeros otherwise
  class_bw [4]          its smallest bandwidth, from the sum it took (recorded from its own torch.sum call)
  global_terms [3], global_bw    the same for all unmasked rows with unit weights (the USE_CLASS_AWARE_MMD = False
                        branch's call)
  total                 ECDALoss.forward
  gram32_terms, gram32_bw        tests/domain_gap_ref.py's float32 Gram-form restatement (class rows, then the global
                        one), for judging what the device's form of the arithmetic alone does

and lam, gamma, delta: the reference config's ECDA_CLASS_ATTENTION_LAMBDA, ECDA_COMPACTNESS_WEIGHT_GAMMA,
ECDA_REPULSION_WEIGHT_DELTA.  Needs the reference checkout (its IEMOCAP trainer directory) on the command line:

    python tests/golden/gen_domain_gap_golden.py <reference>/IEMOCAP/DAD-train-IEMOCAP

(The eval_ prefix keeps the file out of tests/goldens.py's list of step fixtures.)
"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import domain_gap_ref as R      # noqa: E402

CASES = ((37, 29, 401, 2), (65, 64, 402, 0), (129, 140, 403, 3))     # n_clean, n_noisy, seed, single-member class


def make_case(nc, nn, seed, single):
    rs = np.random.RandomState(seed)
    lc = np.array([i % 4 for i in range(nc)], dtype=np.int64)
    rs.shuffle(lc)
    big = [c for c in range(4) if c != single]
    ln = np.array([big[i % 3] for i in range(nn)], dtype=np.int64)
    rs.shuffle(ln)
    spots = rs.permutation(nn)
    ln[spots[0]] = single
    ln[spots[1:3]] = -1
    offsets = 0.08 * rs.standard_normal((4, 256))
    shift = 0.03 * rs.standard_normal((4, 256))
    ec = (0.5 + 0.1 * np.abs(rs.standard_normal((nc, 256))) + offsets[lc]).astype(np.float32)
    k = np.maximum(ln, 0)
    en = (0.5 + 0.13 * np.abs(rs.standard_normal((nn, 256))) + offsets[k] + shift[k]).astype(np.float32)
    dst = int(spots[3])
    src = int(np.where(lc == ln[dst])[0][0])
    en[dst] = ec[src]
    wn = rs.uniform(0.3, 1.0, nn).astype(np.float32)
    cw = rs.uniform(0.5, 1.5, 4).astype(np.float32)
    return ec, lc, en, ln, wn, cw, np.array([src, dst], dtype=np.int64)


class SumTap:
    """Records the results of torch.sum while active (the first call of _gaussian_kernel is sum(L2_dist))."""

    def __enter__(self):
        self.seen, self.orig = [], torch.sum
        torch.sum = lambda *a, **k: self.seen.append(self.orig(*a, **k)) or self.seen[-1]
        return self

    def __exit__(self, *exc):
        torch.sum = self.orig


def kernel_call(loss, xs, xt, ws, wt):
    with SumTap() as tap:
        terms = loss._gaussian_kernel(xs, xt, ws, wt)
    m = len(xs) + len(xt)
    bw = tap.seen[0] / (m ** 2 - m)
    bw = bw / loss.kernel_mul ** (loss.kernel_num // 2)
    return [float(t) for t in terms], float(bw)


def run_reference(ref_utils, dtype, ec, lc, en, ln, wn, cw):
    torch.set_default_dtype(dtype)          # (forward accumulates into torch.tensor(0.0))
    loss = ref_utils.ECDALoss()
    t = lambda a: torch.from_numpy(np.asarray(a)).to(dtype)
    xc, xn, w, cwt = t(ec), t(en), t(wn), t(cw)
    yc, yn = torch.from_numpy(lc), torch.from_numpy(ln)
    mask = yn >= 0
    terms, bws = np.zeros((4, 3)), np.zeros(4)
    for c in range(4):
        s, u = yc == c, (yn == c) & mask
        if int(s.sum()) >= 2 and int(u.sum()) >= 2:
            terms[c], bws[c] = kernel_call(loss, xc[s], xn[u], torch.ones(int(s.sum())), w[u])
    gt, gbw = kernel_call(loss, xc, xn[mask], torch.ones(len(xc)), torch.ones(int(mask.sum())))
    total = float(loss(xc, xn, yc, yn, mask, w, cwt))
    torch.set_default_dtype(torch.float32)
    return {"class_terms": terms, "class_bw": bws, "global_terms": np.array(gt), "global_bw": np.float64(gbw),
            "total": np.float64(total)}


def gram32(ec, lc, en, ln, wn):
    part = np.concatenate([np.ones(len(lc), bool), ln >= 0])
    mu = np.concatenate([ec, en]).astype(np.float64)[part].mean(0).astype(np.float32)
    terms, bws = np.zeros((5, 3)), np.zeros(5)
    for c in range(4):
        s, u = lc == c, ln == c
        if s.sum() >= 2 and u.sum() >= 2:
            *terms[c], bws[c] = R.gaussian_terms_f32(ec[s], en[u], np.ones(s.sum(), np.float32), wn[u], mu)
    u = ln >= 0
    *terms[4], bws[4] = R.gaussian_terms_f32(ec, en[u], np.ones(len(ec), np.float32), np.ones(u.sum(), np.float32), mu)
    return terms, bws


def main():
    sys.path.insert(0, os.path.abspath(sys.argv[1]))
    import config as ref_cfg
    import utils as ref_utils
    assert ref_cfg.USE_CLASS_AWARE_MMD
    out = {"lam": np.float64(ref_cfg.ECDA_CLASS_ATTENTION_LAMBDA),
           "gamma": np.float64(ref_cfg.ECDA_COMPACTNESS_WEIGHT_GAMMA),
           "delta": np.float64(ref_cfg.ECDA_REPULSION_WEIGHT_DELTA)}
    for nc, nn, seed, single in CASES:
        ec, lc, en, ln, wn, cw, dup = make_case(nc, nn, seed, single)
        key = "c%d_" % nc
        for name, v in (("emb_clean", ec), ("labels_clean", lc), ("emb_noisy", en), ("labels_noisy", ln),
                        ("weights_noisy", wn), ("class_weights", cw), ("dup", dup), ("single", np.int64(single))):
            out[key + name] = v
        res = {}
        for tag, dtype in (("f64", torch.float64), ("f32", torch.float32)):
            res[tag] = run_reference(ref_utils, dtype, ec, lc, en, ln, wn, cw)
            for name, v in res[tag].items():
                out["%s%s_%s" % (key, tag, name)] = v
        out[key + "gram32_terms"], out[key + "gram32_bw"] = gram32(ec, lc, en, ln, wn)
        gates = [bool(res["f64"]["class_bw"][c]) for c in range(4)]
        both = np.concatenate([res["f64"]["class_terms"].ravel(), res["f64"]["global_terms"]])
        both32 = np.concatenate([res["f32"]["class_terms"].ravel(), res["f32"]["global_terms"]])
        bw64 = np.concatenate([res["f64"]["class_bw"], [res["f64"]["global_bw"]]])
        bw32 = np.concatenate([res["f32"]["class_bw"], [res["f32"]["global_bw"]]])
        g32 = np.concatenate([out[key + "gram32_terms"][:4].ravel(), out[key + "gram32_terms"][4]])
        print("case %d + %d: gates %s  float32 - float64: term %.2e (max term %.3f)  bandwidth rel %.2e  total %.2e"
              "  |  gram32 - float64: term %.2e"
              % (nc, nn, gates, np.abs(both32 - both).max(), both.max(),
                 np.abs(bw32[bw64 > 0] / bw64[bw64 > 0] - 1).max(),
                 abs(res["f32"]["total"] - res["f64"]["total"]), np.abs(g32 - both).max()))
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "eval_domain_gap.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
