"""One epoch of validation, per-batch path against the whole-split evaluator.

Two synthetic stores of IEMOCAP validation size (n utterances each, lengths uniform in [100, 350],
seeded; one "clean", one "noisy").  One epoch of validation = validate(clean) + validate(noisy,
teacher_disagreement=True), the two calls the trainer loop of INTEGRATION.md makes after every epoch.

  baseline   evaluate.validate over DeviceLoaders of batch 64 (dad_collate + dad_encoder_forward +
             dad_predict_head per batch, a second sweep for the teacher, scikit-learn at the end)
  store fp32 evaluate.validate_store (one dad_eval_split per split), exact-f32 MFMA
  store fp16 the same with FP16 operands

Wall clock with a device synchronise at each end, 3 warm-up repetitions, then `--reps` repetitions
with the three variants interleaved (all see the same clock state); median / min / max.  The GPU-only
time of the new call (its launches between two HIP events, no copy) is measured separately, and the
fp32 call's time is set against its MFMA floor: 2 * 768 * 256 * frames * networks flops at the
exact-f32 MFMA peak (157.3 TFLOP/s).  Results are compared before anything is timed.

  python tools/eval_bench.py [--n 1100] [--reps 20] [--out profiles/eval_split.json]
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import __graft_entry__ as entry  # noqa: E402

F32_MFMA_PEAK = 157.3e12      # v_mfma_f32_32x32x2_f32, 256 CUs at 2.4 GHz


def make_store(PKG, dev, n, seed, base=None):
    """n utterances, lengths uniform in [100, 350]; N(0, 1) features drawn on the device.  With `base`
    (the clean store) the noisy one is the same utterances plus N(0, 0.5^2) noise."""
    rs = np.random.RandomState(seed)
    sizes = rs.randint(100, 351, n) if base is None else base.sizes
    offsets = np.concatenate([[0], np.cumsum(sizes)[:-1]])
    labels = rs.randint(0, 4, n) if base is None else base.labels
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    feats = torch.randn(int(sizes.sum()), 768, device=dev, generator=g)
    if base is not None:
        feats = base.feats + 0.5 * feats
    return PKG.data.FeatureStore(feats, sizes, offsets, labels, device=dev)


def make_model(PKG, dev, seed):
    torch.manual_seed(seed)
    model = PKG.SSRLModel().to(dev)
    with torch.no_grad():       # a teacher that is not the student, so the disagreement count is not trivially 0
        g = torch.Generator(device=dev)
        g.manual_seed(seed + 1)
        model.teacher_flat.add_(0.01 * torch.randn(model.teacher_flat.shape, device=dev, generator=g))
    return model


def stats(xs):
    xs = np.asarray(xs) * 1e3
    return {"median_ms": float(np.median(xs)), "min_ms": float(xs.min()), "max_ms": float(xs.max()), "reps": len(xs)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1100)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--seed", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("eval_bench needs the MI355X")
    PKG = entry._pkg()
    PKG.lib()
    E = PKG.evaluate
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    clean = make_store(PKG, dev, a.n, a.seed)
    noisy = make_store(PKG, dev, a.n, a.seed + 1, base=clean)
    model = make_model(PKG, dev, a.seed)
    cl, nl = PKG.DeviceLoader(clean, a.batch), PKG.DeviceLoader(noisy, a.batch)
    sync = lambda: torch.cuda.synchronize(dev)

    def baseline():
        return E.validate(model, cl), E.validate(model, nl, teacher_disagreement=True)

    def store(precision):
        return (E.validate_store(model, clean, precision=precision),
                E.validate_store(model, noisy, teacher_disagreement=True, precision=precision))

    variants = {"baseline": baseline, "store_fp32": lambda: store("fp32"), "store_fp16": lambda: store("fp16")}

    # results first: the fp32 store path must report what the per-batch path reports
    ref = baseline()
    got = {k: store(k) for k in ("fp32", "fp16")}
    same = {}
    for k, rs in got.items():
        diff = [int(np.abs(r["confusion_matrix"] - b["confusion_matrix"]).sum()) // 2 for r, b in zip(rs, ref)]
        same[k] = {"changed_predictions_clean": diff[0], "changed_predictions_noisy": diff[1],
                   "disagreement_rate": rs[1]["disagreement_rate"]}
    same["baseline"] = {"disagreement_rate": ref[1]["disagreement_rate"], "accuracy_clean": ref[0]["accuracy"],
                        "accuracy_noisy": ref[1]["accuracy"]}
    if same["fp32"]["changed_predictions_clean"] or same["fp32"]["changed_predictions_noisy"] \
            or got["fp32"][1]["disagreement_rate"] != ref[1]["disagreement_rate"]:
        sys.exit("fp32 store path disagrees with validate(): %s" % json.dumps(same))

    for _ in range(a.warmup):
        for fn in variants.values():
            fn()
    wall = {k: [] for k in variants}
    for _ in range(a.reps):
        for k, fn in variants.items():       # interleaved: every variant sees the same clock state
            sync()
            t0 = time.perf_counter()
            fn()
            sync()
            wall[k].append(time.perf_counter() - t0)

    # GPU-only time of the new call: its launches between two events (no copy, no host work in between)
    gpu = {}
    frames = {"clean": E.EvalPlan.of(clean).frames, "noisy": E.EvalPlan.of(noisy).frames}
    # the same clean rows as an fp16 store: half the store bytes, the same W1 traffic and MFMA work (what
    # the FP16 mode's time follows tells which of them bounds it)
    clean16 = PKG.data.FeatureStore(clean.feats, clean.sizes, clean.offsets, clean.labels, device=dev,
                                    dtype=torch.float16)
    frames["clean_f16store"] = frames["clean"]
    for prec in ("fp32", "fp16"):
        for name, st, teach in (("clean", clean, False), ("noisy", noisy, True), ("clean_f16store", clean16, False)):
            plan = E.EvalPlan.of(st)
            ts = []
            for r in range(a.warmup + a.reps):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                sync()
                e0.record()
                E.enqueue_eval_split(model, plan, use_teacher=teach, precision=prec)
                e1.record()
                sync()
                if r >= a.warmup:
                    ts.append(e0.elapsed_time(e1) * 1e-3)
            s = stats(ts)
            nets = 2 if teach else 1
            s["frames"], s["networks"] = frames[name], nets
            s["flops"] = 2.0 * 768 * 256 * frames[name] * nets
            s["tflops_at_median"] = s["flops"] / (s["median_ms"] * 1e-3) / 1e12
            if prec == "fp32":
                s["mfma_floor_ms"] = s["flops"] / F32_MFMA_PEAK * 1e3
                s["fraction_of_floor_at_median"] = s["mfma_floor_ms"] / s["median_ms"]
            s["store_bytes"] = frames[name] * 768 * st.feats.element_size()
            # every slab's wave reads its networks' whole W1 (from L2 after the first)
            s["w1_bytes_read"] = plan.slabs * nets * 256 * 768 * (4 if prec == "fp32" else 2)
            s["w1_gbps_at_median"] = s["w1_bytes_read"] / (s["median_ms"] * 1e-3) / 1e9
            s["store_gbps_at_median"] = s["store_bytes"] / (s["median_ms"] * 1e-3) / 1e9
            gpu["%s_%s" % (prec, name)] = s

    out = {
        "what": "one epoch of validation: validate(clean) + validate(noisy, teacher_disagreement=True)",
        "n_utterances_per_split": a.n, "frames": frames, "batch_size_baseline": a.batch,
        "slabs": {"clean": E.EvalPlan.of(clean).slabs, "noisy": E.EvalPlan.of(noisy).slabs},
        "device": torch.cuda.get_device_name(dev),
        "wall": {k: stats(v) for k, v in wall.items()},
        "gpu_only_new_call": gpu,
        "results": same,
    }
    w = out["wall"]
    out["new_max_below_baseline_min"] = {k: w[k]["max_ms"] < w["baseline"]["min_ms"] for k in ("store_fp32", "store_fp16")}
    out["speedup_at_median"] = {k: w["baseline"]["median_ms"] / w[k]["median_ms"] for k in ("store_fp32", "store_fp16")}
    txt = json.dumps(out, indent=1, sort_keys=True)
    print(txt)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()
