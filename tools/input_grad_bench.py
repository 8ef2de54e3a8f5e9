"""What the worst-case route costs on the device (dad_input_grad, FGSM, PGD), each beside the evaluator it is built
on, in the same session:

  (a) dad_input_grad (all three outputs, no delta) beside dad_eval_split (student only) on the same split.  The
      operator runs two GEMMs of the split evaluator's size (2 * 2 * frames * 256 * 768 FLOP) and writes 3 KB per
      frame twice (grad and the step): the ratio, and in fp32 the share of the exact-f32 MFMA peak (157.3 TFLOP/s)
      that the padded slabs' FLOP over its time come to.
  (b) FGSM with three epsilons (dad_eval_split, dad_input_grad writing the direction, one explicit-mode
      dad_eval_noise at four levels, and the torch plumbing between them) beside dad_eval_noise with three sigmas
      in counter mode: what the materialised direction costs to write and read back.
  (c) PGD at 10 steps for one epsilon.

On tools/eval_bench.py's synthetic stores (lengths uniform in [100, 350]) at n = 1,100 and n = 5,531, fp32 and fp16
operands.  (a) is GPU time between two HIP events around enqueue-only calls; (b) and (c) call the public functions,
which end in one copy of a result block and a synchronise, between the same two events.  One process measures one
size: `--rounds` alternating rounds of the legs, each leg `--warmup` untimed then `--reps` timed calls; a leg's figure
is the median of its round medians and its spread the range of the round medians over that figure.  No kernel trace
is taken: the per-kernel split of (b) and (c) is not measured.

  timeout -k 10 300 python tools/input_grad_bench.py --n 1100 --part out/ig_n1100.json && \
  timeout -k 10 420 python tools/input_grad_bench.py --n 5531 --part out/ig_n5531.json && \
  python tools/input_grad_bench.py --merge out/ig_n1100.json out/ig_n5531.json --out profiles/input_grad.json
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np  # noqa: E402

EPS3 = (0.01, 0.05, 0.25)
SIG3 = (0.01, 0.05, 0.25)
PGD_STEPS = 10
F32_MFMA_PEAK = 157.3e12


def timed(fn, sync, warmup, reps):
    """Median GPU ms of fn between two events."""
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
        sys.exit("input_grad_bench needs the MI355X")
    PKG = entry._pkg()
    PKG.lib()
    E, L = PKG.evaluate, PKG._lib
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    sync = lambda: torch.cuda.synchronize(dev)
    store = make_store(PKG, dev, a.n, a.seed)
    model = make_model(PKG, dev, a.seed)
    model.eval()
    plan = E.EvalPlan.of(store)
    direction_bytes = 4 * 768 * 32 * plan.slabs
    flop = 2 * 2 * 32 * plan.slabs * 256 * 768            # both GEMMs over the padded slabs
    res = {"n": a.n, "frames": plan.frames, "slabs": plan.slabs, "device": torch.cuda.get_device_name(dev),
           "store_bytes": int(store.feats.numel() * store.feats.element_size()), "direction_bytes": direction_bytes,
           "input_grad_flop": flop, "cases": {}}
    ev = E.enqueue_eval_split(model, plan, False, True, "fp32", ("logits", "pred"))
    dz = E._ce_cotangent(ev["logits"], E._adv_target(plan, ev["pred"], "label"))
    grad = torch.empty((32 * plan.slabs, 768), dtype=torch.float32, device=dev)
    for precision in ("fp32", "fp16"):
        prec = E._PRECISIONS[precision]
        bufs = {}

        def input_grad():
            bufs.update(E.enqueue_input_grad(model, plan, dz, None, 1.0, float("inf"), False, precision,
                                             ("grad", "delta", "frame_l1"), _delta_out=grad))

        legs = {
            "input_grad": input_grad,
            "split": lambda: E.enqueue_eval_split(model, plan, False, True, precision),
            "fgsm_3eps": lambda: E.evaluate_adversarial_store(model, plan, EPS3, precision=precision),
            "noise_3sigma_counter": lambda: E.evaluate_noise_store(model, plan, (0.0,) + SIG3, seed=a.seed,
                                                                   precision=precision),
        }
        rounds = {name: [] for name in legs}
        rounds["pgd_10steps"] = []
        for _ in range(a.rounds):
            for name, fn in legs.items():
                rounds[name].append(timed(fn, sync, a.warmup, a.reps))
            rounds["pgd_10steps"].append(timed(
                lambda: E.evaluate_adversarial_store(model, plan, EPS3[1:2], steps=PGD_STEPS, precision=precision),
                sync, 1, 3))
            bufs.clear()
            torch.cuda.empty_cache()
        out = {name: summarise(v) for name, v in rounds.items()}
        case = {"legs": out,
                "input_grad_over_split": out["input_grad"]["ms"] / out["split"]["ms"],
                "fgsm_over_noise": out["fgsm_3eps"]["ms"] / out["noise_3sigma_counter"]["ms"],
                "pgd_ms_per_step": out["pgd_10steps"]["ms"] / PGD_STEPS,
                "input_grad_tflops": flop / (out["input_grad"]["ms"] * 1e-3) / 1e12,
                "input_grad_bytes_written": 2 * direction_bytes + 4 * 32 * plan.slabs,
                "workspace_bytes": int(L.lib().dad_input_grad_workspace_bytes(plan.n, plan.slabs, prec))}
        if precision == "fp32":
            case["input_grad_share_of_f32_mfma_peak"] = case["input_grad_tflops"] * 1e12 / F32_MFMA_PEAK
        res["cases"][precision] = case
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--n", type=int, default=1100)
    ap.add_argument("--reps", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--seed", type=int, default=5)
    ap.add_argument("--part", default=None, help="write this size's measurements here")
    ap.add_argument("--merge", nargs="+", default=None, help="parts to merge into --out")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.merge:
        parts = [json.load(open(p)) for p in a.merge]
        out = {"what": "dad_input_grad beside dad_eval_split, FGSM with three epsilons beside dad_eval_noise with three "
                       "sigmas in counter mode, PGD at 10 steps; GPU ms between events, the median of alternating "
                       "rounds' medians, spread = the range of the round medians over it",
               "not_measured": "no kernel trace: the per-kernel split of the FGSM and PGD legs, and the time of the "
                               "torch plumbing inside them",
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
