"""What exact integrated gradients cost on the device (dad_attribution), each mode beside the operator that runs the
same GEMMs, and beside the route a user has without it, in the same session on the same split:

  (a) full mode (attr, frame_attr, chan_attr, utt_total) beside dad_input_grad (all three outputs, no delta): both run
      two GEMMs of the split evaluator's size (2 * 2 * frames * 256 * 768 FLOP); the attribution writes 3 KB per frame
      once and reads the rows a second time for the factor x - x', the input gradient writes 3 KB per frame twice.
  (b) frame-only mode (frame_attr, utt_total) beside dad_eval_split (student only): both run one GEMM.
  (c) the route without the feature: a 32-point midpoint sum of dad_input_grad at delta = (alpha - 1) x (zero
      baseline), the deltas, the accumulation and the final product in torch.  It is a quadrature, not the closed
      form: its error on a crossing unit is up to 1 / 64 of that unit's share.
  (d) the workspace bytes of both modes.

On tools/eval_bench.py's synthetic stores (lengths uniform in [100, 350]) at n = 1,100 and n = 5,531, fp32 and fp16
operands.  GPU time between two HIP events around enqueue-only calls.  One process measures one size: `--rounds`
alternating rounds of the legs, each leg `--warmup` untimed then `--reps` timed calls ((c): 1 and 3); a leg's figure is
the median of its round medians and its spread the range of the round medians over that figure.  No kernel trace is
taken here.

  timeout -k 10 300 python tools/attribution_bench.py --n 1100 --part out/at_n1100.json && \
  timeout -k 10 420 python tools/attribution_bench.py --n 5531 --part out/at_n5531.json && \
  python tools/attribution_bench.py --merge out/at_n1100.json out/at_n5531.json --out profiles/attribution.json
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np  # noqa: E402

from input_grad_bench import F32_MFMA_PEAK, summarise, timed  # noqa: E402

POINTS = 32
FULL = ("attr", "frame_attr", "chan_attr", "utt_total")
FRAME_ONLY = ("frame_attr", "utt_total")


def explicit_rows(E, plan):
    """The split's rows as float32 in the explicit layout [32 * slabs, 768], zeros past each length."""
    import torch
    utt = E._ig_buffers(plan)["row_utt"]
    t = torch.arange(32 * plan.slabs, device=plan.device) - 32 * plan.slab_off_d[:-1].to(torch.int64)[utt]
    lens = plan.lens_d.to(torch.int64)[utt]
    src = plan.rows_d[utt] + torch.minimum(t, (lens - 1).clamp(min=0))
    return plan.store.feats[src].to(torch.float32) * (t < lens)[:, None]


def measure(a):
    import torch
    import __graft_entry__ as entry
    from eval_bench import make_model, make_store
    if not torch.cuda.is_available():
        sys.exit("attribution_bench needs the MI355X")
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
    flop = 2 * 2 * 32 * plan.slabs * 256 * 768            # both GEMMs over the padded slabs
    res = {"n": a.n, "frames": plan.frames, "slabs": plan.slabs, "device": torch.cuda.get_device_name(dev),
           "store_bytes": int(store.feats.numel() * store.feats.element_size()),
           "attr_bytes": 4 * 768 * 32 * plan.slabs, "two_gemm_flop": flop, "midpoints": POINTS, "cases": {}}
    ev = E.enqueue_eval_split(model, plan, False, True, "fp32", ("logits", "pred"))
    dz = torch.nn.functional.one_hot(ev["pred"].to(torch.int64), 4).to(torch.float32).contiguous()
    shapes = {"attr": (32 * plan.slabs, 768), "frame_attr": (32 * plan.slabs,), "chan_attr": (plan.n, 768),
              "utt_total": (plan.n,)}
    bufs = {k: torch.empty(s, dtype=torch.float32, device=dev) for k, s in shapes.items()}
    step = torch.empty(shapes["attr"], dtype=torch.float32, device=dev)
    x = explicit_rows(E, plan)
    delta, acc = torch.empty_like(x), torch.empty_like(x)
    alphas = [(k + 0.5) / POINTS for k in range(POINTS)]
    for precision in ("fp32", "fp16"):
        prec = E._PRECISIONS[precision]

        def sampled():
            acc.zero_()
            for al in alphas:
                torch.mul(x, al - 1.0, out=delta)
                g = E.enqueue_input_grad(model, plan, dz, delta, 0.0, float("inf"), False, precision, ("grad",),
                                         _delta_out=step)["grad"]
                acc.add_(g)
            acc.mul_(x).mul_(1.0 / POINTS)

        legs = {
            "attribution_full": lambda: E.enqueue_attribution(model, plan, dz, None, False, precision, FULL, _out=bufs),
            "input_grad": lambda: E.enqueue_input_grad(model, plan, dz, None, 1.0, float("inf"), False, precision,
                                                       ("grad", "delta", "frame_l1"), _delta_out=step),
            "attribution_frame_only": lambda: E.enqueue_attribution(model, plan, dz, None, False, precision,
                                                                    FRAME_ONLY, _out=bufs),
            "split": lambda: E.enqueue_eval_split(model, plan, False, True, precision),
        }
        rounds = {name: [] for name in legs}
        rounds["sampled_32_midpoints"] = []
        for _ in range(a.rounds):
            for name, fn in legs.items():
                rounds[name].append(timed(fn, sync, a.warmup, a.reps))
            rounds["sampled_32_midpoints"].append(timed(sampled, sync, 1, 3))
        out = {name: summarise(v) for name, v in rounds.items()}
        # the quadrature's distance from the closed form, on the buffers the last calls left
        E.enqueue_attribution(model, plan, dz, None, False, precision, FULL, _out=bufs)
        sampled()
        sync()
        den = bufs["attr"].abs().sum().item()
        case = {"legs": out,
                "full_over_input_grad": out["attribution_full"]["ms"] / out["input_grad"]["ms"],
                "frame_only_over_split": out["attribution_frame_only"]["ms"] / out["split"]["ms"],
                "sampled_over_full": out["sampled_32_midpoints"]["ms"] / out["attribution_full"]["ms"],
                "full_over_frame_only": out["attribution_full"]["ms"] / out["attribution_frame_only"]["ms"],
                "full_tflops": flop / (out["attribution_full"]["ms"] * 1e-3) / 1e12,
                "sampled_l1_distance_over_l1": (acc - bufs["attr"]).abs().sum().item() / den if den > 0 else None,
                "workspace_bytes_full": E.attribution_plan(model, plan, dz, None, False, precision, FULL)["workspace_bytes"],
                "workspace_bytes_frame_only": E.attribution_plan(model, plan, dz, None, False, precision,
                                                                 FRAME_ONLY)["workspace_bytes"],
                "workspace_bytes_any_mode": int(L.lib().dad_attribution_workspace_bytes(plan.n, plan.slabs, prec)),
                "input_grad_workspace_bytes": int(L.lib().dad_input_grad_workspace_bytes(plan.n, plan.slabs, prec))}
        if precision == "fp32":
            case["full_share_of_f32_mfma_peak"] = case["full_tflops"] * 1e12 / F32_MFMA_PEAK
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
        out = {"what": "dad_attribution: (a) full mode beside dad_input_grad, (b) frame-only mode beside dad_eval_split "
                       "(student only), (c) a 32-point midpoint sum of dad_input_grad accumulated in torch, (d) the "
                       "workspace bytes; GPU ms between events, the median of alternating rounds' medians, spread = "
                       "the range of the round medians over it",
               "not_measured": "no kernel trace: the split of a call between its prologue, slab and finish launches",
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
