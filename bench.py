#!/usr/bin/env python3
"""DAD train-step throughput on MI355X (BASELINE.json metric).

One "step" = the full fused DAD step on one clean + one noisy batch per GPU:
3 encoder passes (student-clean, teacher-weak, student-strong) with in-kernel weak/strong
augmentation, CE + masked KL + class-aware ECDA/MMD, DACP mask, analytic backward,
global-norm clip + Adam + teacher EMA (+ one RCCL all-reduce of the grads for N > 1).
Post-warm-up epoch 60 (full loss weights) with a confident synthetic teacher, so the KL and
ECDA terms are active.  Inputs are resident in HBM before timing.
Order of a run: ~50 ms of untimed headline steps to settle the clocks (--settle-ms, `settle_steps` in
the line), the W warm-up steps, the K timed steps, then (--dump-outputs DIR) the last timed step's
outputs written as DIR/<name>.npy, and the result line.  With --full the run goes on after the timed
steps: a per-kernel pass, the parity block, then the side legs (FP32 / BF16 modes, random labels,
data path) and the CPU baseline, all reported in the same line.

    python bench.py [--gpus N --steps K --warmup W --precision fp16|bf16|fp32] [--dump-outputs DIR] [--full]
    torchrun --nproc-per-node N bench.py --gpus N ...          (one process per GPU)

Prints ONE JSON line (rank 0).
"""
import argparse
import importlib
import json
import math
import os
import statistics
import subprocess
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
PKG = importlib.import_module(
    "robust-speech-emotion-recognition-via-dynamic-asymmetric-distillation-in-noisy-environments_amd")

METRIC = "utterances/sec (DAD train step) batch=64 at 1/2/4/8 MI355X; loss parity"
HBM_PEAK_GBS = 8000.0          # MI355X HBM3E spec (MI355X_MICROARCH.md)
BF16_PEAK_TFLOPS = 2500.0      # dense bf16 / fp16 MFMA (the same rate for both)
PEAK_TFLOPS = {"fp16": BF16_PEAK_TFLOPS, "bf16": BF16_PEAK_TFLOPS}
FP32_PEAK_TFLOPS = 157.3       # f32 MFMA == f32 vector rate
# every 8th timed step (every steps/2-th in short runs) records hip events (DAD_BENCH_EVENT_EVERY
# overrides, for measuring what the events themselves cost)
EVENT_EVERY = int(os.environ.get("DAD_BENCH_EVENT_EVERY", "8"))
                               # at its kernel boundaries (dad_timing_start): per-kernel durations, live
CPU_BASELINE_SECONDS = 15.0    # bounded CPU sample (PyTorch-CPU steps until this much time)
N_BATCHES = 8                  # distinct resident batches cycled by the timed steps: 8 x 118 MB of f32
                               # features, past the 256 MB infinity cache, so encoder reads come from HBM
PMC_SUMMARY = os.path.join(ROOT, "profiles", "pmc_latest.json")   # tools/profile_report.py --json
MFMA_TARGET = 0.40             # north_star: >= 40 % MFMA utilisation on the encoder linears


def init_model_weights(model, seed, margin=5.0):
    """nn.Linear-range W1/b1 and a classifier aligned with class prototypes (confident teacher)."""
    g = torch.Generator().manual_seed(seed)
    P = torch.randn(4, 768, generator=g, dtype=torch.float64) * 2.0
    k1 = 1.0 / math.sqrt(768)
    W1 = (torch.rand(256, 768, generator=g, dtype=torch.float64) * 2 - 1) * k1
    b1 = (torch.rand(256, generator=g, dtype=torch.float64) * 2 - 1) * k1
    mu = torch.relu(P @ W1.T + b1)
    dirs = mu - mu.mean(0, keepdim=True)
    dirs = dirs / dirs.norm(dim=1, keepdim=True)
    proj = mu @ dirs.T
    gap = float(np.mean([float(proj[c, c] - torch.cat([proj[c, :c], proj[c, c + 1:]]).max()) for c in range(4)]))
    W2 = dirs * (margin / gap)
    b2 = torch.zeros(4, dtype=torch.float64)
    flat = torch.cat([W1.reshape(-1), b1, W2.reshape(-1), b2]).float()
    with torch.no_grad():
        model.student_flat.copy_(flat)
        model.teacher_flat.copy_(flat)
    return P.float()


def make_batches(P, n, B, T, seed, device, snr_db=5.0, random_labels=False):
    """n (clean, noisy) batch pairs, all frames valid (BASELINE.md §3 inputs).  Labels: B/4 of each
    class (the default), or drawn uniformly (random_labels: class sizes as a random batch from a
    balanced corpus has them)."""
    g = torch.Generator(device=device).manual_seed(seed)
    Pd = P.to(device)
    out = []
    for i in range(n):
        if random_labels:
            yc = torch.randint(0, 4, (B,), generator=g, device=device)
        else:
            yc = (torch.arange(B, device=device) + i) % 4
        yn = (yc + 1) % 4
        xc = Pd[yc][:, None, :] + 0.5 * torch.randn(B, T, 768, generator=g, device=device)
        sig = (0.5 + 10 ** (-snr_db / 20)) * (0.5 + 2.0 * torch.rand(B, 1, 1, generator=g, device=device))
        xn = Pd[yn][:, None, :] + sig * torch.randn(B, T, 768, generator=g, device=device)
        pad = torch.zeros(B, T, dtype=torch.bool, device=device)
        out.append(({"net_input": {"feats": xc.contiguous(), "padding_mask": pad}, "labels": yc},
                    {"net_input": {"feats": xn.contiguous(), "padding_mask": pad}, "labels": yn}))
    return out


def lib_sha16():
    """sha256 (16 hex) of the loaded libdad_hip.so: ties PMC summaries to the code they measured."""
    import hashlib
    try:
        return hashlib.sha256(open(PKG._build.lib_path(os.environ.get("DAD_LIB_VARIANT") or None), "rb").read()
                              ).hexdigest()[:16]
    except OSError:
        return None


def pmc_counters(kernel):
    """Per-launch PMC values of `kernel` from the committed summary (tools/profile_report.py): HBM
    bytes (2 x FETCH_SIZE + WRITE_SIZE, MI355X_MICROARCH.md's gfx950 correction) and the matrix
    pipe's busy cycles.  The summary records the library hash it was measured with; `stale` is
    True when that is not the library loaded now (the counters then describe other code)."""
    try:
        d = json.load(open(PMC_SUMMARY))
    except Exception:
        return None
    k = d.get("kernels", {}).get(kernel)
    if k is None:
        return None
    out = dict(k)
    out["source"] = d.get("source", PMC_SUMMARY)
    out["lib_sha16"] = d.get("lib_sha16")
    out["stale"] = d.get("lib_sha16") != lib_sha16()
    return out


def pmc_summary_kernels():
    try:
        return set(json.load(open(PMC_SUMMARY)).get("kernels", {}))
    except Exception:
        return None


def _cpu_model():
    try:
        for line in open("/proc/cpuinfo"):
            if line.startswith("model name"):
                return line.split(":", 1)[1].strip()
    except OSError:
        pass
    return None


def _cpu_leg(B, T, steps, epoch, threads, seconds):
    """PyTorch-CPU steps (oracle/torch_cpu.py) with torch's intra-op pool at `threads`: 2 warm-ups,
    then steps until `seconds` of timed steps, at least `steps` of them unless the leg's wall
    time (warm-ups included) passes 2 x `seconds` (an oversubscribed pool: a 256-thread pool on a
    16-CPU job share ran 17 s per step); median seconds per step."""
    from oracle import dad_oracle, synth, torch_cpu
    prev = torch.get_num_threads()
    torch.set_num_threads(threads)
    try:
        cfg = dad_oracle.make_cfg("iemocap")
        W1, b1, W2, b2, _ = synth.init_weights(0)
        st = torch_cpu.TorchCPUStep(W1, b1, W2, b2, cfg)
        times = []
        k = 0
        while (k < steps + 2 and sum(times) < 2 * seconds) or (sum(times[2:]) < seconds and k < 200) or k < 3:
            inp = synth.make_step_inputs(0, k, B, T, ragged=False)
            t0 = time.perf_counter()
            st.step(inp, epoch)
            times.append(time.perf_counter() - t0)
            k += 1
    finally:
        torch.set_num_threads(prev)
    return statistics.median(times[2:]), len(times) - 2, sum(times[2:])


def job_cpus():
    """CPUs this job may use: the affinity mask, capped by the cgroup CPU quota (cgroup v2
    cpu.max / v1 cfs_quota_us).  On the GPU box the affinity mask lists all of the host's CPUs
    while the job's share is a fraction of them (a 256-thread pool on a 16-CPU share ran one
    step in 17 s, round 3)."""
    n = len(os.sched_getaffinity(0))
    quota = None
    try:
        q, p = open("/sys/fs/cgroup/cpu.max").read().split()[:2]
        if q != "max":
            quota = float(q) / float(p)
    except (OSError, ValueError):
        try:
            q = float(open("/sys/fs/cgroup/cpu/cpu.cfs_quota_us").read())
            p = float(open("/sys/fs/cgroup/cpu/cpu.cfs_period_us").read())
            if q > 0:
                quota = q / p
        except (OSError, ValueError):
            pass
    if quota is not None:
        n = max(1, min(n, int(quota)))
    return n


def cpu_baseline(B, T, steps, epoch, seconds=CPU_BASELINE_SECONDS):
    """The PyTorch-CPU step (oracle/torch_cpu.py: the reference's step on the same ATen ops,
    calibrated against the imported reference in profiles/r02_cpu_calibration.json) on this
    host with the job's CPU share: OMP_NUM_THREADS (16 on the GPU box) and, when it differs, the
    CPUs the job may use (affinity mask capped by the cgroup quota, job_cpus()).  Each leg runs
    2 warm-ups then at least `steps` timed steps; `value` is the faster leg."""
    usable = job_cpus()
    job = min(int(os.environ.get("OMP_NUM_THREADS") or usable), usable)
    legs = []
    threads = sorted({job, usable})
    for n in threads:
        med, k, tot = _cpu_leg(B, T, steps, epoch, n, seconds / len(threads))
        legs.append({"threads": n, "value": B / med, "median_s_per_step": med, "steps": k, "seconds": tot})
    best = max(legs, key=lambda r: r["value"])
    out = {"value": best["value"], "unit": "utterances/s", "cores": best["threads"], "kind": "port",
           "host_cpus": os.cpu_count(), "usable_cpus": usable, "job_threads": job, "cpu_model": _cpu_model(),
           "legs": legs,
           "sample": "PyTorch-CPU DAD step (oracle/torch_cpu.py), B=%d T=%d epoch %d, torch RNG, timed at %s threads "
                     "(>= %d steps after 2 warm-ups, about %.0f s in all); value = the faster leg"
                     % (B, T, epoch, " and ".join(str(r["threads"]) for r in legs), steps, seconds)}
    # port/reference ratio measured in the container (profiles/r02_cpu_calibration.json) at the
    # thread counts it has; applied only inside that range (never extrapolated to more threads)
    try:
        cal = json.load(open(os.path.join(ROOT, "profiles", "r02_cpu_calibration.json")))
        rows = {int(k): v["ratio_port_over_reference"] for k, v in cal["by_threads"].items()}
        n = best["threads"]
        inside = min(rows) <= n <= max(rows)
        out["calibration"] = {"ratio_port_over_reference_by_threads": rows, "container_cpu": cal.get("cpu_model"),
                              "source": "profiles/r02_cpu_calibration.json", "applies": inside,
                              "reference_equivalent_value": out["value"] * rows[min(rows, key=lambda k: abs(k - n))]
                              if inside else None,
                              "note": None if inside else "measured at %s threads only; %d threads is outside that "
                              "range, so no reference-equivalent value is derived" % (sorted(rows), n)}
    except Exception:
        out["calibration"] = None
    return out


def synthetic_store(P, n_utt, T, dev, seed, noisy, snr_db=5.0):
    """FeatureStore of n_utt full-length utterances drawn as make_batches draws its rows (label
    y = i mod 4; clean: P[y] + 0.5 N, noisy: P[(y+1) mod 4] + sig N with make_batches' per-utterance
    sig), so steps fed from it see the headline's data: the ECDA member sets, and with them the tail
    launch's time, depend on the features (pure N(0, 1) features made the tail launch 8 us longer)."""
    g = torch.Generator(device=dev).manual_seed(seed)
    Pd = P.to(dev)
    y = torch.arange(n_utt, device=dev) % 4
    feats = torch.empty(n_utt * T, 768, device=dev)
    for i0 in range(0, n_utt, 64):
        i1 = min(n_utt, i0 + 64)
        yy = y[i0:i1]
        if noisy:
            sig = (0.5 + 10 ** (-snr_db / 20)) * (0.5 + 2.0 * torch.rand(i1 - i0, 1, 1, generator=g, device=dev))
            x = Pd[(yy + 1) % 4][:, None, :] + sig * torch.randn(i1 - i0, T, 768, generator=g, device=dev)
        else:
            x = Pd[yy][:, None, :] + 0.5 * torch.randn(i1 - i0, T, 768, generator=g, device=dev)
        feats[i0 * T:i1 * T] = x.reshape(-1, 768)
    return PKG.data.FeatureStore(feats, np.full(n_utt, T, np.int64), np.arange(n_utt, dtype=np.int64) * T,
                                 np.arange(n_utt, dtype=np.int64) % 4, device=dev)


def data_path_bench(step, B, T, epoch, dev, P, n_utt=1024, reps=40, steps=20):
    """The device-resident data path (csrc/collate.hip): dad_collate of
    a [B, T] batch from a FeatureStore of n_utt full-length utterances (n_utt*T*3 KB in HBM,
    well past the caches), timed with HIP events on the launch stream; then the train step fed
    by DeviceLoaders over a clean and a noisy store of the headline's synthetic distribution
    (synthetic_store; clean + noisy collated every step, inside the clock)."""
    store = synthetic_store(P, n_utt, T, dev, seed=3, noisy=False)
    nstore = synthetic_store(P, n_utt, T, dev, seed=4, noisy=True)
    idx = [np.random.RandomState(k).choice(n_utt, B, replace=False) for k in range(reps)]
    idx_d = [torch.from_numpy(i).to(dev) for i in idx]
    for k in range(3):
        store.collate(idx[k], index_d=idx_d[k], T=T)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for k in range(reps):
        store.collate(idx[k], index_d=idx_d[k], T=T)
    e1.record()
    torch.cuda.synchronize()
    ms = e0.elapsed_time(e1) / reps
    nbytes = B * T * 768 * 4 * 2 + B * T + B * 16       # rows read + rows written + mask + labels
    def epochs(loader):      # a new epoch (a new shuffle) whenever one runs out, as a trainer's epoch loop does
        while True:
            yield from loader

    def fed(fused):
        # the step with both batches drawn from device loaders inside the timed region:
        # collated (dad_collate copies [B, T, 768]) or fused (store mode: the encoder gathers)
        clean = PKG.data.DeviceLoader(store, batch_size=B, shuffle=True, fused=fused)
        noisy = PKG.data.DeviceLoader(nstore.subset(np.arange(n_utt), with_labels=False), batch_size=B,
                                      shuffle=True, fused=fused)
        ci, ni = epochs(clean), epochs(noisy)
        # batches drawn one ahead, each step naming the next (checkpoint.train_epoch's loop): the
        # 16-bit modes prepare the next batch's rows inside the tail launch
        nxt = [(next(ci), next(ni))]

        def one():
            cur, nxt[0] = nxt[0], (next(ci), next(ni))
            step.step(cur[0], cur[1], epoch, next_batch=nxt[0])
        for _ in range(3):
            one()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            one()
        torch.cuda.synchronize()
        dt = (time.perf_counter() - t0) / steps
        return {"value": B / dt, "unit": "utterances/s", "ms_per_step": dt * 1e3, "steps": steps}

    collated, fused = fed(False), fed(True)
    collated["note"] = "clean + noisy batch collated (copied) per step"
    fused["note"] = "store mode: rows gathered by the encoder's LDS-DMA, no padded copy"
    return {"kernel": "dad_collate_kernel", "store": "two stores (clean, noisy) of %d utterances x %d frames x 768 f32 "
            "(%.2f GB each) resident in HBM, the headline batches' synthetic distribution" % (n_utt, T, n_utt * T * 3072 / 1e9),
            "collate_ms": ms, "algorithmic_bytes_per_launch": nbytes,
            "achieved_gbs": nbytes / (ms * 1e-3) / 1e9, "peak_gbs": HBM_PEAK_GBS,
            "frac": nbytes / (ms * 1e-3) / 1e9 / HBM_PEAK_GBS,
            "step_with_device_collate": collated, "step_with_store_gather": fused}


# ------------------------------------------------------------------ BASELINE configs[4]: mixed corpora
CORPORA = {   # synthetic stand-ins with each corpus's utterance count and fold structure
    "iemocap": {"sessions": [1085, 1023, 1151, 1031, 1241]},           # I/config.py:36, 5 session folds
    "casia": {"speakers": ["spk_%d" % k for k in range(4)], "n": 5996},  # 4 speaker folds
    "emodb": {"n": 535},                                                 # 10 speakers, LOSO folds
}


def _synthetic_store(P, labels, sizes, sigma, dev, gen):
    """FeatureStore of utterances x[t] = P[y] + sigma_u * N(0, 1), all on the device."""
    sizes = np.asarray(sizes, np.int64)
    offsets = np.concatenate([[0], np.cumsum(sizes)[:-1]]).astype(np.int64)
    n_rows = int(sizes.sum())
    feats = torch.empty(n_rows, 768, device=dev)
    row_utt = torch.repeat_interleave(torch.arange(len(sizes), device=dev), torch.from_numpy(sizes).to(dev))
    lab_d = torch.from_numpy(np.asarray(labels, np.int64)).to(dev)
    sig_d = torch.as_tensor(sigma, dtype=torch.float32, device=dev).reshape(-1).expand(len(sizes))
    chunk = 1 << 18
    for r0 in range(0, n_rows, chunk):
        u = row_utt[r0:r0 + chunk]
        feats[r0:r0 + len(u)] = P[lab_d[u]] + sig_d[u, None] * torch.randn(len(u), 768, device=dev, generator=gen)
    st = PKG.data.FeatureStore.__new__(PKG.data.FeatureStore)
    st.feats = feats
    st._init_index(dev, sizes, offsets, labels)
    return st


def mixed_corpora(P, dev, seed, snr_db, t_min=100, t_max=300):
    """Clean and noisy unions of synthetic IEMOCAP + CASIA + EMODB stores (fused-loader ready),
    with the per-corpus fold metadata: returns (clean, noisy, starts, meta)."""
    rs = np.random.RandomState(seed)
    gen = torch.Generator(device=dev)
    gen.manual_seed(seed)
    Pd = P.to(dev)
    cleans, noisys, meta = [], [], {}
    for name in ("iemocap", "casia", "emodb"):
        c = CORPORA[name]
        if name == "iemocap":
            sess = np.concatenate([np.full(n, k + 1) for k, n in enumerate(c["sessions"])])
            n = len(sess)
            meta[name] = sess
        elif name == "casia":
            n = c["n"]
            meta[name] = np.array(c["speakers"])[np.arange(n) % 4]
        else:
            n = c["n"]
            meta[name] = np.array(["emodb_spk_" + s for s in PKG.data.EMODB_SPEAKERS])[np.arange(n) % 10]
        labels = rs.permutation(np.arange(n) % 4)
        sizes = rs.randint(t_min, t_max + 1, size=n)
        sig_n = (0.5 + 10 ** (-snr_db / 20)) * rs.uniform(0.5, 2.5, size=n)
        cleans.append(_synthetic_store(Pd, labels, sizes, np.full(n, 0.5), dev, gen))
        noisys.append(_synthetic_store(Pd, labels, sizes, sig_n, dev, gen))
    clean, starts = PKG.data.FeatureStore.concat(cleans)
    noisy, _ = PKG.data.FeatureStore.concat(noisys)
    del cleans, noisys
    return clean, noisy, starts, meta


def mixed_fold_train(starts, meta, k):
    """Fold k of the K-fold sweep: the union of IEMOCAP session fold (k mod 5) + 1, CASIA speaker
    fold k mod 4 and EMODB speaker fold k mod 10 training utterances (data.py fold rules)."""
    d = PKG.data
    tr = [d.iemocap_fold_split(meta["iemocap"], k % 5 + 1)[0], d.casia_fold_split(meta["casia"], k % 4)[0],
          d.emodb_fold_split(meta["emodb"], k % 10)[0]]
    return np.concatenate([s + t for s, t in zip(starts, tr)])


def run_mixed(args, model, dev, rank, world, dist, comm, after_timed=None):
    """BASELINE configs[4]: mixed IEMOCAP+CASIA+EMODB batches, K-fold throughput sweep.  Every
    step's clean and noisy batches mix utterances of the three corpora (fused store-mode
    loaders over the unions of the fold's training splits, variable lengths); the DAD config
    rotates over the three flavours per batch.  One timed segment per fold."""
    P = init_model_weights(model, seed=0)
    clean, noisy, starts, meta = mixed_corpora(P, dev, seed=23, snr_db=args.snr)
    views = [PKG.ConfigView(None, flavor="iemocap"), PKG.ConfigView(None, flavor="casia", USE_DACP=True, USE_ECDA=True),
             PKG.ConfigView(None, flavor="emodb")]
    step = PKG.DADStep(model, views[0], precision=args.precision, rng="counter", seed=1000 + rank, comm=comm)
    B = args.batch

    def batches(store, labeled, seed):
        g = torch.Generator()
        g.manual_seed(seed)
        while True:
            yield from PKG.data.DeviceLoader(store, batch_size=B, shuffle=True, generator=g, fused=True,
                                             with_labels=labeled)

    folds, ktimes = [], []
    n = 0
    for k in range(args.folds):
        tr = mixed_fold_train(starts, meta, k)
        ci = batches(clean.subset(tr), True, 1000 * k + rank)
        ni = batches(noisy.subset(tr, with_labels=False), False, 1000 * k + 500 + rank)

        def run(nsteps, timed):
            rows = 0
            utts = 0
            nonlocal n
            for i in range(nsteps):
                c, nb = next(ci), next(ni)
                step.view = views[n % 3]
                n += 1
                if timed:
                    for b in (c, nb):
                        f = b["net_input"]["feats"]
                        rows += int(f.store.sizes[f.index].sum())
                    utts += c["net_input"]["feats"].shape[0]
                step.step(c, nb, args.epoch)
            return rows, utts
        run(args.warmup if k == 0 else 3, False)
        torch.cuda.synchronize()
        timer = PKG._lib.KernelTimer(event_every(args.steps), args.steps // event_every(args.steps) + 1,
                                     kernels=TIMED_KERNELS)
        if dist:
            dist.barrier()
        t0 = time.perf_counter()
        rows, utts = run(args.steps, True)
        torch.cuda.synchronize()
        if dist:
            dist.barrier()
        el = time.perf_counter() - t0
        ktimes.append(timer.stop())
        if dist:
            t = torch.tensor([el], dtype=torch.float64)
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
            el = float(t.item())
            u = torch.tensor([utts], dtype=torch.float64)
            dist.all_reduce(u)
            utts = int(u.item())
        folds.append({"fold": k, "train_utterances": int(len(tr)), "seconds": el, "utterances": utts,
                      "value": utts / el, "avg_valid_frames_per_step": rows / args.steps})
    if after_timed is not None:
        after_timed(step)
    table = kernel_pass(lambda: run(1, False), args.kernel_steps) if args.full else {}
    return step, folds, merge_ktimes(ktimes), table


def event_every(steps):
    # (a 20-step region records 2 steps, not 4: each recorded step puts its events on the stream)
    return max(1, min(EVENT_EVERY, steps // 2))


# The timed region records events around one kernel only (the roofline kernel, timed_kernels):
# with the default system-scope fence every recorded event had cost the stream ~3 us (events at
# every boundary of every 8th step put 3.2 us on the mean step); the library's timing events are
# now created without that fence (hipEventDisableSystemFence), and the per-kernel table still
# comes from a separate pass after the timed region.
TIMED_KERNELS = ["encode"]


def timed_kernels(precision, ahead):
    """The kernels the timed region records events around: with next-batch preparation (16-bit)
    the three long launches (encoder; tail launch with the noisy-row preparation; weight gradient
    with the clean-row conversion, the longest), else the encoder.  The other kernels' times come
    from the separate eager pass after the timed region."""
    return ["wgrad", "tail", "encode"] if precision != "fp32" and ahead else TIMED_KERNELS


def capture_steps(step, data, epoch, split=None, ahead=False):
    """One hipGraph (torch.cuda.CUDAGraph) per resident batch pair, each holding one full fused
    step (the C ABI is enqueue-only; tests/test_gpu_graph.py proves replay == eager bit for bit).
    A graph bakes its step's host scalars into the kernel arguments: the RNG step counter and the
    Adam bias corrections of steps g0 .. g0+7, so replay k runs graph k mod 8 -- a full step on
    batch k mod 8 with that graph's noise stream and Adam step, reading and updating the live
    device state (parameters, moments, DACP).  Batch `split` is captured as two graphs, the
    encoder launch and the rest of its step, so stream events recorded between their replays
    time the encoder inside the timed region (HIP event nodes captured INSIDE a graph do not
    report elapsed times).
    ahead (16-bit): every graph also prepares the next graph's rows in its tail launch, the last
    one for the first graph's counter (next_counter), and one eager step on the last batch first
    prepares the first graph's rows -- so the cycle of replays is the eager prepared-ahead chain
    with its counters repeating.  Returns a list of graph tuples, or raises on a capture error."""
    torch.cuda.synchronize()
    n = len(data)
    if ahead:
        c, nb = data[-1]
        step.step(c, nb, epoch, next_batch=data[0])
        torch.cuda.synchronize()
    g0 = step.global_step
    graphs = []
    for i, (c, nb) in enumerate(data):
        kw = {}
        if ahead:
            kw = {"next_batch": data[(i + 1) % n], "next_counter": g0 if i == n - 1 else None}
        if i != split:
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                step.step(c, nb, epoch, **kw)
            if ahead and not step.last_prepped:
                raise RuntimeError("graph %d was captured without its prepared rows" % i)
            graphs.append((g,))
            continue
        ga, gb = torch.cuda.CUDAGraph(), torch.cuda.CUDAGraph()

        def cut():
            ga.capture_end()
            gb.capture_begin(pool=ga.pool())
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            ga.capture_begin()
            step.step(c, nb, epoch, after_encode=cut, **kw)
            gb.capture_end()
        torch.cuda.current_stream().wait_stream(s)
        if ahead and not step.last_prepped:
            raise RuntimeError("graph %d was captured without its prepared rows" % i)
        graphs.append((ga, gb))
    torch.cuda.synchronize()
    return graphs


def kernel_pass(run1, n):
    """Per-kernel durations (all boundaries, every 2nd step) over n steps run after the timed
    region: the `kernels` table of the line (the encoder's own entry is the timed region's)."""
    if n <= 0:
        return {}
    timer = PKG._lib.KernelTimer(2, n // 2 + 1)
    for _ in range(n):
        run1()
    torch.cuda.synchronize()
    return timer.stop()


def merge_ktimes(parts):
    """Weighted mean of several KernelTimer.stop() results."""
    acc = {}
    for p in parts:
        for k, (m, n) in p.items():
            t, c = acc.get(k, (0.0, 0))
            acc[k] = (t + m * n, c + n)
    return {k: (t / c, c) for k, (t, c) in acc.items() if c}


ENC_KERNEL = {"fp16": "dad_encode_wp_f16", "bf16": "dad_encode_wp", "fp32": "dad_encode_f32"}
WGRAD_KERNEL = {"fp16": ("wgrad", "dad_wgrad_direct_f16"), "bf16": ("wgrad", "dad_wgrad_direct"),
                "fp32": ("wgrad", "dad_wgrad_f32")}
KNAMES = {p: {"encode": ENC_KERNEL[p], "pool": "dad_pool", "wgrad": WGRAD_KERNEL[p][1],
              "reduce": "dad_reduce" if p == "fp32" else "dad_reduce_w", "optim": "dad_optim"}
          for p in ("fp16", "bf16", "fp32")}


def class_aware(view):
    """config.py's class_aware switch: USE_CLASS_AWARE_MMD on IEMOCAP, always on for CASIA / EMODB."""
    return view.flavor != "iemocap" or bool(getattr(view, "USE_CLASS_AWARE_MMD", True))


def tail_kernel(B, Bn, class_aware=True):
    """The launch in the "tail" slot (dad_abi.hip): the wave-centric dad_tail_ecda_w for batches of
    at most 64 per side with class-aware MMD (unless DAD_TAIL_W=0), else dad_tail_ecda."""
    w = B <= 64 and Bn <= 64 and class_aware and os.environ.get("DAD_TAIL_W", "1") != "0"
    return "dad_tail_ecda_w" if w else "dad_tail_ecda"


def _roof(kernel, ms, bytes_, flops, peak_tf, bound=None, note=None, bytes_moved=None):
    """One kernel's roofline block: algorithmic bytes (or FLOPs) per launch / mean launch time.
    bytes_moved: what the launch's design reads and writes when that is more than the algorithmic
    bytes (reported beside them, never in `frac`)."""
    ridge = peak_tf * 1e12 / (HBM_PEAK_GBS * 1e9)
    intensity = flops / bytes_ if bytes_ else float("inf")
    bound = bound or ("mfma" if intensity > ridge else "hbm")
    if bound == "hbm":
        achieved, peak, unit = bytes_ / (ms * 1e-3) / 1e9, HBM_PEAK_GBS, "GB/s"
    else:
        achieved, peak, unit = flops / (ms * 1e-3) / 1e12, peak_tf, "TFLOP/s"
    pmc = pmc_counters(kernel)
    r = {"bound": bound, "kernel": kernel, "achieved": achieved, "peak": peak, "unit": unit, "frac": achieved / peak,
         "traffic": pmc["hbm_bytes_per_launch"] if pmc and "hbm_bytes_per_launch" in pmc else None,
         "avg_launch_ms": ms, "algorithmic_bytes_per_launch": bytes_, "algorithmic_flops_per_launch": flops,
         "arithmetic_intensity_flop_per_byte": intensity, "ridge_flop_per_byte": ridge,
         "traffic_source": None if pmc is None else pmc["source"],
         "traffic_stale": None if pmc is None else pmc["stale"]}
    if bytes_moved is not None:
        r["bytes_moved_per_launch"] = bytes_moved
        r["bytes_moved_rate_gbs"] = bytes_moved / (ms * 1e-3) / 1e9
    if note:
        r["note"] = note
    return r


def step_traffic(names):
    """PMC HBM bytes per step summed over the step's kernels (one launch each), from the committed
    summary: the whole step's fabric traffic against the survey's compulsory bytes."""
    tot, parts, stale = 0.0, {}, False
    for n in names:
        pk = pmc_counters(n)
        if not pk or "hbm_bytes_per_launch" not in pk:
            return None
        parts[n] = pk["hbm_bytes_per_launch"]
        tot += pk["hbm_bytes_per_launch"]
        stale = stale or bool(pk["stale"])
    return {"bytes": tot, "per_kernel": parts, "stale": stale}


def rooflines(ktimes, rows_c, rows_n, ms_step, precision, tail_name="dad_tail_ecda_w", prepped_ahead=False):
    """`roofline` of the dominant launch, the encoder's own roofline, `step_roofline` of the whole
    step and the per-kernel table (live HIP-event durations of dad_timing_start) with MFMA
    utilisation of the encoder linears.  Algorithmic work:
      FP32 encoder: bytes = (rows_c + rows_n) x 768 x 4 (both fp32 feature tensors, read once);
      16-bit encoder (dad_encode_wp): bytes = (rows_c + 2 rows_n) x 768 x 2 (its prepared rows);
        flops = 2 x 768 x 256 x (rows_c + 2 rows_n) (student-clean, teacher-weak, student-strong)
      row preparation (16-bit, in the tail launch when the next batch is prepared ahead):
        bytes = (rows_c + rows_n) x 768 x 4 read + (rows_c + 2 rows_n) x 768 x 2 written
      dW1:      flops = 2 x 768 x 256 x (rows_c + rows_n)
      step:     t_roof = max(F / P_mfma, Q / BW) with F = 2 x 768 x 256 x (2 rows_c + 3 rows_n) and
                Q = the fp32 features read once.
    bound: the kernel's arithmetic intensity against the ridge point P_mfma / BW."""
    peak_tf = PEAK_TFLOPS.get(precision, FP32_PEAK_TFLOPS)
    h16 = precision != "fp32"
    src_bytes = int((rows_c + rows_n) * 768 * 4)
    prep_bytes = int((rows_c + 2 * rows_n) * 768 * 2)
    enc_bytes = prep_bytes if h16 else src_bytes
    enc_flops = 2 * 768 * 256 * (rows_c + 2 * rows_n)
    wg_flops = 2 * 768 * 256 * (rows_c + rows_n)
    step_flops = 2 * 768 * 256 * (2 * rows_c + 3 * rows_n)
    names = dict(KNAMES[precision], tail=tail_name)
    if h16 and prepped_ahead:   # the weight gradient that also converts the next batch's clean rows
        names["wgrad"] = WGRAD_KERNEL[precision][1] + "_cp"
    kern = {}
    for k, (m, n) in sorted(ktimes.items()):
        kern[names.get(k, k)] = {"avg_ms": m, "timed_launches": n}
    if "encode" not in ktimes:
        return None, None, kern
    enc = ktimes["encode"][0]
    wkey, wname = "wgrad", names["wgrad"]
    wg = ktimes.get(wkey, (float("nan"), 0))[0]
    ekn = ENC_KERNEL[precision]
    enc_rf = _roof(ekn, enc, enc_bytes, enc_flops, peak_tf)
    enc_rf["timed_launches"] = ktimes["encode"][1]
    launch_rf = {"encode": enc_rf}
    if h16 and prepped_ahead:
        # the next batch's preparation rides in two launches (padded batches): the tail launch
        # prepares its noisy rows, the weight gradient converts its clean rows
        nsrc, csrc = int(rows_n * 768 * 4), int(rows_c * 768 * 4)
        if "tail" in ktimes:
            launch_rf["tail"] = _roof(
                tail_name, ktimes["tail"][0], nsrc, 0.0, peak_tf, bound="hbm",
                bytes_moved=nsrc + int(2 * rows_n * 768 * 2),
                note="pooling, tail + ECDA blocks and the next batch's noisy-row preparation in one launch; "
                     "algorithmic bytes (SURVEY.md §8(d)) = the noisy fp32 features read once; bytes_moved adds "
                     "their strong and weak 16-bit rows written")
            launch_rf["tail"]["timed_launches"] = ktimes["tail"][1]
        if wkey in ktimes:
            launch_rf["wgrad"] = _roof(
                wname, wg, csrc, wg_flops, peak_tf,
                bytes_moved=int((rows_c + rows_n) * 768 * 2) + csrc + int(rows_c * 768 * 2),
                note="dW1 split-K GEMM and the next batch's clean-row conversion in one launch; algorithmic "
                     "work = dW1's FLOPs and the clean fp32 features read once; bytes_moved adds the prepared "
                     "clean + strong rows the GEMM reads and the clean 16-bit rows written (not the split-K "
                     "partials)")
            launch_rf["wgrad"]["timed_launches"] = ktimes[wkey][1]
    # `roofline`: the launch that takes longest
    dom = max(launch_rf, key=lambda k: launch_rf[k]["avg_launch_ms"])
    rf = dict(launch_rf[dom])
    rf["dominant_of"] = {k: round(v["avg_launch_ms"] * 1e3, 2) for k, v in launch_rf.items()}
    t_roof = max(step_flops / (peak_tf * 1e12), src_bytes / (HBM_PEAK_GBS * 1e9))
    srf = {"t_roof_us": t_roof * 1e6, "t_step_us": ms_step * 1e3, "frac": t_roof / (ms_step * 1e-3),
           "flops_per_step": step_flops, "bytes_per_step": src_bytes, "mfma_peak_tflops": peak_tf}
    # the step's launches (dad_pool only when it runs: the wave-centric tail launch pools itself)
    tr = step_traffic([names[k] for k in ("encode", "pool", "wgrad", "reduce", "optim") if k in ktimes] +
                      ([tail_name] if tail_name in (pmc_summary_kernels() or ()) else []))
    if tr is not None:
        srf["step_traffic_bytes"] = tr["bytes"]
        srf["step_traffic_over_compulsory"] = tr["bytes"] / src_bytes
        srf["step_traffic_per_kernel"] = tr["per_kernel"]
        srf["step_traffic_stale"] = tr["stale"]
    # MFMA utilisation of the encoder linears (north_star: >= 40 %): algorithmic FLOPs / time / peak
    enc_tf = enc_flops / (enc * 1e-3) / 1e12
    mf = {ekn: {"flops": enc_flops, "avg_ms": enc, "tflops": enc_tf, "util": enc_tf / peak_tf},
          "peak_tflops": peak_tf, "peak_source": "MI355X_MICROARCH.md dense MFMA peak (%s)" % precision}
    if wkey in ktimes:        # (a run that timed the encoder only has no weight-gradient time: no entries, not NaN)
        wg_tf = wg_flops / (wg * 1e-3) / 1e12
        mf[wname] = {"flops": wg_flops, "avg_ms": wg, "tflops": wg_tf, "util": wg_tf / peak_tf}
        mf["encoder_linears"] = {"flops": enc_flops + wg_flops, "ms": enc + wg,
                                 "util": (enc_flops + wg_flops) / ((enc + wg) * 1e-3) / 1e12 / peak_tf,
                                 "target": MFMA_TARGET}
    for kn in (k for k in (ekn, wname) if k in mf):   # matrix-pipe busy share from the committed PMC pass, when it covers this library
        pk = pmc_counters(kn)
        if pk and pk.get("mfma_busy_frac") is not None:
            mf[kn]["pmc_matrix_busy_frac"] = pk["mfma_busy_frac"]
            mf[kn]["pmc_stale"] = pk["stale"]
    kern["mfma_util"] = mf
    kern["encoder_roofline"] = enc_rf
    kern["launch_rooflines"] = launch_rf
    return rf, srf, kern


DUMP_LIMIT_BYTES = 64 << 20     # --dump-outputs writes at most this much (about 4 MB at the default batch)


def last_step_outputs(model, step):
    """What a caller of the timed path holds after its last step, as float32 host arrays: the loss
    terms DADStep.step() returns, the step's per-utterance outputs (DADStep.outputs(): embeddings,
    logits, DACP scores / predictions / mask / class probabilities, thresholds, the gradient
    and its clip norm) and the state the step updated (student and teacher parameters, Adam
    moments, DACP state).  Host copies: later steps do not change them."""
    out = {k: v for k, v in step.losses().items()}
    o = step.outputs(*step._last_shape)
    for k in ("e_clean", "e_teacher", "e_strong", "z_clean", "z_teacher", "z_strong", "score", "pred", "mask", "q",
              "w", "tau_before", "tau_after", "ecda_terms", "clip_norm", "clip_coef", "msum", "ecda_on", "grad"):
        out[k] = o[k]
    out.update(student_params=model.student_flat, teacher_params=model.teacher_flat, exp_avg=step.exp_avg,
               exp_avg_sq=step.exp_avg_sq, dacp=step.dacp)
    torch.cuda.synchronize()
    return {k: np.atleast_1d(v.detach().to(torch.float32).cpu().numpy()) for k, v in out.items()}


def dump_outputs(path, arrays):
    """--dump-outputs: one <name>.npy (float32) per array of last_step_outputs(); returns the shapes
    written.  Past DUMP_LIMIT_BYTES in all (a very large --batch), every array above an equal share
    of the limit is written as a fixed sample of its elements: the same seeded, sorted indices into
    the flattened array in every run."""
    share = DUMP_LIMIT_BYTES // max(1, len(arrays))
    sample = sum(a.nbytes for a in arrays.values()) > DUMP_LIMIT_BYTES
    os.makedirs(path, exist_ok=True)
    shapes = {}
    for k, a in sorted(arrays.items()):
        if sample and a.nbytes > share:
            idx = np.sort(np.random.RandomState(0).choice(a.size, share // a.itemsize, replace=False))
            a = a.reshape(-1)[idx]
        np.save(os.path.join(path, k + ".npy"), a)
        shapes[k] = list(a.shape)
    return shapes


def snapshot(model, step):
    """Model parameters + step state (Adam moments, DACP state, step counters)."""
    return model.student_flat.clone(), model.teacher_flat.clone(), step.state_dict()


def restore(model, step, snap):
    with torch.no_grad():
        model.student_flat.copy_(snap[0])
        model.teacher_flat.copy_(snap[1])
    step.load_state_dict(snap[2])
    step.refresh_shadow()


def parity_block(model, step, view, snap, batch, epoch, precision):
    """The timed mode (fp16 or bf16 operands) vs fp32 (the reference's arithmetic, exact-f32 MFMA) on
    the first timed batch from the state the timed region started in, with the same counter-RNG
    draws (same seed and global step): the four loss terms, the student logits and the DACP mask.
    The golden replays of tests/test_gpu_throughput_parity.py pin the same comparison against the
    reference."""
    c, nb = batch
    out = {}
    for prec in (precision, "fp32"):
        restore(model, step, snap)
        s = PKG.DADStep(model, view, precision=prec, rng="counter", seed=step.seed)
        s.load_state_dict(snap[2])
        l = s.step(c, nb, epoch)
        torch.cuda.synchronize()
        Bc, Bn = s._last_shape
        o = s.outputs(Bc, Bn)
        out[prec] = {"losses": {k: float(v) for k, v in l.items()},
                     "z_clean": o["z_clean"].detach().cpu().double(), "z_strong": o["z_strong"].detach().cpu().double(),
                     "mask": o["mask"].detach().cpu()}
    restore(model, step, snap)
    b, f = out[precision], out["fp32"]
    rel = lambda a, r: float((a - r).abs().max() / max(1e-6, float(r.abs().max())))
    return {"batch": "first timed batch", "mode": precision,
            "reference_mode": "fp32 (exact-f32 MFMA), same counter-RNG draws",
            "losses_" + precision: b["losses"], "losses_fp32": f["losses"],
            "loss_err": {k: abs(b["losses"][k] - f["losses"][k]) / max(1.0, abs(f["losses"][k])) for k in f["losses"]},
            "z_clean_err": rel(b["z_clean"], f["z_clean"]), "z_strong_err": rel(b["z_strong"], f["z_strong"]),
            "mask_equal": bool(torch.equal(b["mask"], f["mask"])), "mask_sum": float(f["mask"].sum()),
            "bound": 1e-4 if precision == "fp16" else None,
            "err_definition": "losses |x - fp32| / max(1, |fp32|); logits max|x - fp32| / max|fp32|"}


def side_mode(model, view, data, B, T, args, precision, n):
    """Another precision of the same step timed over n steps on the resident batches (eager
    launches), with its own per-kernel timing and rooflines: fp32 (the reference's arithmetic,
    exact-f32 MFMA, f32 peak) or bf16 (BASELINE configs[1]'s named dtype, bf16 peak)."""
    s32 = PKG.DADStep(model, view, precision=precision, rng="counter", seed=5)
    ahead = precision != "fp32" and not args.no_ahead
    pos = [0]

    def run1():
        i = pos[0]
        pos[0] += 1
        s32.step(data[i % 4][0], data[i % 4][1], args.epoch, next_batch=data[(i + 1) % 4] if ahead else None)
    for _ in range(3):
        run1()
    torch.cuda.synchronize()
    timer = PKG._lib.KernelTimer(4, n // 4 + 1, kernels=timed_kernels(precision, ahead))
    t1 = time.perf_counter()
    for _ in range(n):
        run1()
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t1) / n
    enc = timer.stop()          # (one timer at a time: dad_timing_start refuses a second)
    kt = kernel_pass(run1, max(8, n // 2))
    kt.update(enc)
    rf, srf, kern = rooflines(kt, B * T, B * T, dt * 1e3, precision, tail_kernel(B, B, class_aware(view)),
                              prepped_ahead=ahead)
    return {"value": B / dt, "ms_per_step": dt * 1e3, "steps": n, "dtype": "f32" if precision == "fp32" else precision,
            "launch": "eager", "roofline": rf, "step_roofline": srf, "kernels": kern}


def _free_port():
    import socket
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def launch_ranks(n, argv):
    """`bench.py --gpus N` without a launcher: N rank processes of this script, one per GPU,
    with the torchrun environment (RANK / LOCAL_RANK / WORLD_SIZE / MASTER_*).  This parent
    never touches the GPU.  If a rank fails, the others are stopped (by PID) and the first
    non-zero exit code is returned."""
    port = _free_port()
    procs = []
    for r in range(n):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(n), LOCAL_WORLD_SIZE=str(n),
                   MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
        env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        procs.append(subprocess.Popen([sys.executable, os.path.abspath(__file__)] + list(argv), env=env))
    rc = 0
    live = list(procs)
    while live:
        time.sleep(0.2)
        for p in list(live):
            code = p.poll()
            if code is None:
                continue
            live.remove(p)
            if code != 0 and rc == 0:
                rc = code
                for q in live:
                    q.kill()
    return rc


def flavor_view(args):
    """The step's config for the workload: the dataset flavour's defaults (config.py), with
    CASIA's DACP + ECDA forced on for BASELINE config 4 (C/config_casia.py:85-86 overridden)."""
    ov = {}
    if args.force_ecda:
        ov.update(USE_DACP=True, USE_ECDA=True)
    return PKG.ConfigView(None, flavor=args.flavor, **ov)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--precision", default="fp16", choices=["fp16", "bf16", "fp32"])
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--frames", type=int, default=300)
    ap.add_argument("--epoch", type=int, default=60)
    ap.add_argument("--flavor", default="iemocap", choices=["iemocap", "casia", "emodb"])
    ap.add_argument("--force-ecda", action="store_true", help="USE_DACP=USE_ECDA=True (CASIA, BASELINE config 4)")
    ap.add_argument("--snr", type=float, default=5.0, help="SNR (dB) of the synthetic noisy branch")
    ap.add_argument("--mixed", action="store_true",
                    help="BASELINE configs[4]: mixed IEMOCAP+CASIA+EMODB batches, K-fold sweep (--folds)")
    ap.add_argument("--folds", type=int, default=5)
    ap.add_argument("--comm", default="rccl", choices=["rccl", "gloo"],
                    help="gradient all-reduce transport for N > 1 (gloo lets ranks share one GPU)")
    ap.add_argument("--cpu-steps", type=int, default=10)
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--fp32-steps", type=int, default=24, help="also time the FP32 parity mode (N=1)")
    ap.add_argument("--bf16-steps", type=int, default=48, help="also time the BF16 mode (N=1, fp16 runs)")
    ap.add_argument("--randlab-steps", type=int, default=48,
                    help="also time the step on batches with random class sizes (labels drawn uniformly, as a "
                         "random batch of a balanced corpus has them; N=1)")
    ap.add_argument("--kernel-steps", type=int, default=32,
                    help="steps of the per-kernel timing pass after the timed region (0: none)")
    ap.add_argument("--no-data-path", action="store_true", help="skip the device collate measurement (N=1)")
    ap.add_argument("--no-parity", action="store_true", help="skip the 16-bit-vs-fp32 parity block (N=1)")
    ap.add_argument("--no-ahead", action="store_true",
                    help="16-bit modes: every step prepares its own rows (no next-batch preparation in the tail launch)")
    ap.add_argument("--prep-under-exchange", default="auto", choices=["auto", "off", "clean", "noisy", "all"],
                    help="16-bit modes: which of the next batch's rows are prepared on a side stream from the end of "
                         "the backward (under the all-reduce) instead of inside the step's launches; auto = off (measured "
                         "slower at exchange windows of 0-20 us, DESIGN.md section 5)")
    ap.add_argument("--exchange-us", type=float, default=0.0,
                    help="N = 1 only: a spin of about this many microseconds after the backward, standing in for a DP "
                         "step's all-reduce window (measures the --prep-under-exchange layouts on one GPU)")
    ap.add_argument("--settle-ms", type=float, default=50.0,
                    help="untimed headline steps (about this many ms of GPU time) right before the warm-up")
    ap.add_argument("--launch", default="eager", choices=["graph", "eager"],
                    help="timed steps as eager launches (default) or hipGraph replays (one graph per resident batch; "
                         "measured no faster on this ROCm, DESIGN.md §5)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the last timed step computed (losses, per-utterance "
                         "outputs, updated parameters and state) as DIR/<name>.npy in float32; the inputs are seeded, "
                         "so two runs with the same arguments can be compared output for output")
    ap.add_argument("--full", action="store_true",
                    help="after the timed steps also run the per-kernel pass, the parity block, the side legs (FP32 / "
                         "BF16 modes, random labels, data path) and the CPU baseline (each with its own switch above); "
                         "without it the run ends with the timed steps")
    args = ap.parse_args()
    if args.steps < 1 or args.warmup < 0:
        ap.error("--steps must be at least 1 and --warmup at least 0")
    settle_steps = 0
    dumped = {}

    def capture(s):          # written right after the timed steps, before anything else runs a step
        if args.dump_outputs and rank == 0:
            dumped.update(dump_outputs(args.dump_outputs, last_step_outputs(model, s)))

    if "WORLD_SIZE" not in os.environ and args.gpus > 1:
        sys.exit(launch_ranks(args.gpus, sys.argv[1:]))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus:
        print("bench.py: --gpus %d but WORLD_SIZE=%d" % (args.gpus, world), file=sys.stderr)
        sys.exit(2)
    ndev = torch.cuda.device_count()
    if args.comm == "rccl" and world > 1 and local >= ndev:
        print("bench.py: rank %d has no GPU of its own (%d visible); RCCL needs one GPU per rank "
              "(--comm gloo shares)" % (local, ndev), file=sys.stderr)
        sys.exit(2)
    dev = torch.device("cuda", local % max(ndev, 1))
    torch.cuda.set_device(dev)
    dist = None
    if world > 1:
        import datetime
        import torch.distributed as dist
        # control plane (barriers, the max-over-ranks clock, RCCL id broadcast) on gloo; the
        # data path's one collective is the step's own all-reduce (RCCL through the C ABI)
        dist.init_process_group("gloo", timeout=datetime.timedelta(seconds=300))
    PKG.lib()
    B, T = args.batch, args.frames

    model = PKG.SSRLModel().to(dev)
    P = init_model_weights(model, seed=0)
    comm = None
    if world > 1:
        comm = PKG.DPComm.from_torch_distributed() if args.comm == "rccl" else PKG.ProcessGroupComm()
    ranks_seen = comm.ranks_seen(dev) if comm is not None else 1
    if ranks_seen != args.gpus:
        print("bench.py: the %s transport connected %d ranks, expected %d" % (args.comm, ranks_seen, args.gpus),
              file=sys.stderr)
        sys.exit(3)
    folds = None
    if args.mixed:
        step, folds, ktimes, table = run_mixed(args, model, dev, rank, world, dist, comm, after_timed=capture)
        elapsed = sum(f["seconds"] for f in folds)
        total_utts = sum(f["utterances"] for f in folds)
        timed_steps = args.steps * args.folds
        rows_per_step = statistics.mean(f["avg_valid_frames_per_step"] for f in folds)
        view = step.view
    else:
        view = flavor_view(args)
        step = PKG.DADStep(model, view, precision=args.precision, rng="counter", seed=1000 + rank, comm=comm,
                           prep_under_exchange={"auto": None, "off": 0, "clean": 1, "noisy": 2,
                                                "all": 3}[args.prep_under_exchange])
        data = make_batches(P, N_BATCHES, B, T, seed=17 + rank, device=dev, snr_db=args.snr)
        torch.cuda.synchronize()

        pos = [0]
        spin = None
        if args.exchange_us > 0 and world == 1:
            # torch.cuda._sleep spins for a number of GPU clock cycles: calibrated here against events
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            torch.cuda._sleep(1000000)
            e1.record()
            torch.cuda.synchronize()
            cyc = int(args.exchange_us * 1e6 / (e0.elapsed_time(e1) * 1e3))
            spin = lambda: torch.cuda._sleep(cyc)

        def run(n):
            # each step names the next resident batch: its augmentation + 16-bit conversion run in
            # this step's tail launch (DADStep.step(next_batch=...)); bit-identical either way
            for _ in range(n):
                i = pos[0]
                pos[0] += 1
                c, nb = data[i % len(data)]
                step.step(c, nb, args.epoch, next_batch=None if args.no_ahead else data[(i + 1) % len(data)],
                          after_backward=spin)

        # Order: the clock-settling run (--settle-ms), the W warm-up steps right before the timed
        # region (it starts on a GPU that has been busy for ~50 ms, with the warm-up's prepared rows
        # and caches in place; round 2 had measured the clock ramp of a cold start: 137 -> 130 -> 124
        # us per step over consecutive 20-step segments), the timed region, then the per-kernel pass,
        # the parity block (from the state the region started in) and the side legs.
        parity = fp32 = bf16 = data_path = randlab = None
        side = args.full and rank == 0 and world == 1
        launch = args.launch
        if launch == "graph" and isinstance(comm, PKG.ProcessGroupComm):
            launch = "eager (the gloo all-reduce runs on the host: not capturable)"
        graphs = None
        timer = None
        enc_events = []
        if launch != "graph":
            # every EVENT_EVERY-th timed step records hip events at its kernel boundaries.  The
            # events are created here, BEFORE the warm-up (milliseconds of host time: created
            # between the warm-up and the clock they had idled the GPU right before the timed
            # region, and a short region then started on lowered clocks), and the timer is reset
            # after the warm-up, so only timed steps are counted
            timer = PKG._lib.KernelTimer(event_every(args.steps), args.steps // event_every(args.steps) + 1,
                                         kernels=timed_kernels(args.precision, not args.no_ahead))
        if args.settle_ms > 0:
            # clock settling: untimed steps of the headline, enqueued back to back for about
            # settle_ms of GPU time right before the warm-up (the side legs above leave the GPU idle
            # between their pieces: a 20-step region after them ran 4-6 % above the steady rate,
            # tools/gpu_region_ab.sh, and a GPU idle for 2 s needs ~100 steps to settle,
            # tools/region_segments.py).  Not part of W or of the timed region; in the line as
            # settle_steps.
            settle_steps = max(1, int(args.settle_ms / 0.1))
            run(settle_steps)
        else:
            settle_steps = 0
        run(args.warmup)
        torch.cuda.synchronize()
        snap = snapshot(model, step)          # the state the first timed step starts from
        if launch == "graph":
            # the capture advances the host's step counters by len(data): the timed replays are
            # steps warmup .. warmup+7 of the same run, cycled; the encoder of the last batch's
            # graph is timed by stream events around its own graph (every 8th step)
            split = len(data) - 1
            try:
                graphs = capture_steps(step, data, args.epoch, split=split,
                                       ahead=args.precision != "fp32" and not args.no_ahead)
            except Exception as e:   # (e.g. a transport that refuses capture): eager, said so in the line
                err = str(e).splitlines()[0][:200] if str(e) else type(e).__name__
                restore(model, step, snap)
                torch.cuda.synchronize()
                launch = "eager (graph capture failed: %s)" % err
            if graphs is not None:
                n_ev = sum(1 for i in range(args.steps) if i % len(graphs) == split)
                enc_events = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
                              for _ in range(n_ev)]
                for e0, e1 in enc_events:   # first use outside the timed region
                    e0.record()
                    e1.record()
                torch.cuda.synchronize()
        if graphs is None and timer is None:
            # (graph capture failed: eager after all) one event set per recorded step only (each
            # set is 8 events created up front: sized for every step, a 200-step region had created
            # 1,608 events right before its clock)
            timer = PKG._lib.KernelTimer(event_every(args.steps), args.steps // event_every(args.steps) + 1,
                                         kernels=timed_kernels(args.precision, not args.no_ahead))
        if timer is not None:
            timer.reset()                     # (host only: the warm-up's steps are not counted)

        def timed(n):
            if graphs is None:
                run(n)
                return
            k = 0
            for i in range(n):
                gs = graphs[i % len(graphs)]
                if len(gs) == 1:
                    gs[0].replay()
                else:
                    e0, e1 = enc_events[k]
                    k += 1
                    e0.record()
                    gs[0].replay()
                    e1.record()
                    gs[1].replay()
        torch.cuda.synchronize()
        if dist:
            dist.barrier()
        t0 = time.perf_counter()
        timed(args.steps)
        torch.cuda.synchronize()
        if dist:
            dist.barrier()
        elapsed = time.perf_counter() - t0
        if timer is not None:
            ktimes = timer.stop()
        else:
            ms_enc = [e0.elapsed_time(e1) for e0, e1 in enc_events]
            ktimes = {"encode": (sum(ms_enc) / len(ms_enc), len(ms_enc))} if ms_enc else {}
        if dist:
            t = torch.tensor([elapsed], dtype=torch.float64)
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
            elapsed = float(t.item())
        losses = {k: float(v) for k, v in step.losses().items()}   # the last timed (or captured) step's
        nbc = step._last_shape
        msum = float(step.outputs(*nbc)["msum"])
        ecda_on = float(step.outputs(*nbc)["ecda_on"])
        capture(step)
        table = kernel_pass(lambda: run(1), args.kernel_steps) if args.full else {}
        if side and args.precision != "fp32" and not args.no_parity:
            parity = parity_block(model, step, view, snap, data[args.warmup % len(data)], args.epoch,
                                  args.precision)
        if side:
            # The side legs (the FP32 / BF16 modes, random labels, the data path) run after the timed
            # region, from the weights it left: run before it, from the initial weights, every kernel
            # read 1-3 us slower on the same batches (tools/data_effect.py: the encoder 30.4-31.6 against
            # 28.7 us after 500 steps, the weight gradient 34.5-35.6 against 33.4; the chip's clock
            # follows the operands), which the random-label leg then showed as the labels' cost
            # (0.1148 against 0.0976 ms; from trained weights 0.1026 against 0.1005).
            if args.precision != "fp32":
                if args.fp32_steps > 0:
                    fp32 = side_mode(model, view, data, B, T, args, "fp32", args.fp32_steps)
                if args.precision == "fp16" and args.bf16_steps > 0:
                    bf16 = side_mode(model, view, data, B, T, args, "bf16", args.bf16_steps)
            if args.randlab_steps > 0:
                # the headline batches hold exactly B/4 utterances per class; a trainer's random batches
                # have Binomial(B, 1/4) class sizes, and classes of more than 32 ECDA members take the
                # 64-row tiling of the tail launch's class blocks
                rdata = make_batches(P, N_BATCHES, B, T, seed=29, device=dev, snr_db=args.snr, random_labels=True)
                randlab = side_mode(model, view, rdata, B, T, args, args.precision, args.randlab_steps)
                randlab["data"] = "synthetic, labels drawn uniformly per utterance (random class sizes)"
                del rdata
            if not args.no_data_path:
                data_path = data_path_bench(step, B, T, args.epoch, dev, P)
        timed_steps = args.steps
        total_utts = B * world * args.steps
        rows_per_step = 2 * B * T
    if args.mixed:
        parity = fp32 = bf16 = data_path = randlab = None
        losses = {k: float(v) for k, v in step.losses().items()}
        nbc = step._last_shape
        msum = float(step.outputs(*nbc)["msum"])
        ecda_on = float(step.outputs(*nbc)["ecda_on"])

    if rank != 0:
        if comm is not None:
            comm.close()
        if dist:
            dist.destroy_process_group()
        return
    ms = elapsed / timed_steps * 1e3
    value = total_utts / elapsed
    rows = rows_per_step / 2                            # valid frames per batch (clean = noisy count here)
    if args.mixed:
        workload = ("IEMOCAP+CASIA+EMODB mixed-batch DAD step (configs[4]): batch=%d/GPU of utterances from all three "
                    "corpora (synthetic stores with each corpus's utterance count and fold structure, %d-%d frames), "
                    "DAD config rotating IEMOCAP / CASIA (DACP+ECDA) / EMODB per batch, %d-fold sweep, fused "
                    "store-mode loaders, epoch %d, counter-RNG augmentation" % (B, 100, 300, args.folds, args.epoch))
    elif args.flavor == "iemocap":
        workload = ("IEMOCAP DAD train step (configs[%d]): batch=64/GPU, T=300x768 synthetic emotion2vec-shaped "
                    "features, post-warm-up epoch %d (CE+KL+ECDA active), counter-RNG augmentation (16-bit modes: prepared for "
                    "each next step inside the tail launch (noisy rows) and the weight-gradient launch (clean rows))"
                    % (1 if world == 1 else 2, args.epoch))
    else:
        workload = ("%s DAD train step%s: batch=%d/GPU, T=%dx768 synthetic features, noisy branch at SNR %g dB, "
                    "post-warm-up epoch %d, counter-RNG augmentation (16-bit modes: prepared for each next step inside the "
                    "tail and weight-gradient launches)"
                    % (args.flavor.upper(), " (configs[3]: DACP+ECDA forced on; SCL is 0 in the reference)"
                       if args.force_ecda else "", B, T, args.snr, args.epoch))
    # per-kernel table: the separate pass, with the timed region's encoder entry
    kt = dict(table)
    kt.update(ktimes)
    rf, srf, kern = rooflines(kt, rows, rows, ms, args.precision,
                              tail_kernel(B, B, True if args.mixed else class_aware(view)),
                              prepped_ahead=not args.mixed and not args.no_ahead)
    if not args.mixed and graphs:
        src = "encoder: stream events around the encoder graph of every %d-th replayed step" % len(graphs)
    else:
        tk = timed_kernels(args.precision, not args.mixed and not args.no_ahead)[0]
        tks = timed_kernels(args.precision, not args.mixed and not args.no_ahead)
        src = "%s: HIP events around them in the timed region (every %d-th step)" % (
            ", ".join({"wgrad": "weight gradient (+ clean-row conversion)", "tail": "tail launch (+ pooling, noisy-row "
                       "preparation)", "encode": "encoder"}[k] for k in tks), event_every(args.steps))
    if args.full:
        kern["source"] = ("%s; the other kernels: a separate eager pass of %d steps after it (events at every "
                          "boundary of every 2nd step)" % (src, args.kernel_steps))
    else:
        kern["source"] = "%s; the other kernels are timed only with --full" % src
    line = {
        "metric": METRIC, "value": value, "unit": "utterances/s", "n_gpus": world, "steps": args.steps,
        "warmup": args.warmup, "settle_steps": settle_steps, "ms_per_step": ms, "higher_is_better": True,
        "scaling": "weak",
        "vs_baseline": None, "dtype": args.precision, "data": "synthetic",
        "dtype_note": {"fp16": "encoder and weight-gradient GEMMs on fp16 operands (11-bit significand), fp32 "
                               "accumulation; everything else fp32 (the mode that meets north_star's 1e-4)",
                       "bf16": "encoder and weight-gradient GEMMs on bf16 operands, fp32 accumulation",
                       "fp32": "exact-f32 MFMA throughout"}[args.precision],
        "config": {"workload": workload, "flavor": "mixed" if args.mixed else args.flavor, "snr_db": args.snr,
                   "global_batch": B * world, "per_gpu_batch": B, "seq_len": T, "feature_dim": 768,
                   "parallelism": "dp%d" % world},
        "comm": {"transport": args.comm if world > 1 else None, "ranks_seen": ranks_seen,
                 "next_rows_under_exchange": {0: "none", 1: "clean", 2: "noisy", 3: "clean+noisy"}[
                     step._defer_parts() if hasattr(step, "_defer_parts") else 0],
                 "exchange_standin_us": args.exchange_us if world == 1 else None},
        "launch": launch if not args.mixed else "eager",
        "roofline": rf, "step_roofline": srf, "kernels": kern,
        "losses_last_step": losses, "mask_sum_last_step": msum, "ecda_on_last_step": ecda_on,
    }
    if parity is not None:
        line["parity"] = parity
    if folds is not None:
        line["folds"] = folds
    if fp32 is not None:
        line["fp32_mode"] = fp32
    if bf16 is not None:
        line["bf16_mode"] = bf16
    if randlab is not None:
        line["random_labels"] = randlab
    if data_path is not None:
        line["data_path"] = data_path
    if args.dump_outputs:
        line["dumped_outputs"] = dumped
    if args.full and world == 1 and not args.no_cpu_baseline:
        line["cpu_baseline"] = cpu_baseline(B, T, args.cpu_steps, args.epoch)
    print(json.dumps(line), flush=True)
    if comm is not None:
        comm.close()
    if dist:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
