"""The reference trainers' analysis records, kept on the device while the fused step runs.

  TrainingTrace.bias_log()   Trainer.bias_analysis_log        I/train.py:94-95, 279-284, 425-437
  TrainingTrace.history()    Trainer.training_history's DACP / ECDA rows and disagreement series
                                                              I/train.py:498-517, 546-551
  TrainingTrace.save()       Trainer._save_analysis_data      I/train.py:674-700

The reference appends a log entry per tracked row inside train_step, with a .cpu() of the ids and three
.item() reads per row: a host sync per step.  Here DADStep enqueues one dad_trace_append (csrc/trace.hip)
behind the step's tail launch, which compacts the tracked rows of that step's score / pred / mask into a
device buffer; nothing is read back until bias_log() / save().  So the log costs one small launch per step
and the reference's limit of 50 samples is no longer needed (tracked="all").

analyze_confirmation_bias.py, analyze_dacp_evolution.py and analyze_disagreement.py read the two files
save() writes.
"""
import json
import os
import warnings

import numpy as np
import torch

from . import _lib

BIAS_LOG_FILE = "confirmation_bias_log.json"
HISTORY_FILE = "training_history.json"
_HISTORY_KEYS = ("dacp_ema_thresholds", "dacp_class_quality", "ecda_class_attention")


def choose_tracked(n_samples, tracked=50):
    """The tracked sample ids.  An int k: the reference's draw (I/train.py:279-284),
    np.random.choice(n_samples, k, replace=False).tolist() from the global NumPy RNG when n_samples > k,
    else [] (the reference leaves tracked_sample_indices None: no logging).  "all": every id.  An iterable
    of ids: as given."""
    n_samples = int(n_samples)
    if isinstance(tracked, str):
        if tracked != "all":
            raise ValueError("tracked must be an int, an iterable of ids or 'all', got %r" % (tracked,))
        return list(range(n_samples))
    if isinstance(tracked, (int, np.integer)) and not isinstance(tracked, bool):
        if n_samples > tracked:
            return np.random.choice(n_samples, int(tracked), replace=False).tolist()
        return []
    ids = [int(i) for i in tracked]
    if any(i < 0 or i >= n_samples for i in ids):
        raise ValueError("a tracked id lies outside [0, %d)" % n_samples)
    return ids


def pack_bitmap(ids, n_samples):
    """dad_trace_append's `tracked` argument: uint32 [ceil(n_samples / 32)], bit (id & 31) of word (id >> 5)."""
    bits = np.zeros(-(-int(n_samples) // 32) * 32, dtype=bool)
    if len(ids):
        bits[np.asarray(ids, dtype=np.int64)] = True
    # bit k of a word = flag 32 * word + k: little-endian bit order inside little-endian words
    return np.packbits(bits.reshape(-1, 32), axis=1, bitorder="little").view("<u4").reshape(-1).astype(np.uint32)


def decode_records(words, capacity):
    """(entries, offered) of a trace buffer's int32 words (dad.h DAD_TRACE_*): the reference's log entries
    (I/train.py:430-436, same keys and Python types) of the min(offered, capacity) records, in append order."""
    words = np.ascontiguousarray(words, dtype=np.int32).reshape(-1)
    offered = int(words[0])
    n = max(0, min(offered, int(capacity)))
    H, R = _lib.TRACE_HDR_WORDS, _lib.TRACE_REC_WORDS
    rec = words[H:H + n * R].reshape(n, R)
    score = rec[:, 3].copy().view(np.float32)
    out = []
    for (ep, sid, w2, _), sc in zip(rec.tolist(), score.tolist()):     # .tolist(): Python ints / floats
        out.append({"epoch": ep, "sample_id": sid, "pseudo_label": w2 & 0xff, "certainty_score": sc,
                    "is_masked_in": bool(w2 & _lib.TRACE_MASKED_IN)})
    return out, offered


class TrainingTrace:
    """The confirmation-bias log and the per-epoch DACP / ECDA history of one training run.

    Args:
        n_samples: samples of the noisy training set (len(noisy_loader.dataset)): the range of batch['id'].
        tracked: int k (the reference's 50: k random ids from the global NumPy RNG, none when n_samples <= k),
            an iterable of ids, or "all".
        epochs: the run's epoch count; sizes the log as len(tracked) * epochs records (a sample is met at
            most once per epoch).  Not needed with `capacity`.
        capacity: records the log holds (16 bytes each).  Records past it are counted and dropped (`dropped`).
        device: where the buffers live (default: the current cuda device).  On 'cpu' everything but the
            step's append works (decoding, history, save).

    Attach with DADStep(..., trace=tr) or `step.trace = tr`; call end_epoch(step) after step.epoch_end()
    (checkpoint.train_epoch does) and add_validation(name, results) after each validation; save(results_dir)
    at the end.  One trace per process: DP ranks keep their own."""

    def __init__(self, n_samples, tracked=50, epochs=None, capacity=None, device=None):
        self.n_samples = int(n_samples)
        if not 1 <= self.n_samples <= 2 ** 31 - 1:
            raise ValueError("n_samples must be in [1, 2^31 - 1], got %d" % self.n_samples)
        self.tracked_sample_indices = choose_tracked(self.n_samples, tracked)
        if capacity is None:
            if epochs is None:
                raise ValueError("pass epochs (the log holds len(tracked) * epochs records) or capacity")
            capacity = len(self.tracked_sample_indices) * int(epochs)
        self.capacity = int(capacity)
        if not 0 <= self.capacity <= 2 ** 31 - 1:
            raise ValueError("capacity must be in [0, 2^31 - 1], got %d" % self.capacity)
        device = torch.device("cuda" if device is None else device)
        if device.type == "cuda" and device.index is None:      # (an explicit index: it is compared with the ids')
            device = torch.device("cuda", torch.cuda.current_device())
        self.device = device
        words = _lib.TRACE_HDR_WORDS + self.capacity * _lib.TRACE_REC_WORDS
        self.buffer = torch.zeros(words, dtype=torch.int32, device=self.device)    # zero-filled once (dad.h)
        bitmap = pack_bitmap(self.tracked_sample_indices, self.n_samples)
        self.bitmap = torch.from_numpy(bitmap.view(np.int32)).to(self.device)      # (torch has no uint32 ops: same bits)
        self._rows = []            # per epoch: device [3][4] (tau, Q, ECDA class attention)
        self._series = {}          # disagreement_rate_<domain>: host floats
        self._warned = False
        self.offered = 0           # records offered, as of the last bias_log() / dropped read

    @classmethod
    def for_loader(cls, noisy_loader, tracked=50, epochs=None, capacity=None, device=None):
        """A trace over len(noisy_loader.dataset) samples, as the reference counts them (I/train.py:280)."""
        if device is None:
            device = getattr(noisy_loader.dataset, "device", None)
        return cls(len(noisy_loader.dataset), tracked=tracked, epochs=epochs, capacity=capacity, device=device)

    @property
    def active(self):
        """The reference's `if self.tracked_sample_indices` (I/train.py:425)."""
        return bool(self.tracked_sample_indices)

    # ------------------------------------------------------------------------- the step's hook
    def device_ids(self, ids, Bn):
        """The noisy batch's 'id' as dad_trace_append reads it: int64 [Bn] on the trace's device (the
        loaders' own tensor as it is; a host tensor is moved)."""
        if not torch.is_tensor(ids):
            ids = torch.as_tensor(np.asarray(ids))
        if ids.dim() != 1 or ids.shape[0] != Bn:
            raise ValueError("the noisy batch's 'id' has shape %s, its batch %d rows" % (tuple(ids.shape), Bn))
        if not (ids.dtype == torch.int64 and ids.device == self.device and ids.is_contiguous()):
            ids = ids.to(device=self.device, dtype=torch.int64).contiguous()
        return ids

    def append(self, tail, Bn, ids, epoch, stream):
        """Enqueue one step's entries on `stream` (a raw stream handle), behind the launch that writes `tail`.
        ids: device_ids() of the noisy batch's 'id'."""
        fn = _lib.require("dad_trace_append", "a TrainingTrace")
        _lib.check(fn(_lib.ptr(tail), Bn, _lib.ptr(ids), _lib.ptr(self.bitmap), self.n_samples, int(epoch),
                      _lib.ptr(self.buffer), self.capacity, stream), "dad_trace_append")
        self._ids_keep = ids       # (a converted copy must outlive the enqueue; the stream orders its reuse)

    # ------------------------------------------------------------------------------- the log
    def _decode(self):
        entries, offered = decode_records(self.buffer.cpu().numpy(), self.capacity)    # the one copy
        self.offered = offered
        lost = max(0, offered - self.capacity)
        if lost and not self._warned:
            self._warned = True
            warnings.warn("TrainingTrace: %d of %d log records were dropped (capacity %d)"
                          % (lost, offered, self.capacity), RuntimeWarning)
        return entries, lost

    def bias_log(self):
        """Trainer.bias_analysis_log: the entries in append order (one device->host copy)."""
        return self._decode()[0]

    @property
    def dropped(self):
        """max(0, records offered - capacity); a non-zero value warns once."""
        return self._decode()[1]

    # --------------------------------------------------------------------------- the history
    def end_epoch(self, step):
        """The epoch's DACP / ECDA rows (I/train.py:498-517), after step.epoch_end(): tau, Q and
        exp(ECDA_CLASS_ATTENTION_LAMBDA * (Q.mean() - Q)), computed and kept on the device."""
        tau, q = step.ema_thresholds, step.class_quality_scores
        att = torch.exp(step.view.ECDA_CLASS_ATTENTION_LAMBDA * (q.mean() - q))
        self._rows.append(torch.stack([tau, q, att]))

    def add_validation(self, domain_name, results):
        """Trainer.validate's disagreement series (I/train.py:546-551)."""
        if results is not None and "disagreement_rate" in results:
            self._series.setdefault("disagreement_rate_%s" % domain_name.lower(), []).append(
                float(results["disagreement_rate"]))

    def history(self):
        """Trainer.training_history's analysis keys as lists (one device->host copy)."""
        rows = torch.stack(self._rows).cpu().tolist() if self._rows else []
        out = {k: [r[j] for r in rows] for j, k in enumerate(_HISTORY_KEYS)}
        out.update({k: list(v) for k, v in self._series.items()})
        return out

    def save(self, results_dir):
        """Trainer._save_analysis_data (I/train.py:674-700): reports/training_history.json, and
        reports/confirmation_bias_log.json when the log is not empty.  Returns the paths written."""
        reports = os.path.join(results_dir, "reports")
        os.makedirs(reports, exist_ok=True)
        paths = [os.path.join(reports, HISTORY_FILE)]
        with open(paths[0], "w") as f:
            json.dump(self.history(), f, indent=4)
        log = self.bias_log()
        if log:
            paths.append(os.path.join(reports, BIAS_LOG_FILE))
            with open(paths[1], "w") as f:
                json.dump(log, f, indent=4)
        return paths
