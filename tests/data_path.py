"""The device data path's cases, NumPy references and conditions (tests/test_data_path_cpu.py checks them on the CPU,
tests/test_gpu_data_path.py holds the kernels to them).  Nothing here imports the package or reads a kernel: the
references restate include/dad.h's contract for dad_collate, dad_collate_index and dad_collate_index_epoch, in integer
NumPy on bit patterns wherever a value is widened or rounded, so a NaN payload or a signed zero survives the
reference itself.

Widening (a store element as every consumer sees it in f32):
  fp16   bits.view(float16).astype(float32)         (exact: every fp16 value, subnormals included, is an f32 value)
  bf16   bits.astype(uint32) << 16                  (the bf16 bits are the f32's high half)
Operand rounding (what a 16-bit precision multiplies): round to nearest, ties to even, written out on the bit patterns
(f32_to_f16_bits, f32_to_bf16_bits); fp16 -> bf16 and bf16 -> fp16 are the widening followed by one of them.
"""
import functools

import numpy as np

DIM = 768
GUARD = 64                               # guard elements behind every output buffer
PAD_SENTINEL = 0xA5
INT_SENTINEL = -7
FEAT_SENTINEL = 0x7FA5A5A5               # a NaN no widening of a 16-bit pattern gives (low 13 bits set)
INT64_MIN = -2 ** 63
STORES = ("f32", "f16", "bf16")


# ---- bit-pattern arithmetic -------------------------------------------------------------------------------------------
def widen_f16(bits):
    return np.ascontiguousarray(bits, np.uint16).view(np.float16).astype(np.float32).view(np.uint32)


def widen_bf16(bits):
    return np.asarray(bits, np.uint16).astype(np.uint32) << np.uint32(16)


def widen(bits, dt):
    """uint32 f32 patterns of a store's elements: 16-bit patterns widened, f32 patterns as they are."""
    if dt == "f32":
        return np.asarray(bits, np.uint32)
    return widen_f16(bits) if dt == "f16" else widen_bf16(bits)


def f32_to_bf16_bits(u, mode="rne"):
    """f32 patterns -> bf16 patterns, round to nearest even (a NaN stays a NaN).  mode 'trunc' is the wrong-answer
    control: the low half dropped."""
    u = np.asarray(u, np.uint32).astype(np.uint64)
    nan = ((u >> 23) & 0xFF == 0xFF) & (u & 0x7FFFFF != 0)
    r = (u >> 16) if mode == "trunc" else ((u + 0x7FFF + ((u >> 16) & 1)) >> 16)
    return np.where(nan, (u >> 16) | 0x40, r).astype(np.uint16)


def f32_to_f16_bits(u, mode="rne"):
    """f32 patterns -> fp16 patterns, round to nearest even: overflow to Inf, gradual underflow through the fp16
    subnormals.  Controls: 'trunc' drops the discarded bits, 'ftz' returns a signed zero where the result is
    subnormal."""
    u = np.asarray(u, np.uint32).astype(np.int64)
    sign = (u >> 16) & 0x8000
    e = (u >> 23) & 0xFF
    m = u & 0x7FFFFF
    e16 = e - 127 + 15
    mant = np.where(e > 0, m | 0x800000, 0)                      # an f32 subnormal is far below half an fp16 ulp
    shift = np.clip(np.where(e16 > 0, 13, 14 - e16), 13, 40)     # subnormal result: the exponent becomes a shift
    kept = mant >> shift
    rem = mant & ((np.int64(1) << shift) - 1)
    half = np.int64(1) << (shift - 1)
    up = (rem > half) | ((rem == half) & (kept & 1 == 1))
    if mode == "trunc":
        up = np.zeros_like(up)
    body = np.where(e16 > 0, (e16 << 10) + (kept & 0x3FF), kept) + up        # a carry moves into the exponent
    body = np.minimum(body, 0x7C00)                                              # overflow -> Inf
    if mode == "ftz":
        body = np.where(body < 0x0400, 0, body)
    nan = (e == 0xFF) & (m != 0)
    inf = (e == 0xFF) & (m == 0)
    body = np.where(inf, 0x7C00, np.where(nan, 0x7E00 | (m >> 13), body))
    return (sign | body).astype(np.uint16)


def operand_bits(bits, dt, precision, mode="rne"):
    """uint32 f32 patterns of what a GEMM of `precision` ('fp32' / 'fp16' / 'bf16') multiplies for store elements
    `bits` of type dt: the widening (fp32), or the widening rounded once to the operand type and widened again."""
    w = widen(bits, dt)
    if precision == "fp32":
        return w
    if precision == "fp16":
        return widen_f16(f32_to_f16_bits(w, mode))
    return widen_bf16(f32_to_bf16_bits(w, mode))


def finite32(u):
    return (np.asarray(u, np.uint32) >> np.uint32(23)) & np.uint32(0xFF) != 0xFF


def is_nan16(bits, dt):
    b = np.asarray(bits, np.uint16)
    if dt == "f16":
        return (b & 0x7C00 == 0x7C00) & (b & 0x03FF != 0)
    return (b & 0x7F80 == 0x7F80) & (b & 0x007F != 0)


def is_subnormal16(bits, dt):
    b = np.asarray(bits, np.uint16)
    if dt == "f16":
        return (b & 0x7C00 == 0) & (b & 0x03FF != 0)
    return (b & 0x7F80 == 0) & (b & 0x007F != 0)


# ---- 1. every 16-bit pattern ---------------------------------------------------------------------------------------------
PATTERN_FRAMES = 1024


@functools.lru_cache(None)
def pattern_store():
    """uint16 [1024][768]: pattern (96 f + c // 8 + 8191 (c mod 8)) mod 65536 at frame f, column c, so that every
    pattern occurs at every column residue c mod 8 (all_patterns_at_every_residue)."""
    f = np.arange(PATTERN_FRAMES, dtype=np.int64)[:, None]
    c = np.arange(DIM, dtype=np.int64)[None, :]
    out = ((96 * f + c // 8 + 8191 * (c % 8)) % 65536).astype(np.uint16)
    out.setflags(write=False)
    return out


def all_patterns_at_every_residue(bits, keep=None):
    """Every pattern (of `keep`, a bool [65536]; default all) occurs in `bits` at every column residue mod 8."""
    keep = np.ones(65536, bool) if keep is None else keep
    for r in range(8):
        seen = np.zeros(65536, bool)
        seen[bits[:, r::8].reshape(-1)] = True
        if not seen[keep].all():
            return False
    return True


def pattern_layout():
    """(sizes, offsets) that cut the 1024 frames into utterances, lengths 1, 2 and 33 among them, and the batches
    (lists of utterance indices, B <= 64) that cover them all."""
    lens = [1, 2, 33, 7, 64, 1, 31, 32, 100, 2, 33, 129, 1, 256, 300]
    sizes = lens + [PATTERN_FRAMES - sum(lens)]
    assert sizes[-1] > 0
    sizes = np.array(sizes, np.int64)
    offsets = np.concatenate([[0], np.cumsum(sizes)[:-1]]).astype(np.int64)
    batches = [[0, 1, 2], [3, 4, 5, 6, 7], [8, 9, 10, 11, 12], [13], [14, 15]]
    return sizes, offsets, batches


# ---- 3. the read-out network -----------------------------------------------------------------------------------------------
ONE = {"f16": 0x3C00, "bf16": 0x3F80}
READOUT = tuple((g, s) for g in range(3) for s in (1.0, -1.0))     # six checkpoints: column group, sign


def probe_store(dt, precision, limit=None):
    """(bits uint16 [1024][768], covered bool [1024][768]) for store type dt ('f16' / 'bf16') read at `precision`:
    pattern_store() with every pattern that is not finite, or whose operand conversion is not finite, replaced by
    1.0 (a 0 weight times an Inf operand would make every embedding of the row a NaN).  limit: patterns of magnitude
    above it leave as well (the train step's probe: 256, so that every loss stays finite).  covered marks the
    elements that kept their pattern."""
    bits = pattern_store().copy()
    wide, ops = widen(bits, dt), operand_bits(bits, dt, precision)
    ok = finite32(wide) & finite32(ops)
    if limit is not None:
        top = np.float32(limit).view(np.uint32)
        ok &= (wide & np.uint32(0x7FFFFFFF) <= top) & (ops & np.uint32(0x7FFFFFFF) <= top)
    bits[~ok] = ONE[dt]
    return bits, ok


def probe_f32(precision, limit=None):
    """The f32 probe store: the widened fp16 probe (uint32 patterns) and its covered mask."""
    bits, ok = probe_store("f16", precision, limit)
    return widen_f16(bits), ok


def probe(dt, precision, limit=None):
    """(store elements in their own type: uint16 or uint32 patterns, operands uint32, covered) of one probe case."""
    if dt == "f32":
        bits, ok = probe_f32(precision, limit)
    else:
        bits, ok = probe_store(dt, precision, limit)
    return bits, operand_bits(bits, dt, precision), ok


def subnormal_operand(ops, precision):
    """Operands (uint32 f32 patterns) that are subnormal in the type the GEMM of `precision` multiplies."""
    mag = np.asarray(ops, np.uint32) & np.uint32(0x7FFFFFFF)
    floor = {"fp32": 0x00800000, "bf16": 0x00800000, "fp16": 0x38800000}[precision]     # the smallest normal
    return (mag != 0) & (mag < np.uint32(floor))


def readout_params(group, sign):
    """(W1, b1, W2, b2): hidden unit h reads column 256 group + h with weight sign; b1 = 0, W2 = 0, b2 fixed."""
    W1 = np.zeros((256, DIM), np.float32)
    W1[np.arange(256), 256 * group + np.arange(256)] = sign
    return W1, np.zeros(256, np.float32), np.zeros((4, 256), np.float32), np.array([0.5, -1.0, 2.0, 0.25], np.float32)


def readout_expected(operands, group, sign):
    """uint32 [frames][256]: relu(sign * x[256 group + h]) of one-frame utterances, bit for bit: the operand (sign
    flipped for -1) where that is positive, +0 elsewhere."""
    x = np.asarray(operands, np.uint32)[:, 256 * group:256 * (group + 1)]
    if sign < 0:
        x = x ^ np.uint32(0x80000000)
    positive = (x >> np.uint32(31) == 0) & (x != 0)
    return np.where(positive, x, np.uint32(0))


# ---- 0. the contract's references -------------------------------------------------------------------------------------------
def _valid(index, n_samples):
    index = np.asarray(index, np.int64).reshape(-1)
    return index, (index >= 0) & (index < n_samples)


def ref_collate(wide, sizes, offsets, labels, index, T):
    """dad_collate by include/dad.h: feats uint32 [B][T][768] (the widened store patterns `wide`, zeros past each
    size), pad uint8 [B][T] (1 for t >= size), labels int64 [B] copied verbatim or None.  An index outside
    [0, n_samples) is an all-padding row with label -1; a sample of size 0 is all padding."""
    index, ok = _valid(index, len(sizes))
    B = len(index)
    feats = np.zeros((B, T, DIM), np.uint32)
    pad = np.ones((B, T), np.uint8)
    lab = None if labels is None else np.full(B, -1, np.int64)
    for b in range(B):
        if not ok[b]:
            continue
        s = int(index[b])
        n = int(sizes[s])
        assert n <= T, "the contract: T >= max(sizes[index])"
        if n:
            feats[b, :n] = wide[int(offsets[s]):int(offsets[s]) + n]
        pad[b, :n] = 0
        if lab is not None:
            lab[b] = labels[s]
    return {"feats": feats, "pad": pad, "labels": lab}


def ref_collate_index(sizes, offsets, labels, index, T, mutate=None):
    """dad_collate_index: rows int64 [B] = offsets[s] (0 when the sample is empty or the index out of range), lens
    int32 [B] = the size or 0, pad and labels as ref_collate's.  mutate: a wrong-answer control, 'pad_off_by_one'
    (t <= size) or 'row_kept' (the row base of an empty sample not zeroed)."""
    index, ok = _valid(index, len(sizes))
    B = len(index)
    rows = np.zeros(B, np.int64)
    lens = np.zeros(B, np.int32)
    pad = np.ones((B, T), np.uint8)
    lab = None if labels is None else np.full(B, -1, np.int64)
    for b in range(B):
        if not ok[b]:
            continue
        s = int(index[b])
        n = int(sizes[s])
        lens[b] = n
        rows[b] = offsets[s] if (n > 0 or mutate == "row_kept") else 0
        pad[b, :min(T, n + 1 if mutate == "pad_off_by_one" else n)] = 0
        if lab is not None:
            lab[b] = labels[s]
    return {"rows": rows, "lens": lens, "pad": pad, "labels": lab}


def epoch_layout(sizes, batches, Ts=None):
    """(flat index, pad_off [n], pad_T [n], T per batch) of an epoch: batch k's T is Ts[k], or its longest valid
    sample; sample i's pad row follows the previous sample's."""
    n_samples = len(sizes)
    flat, pad_T, Tk = [], [], []
    for k, b in enumerate(batches):
        b, ok = _valid(b, n_samples)
        T = int(Ts[k]) if Ts is not None else int(max([int(sizes[s]) for s in b[ok]] + [0]))
        Tk.append(T)
        flat.extend(int(x) for x in b)
        pad_T.extend([T] * len(b))
    pad_T = np.array(pad_T, np.int64)
    pad_off = np.concatenate([[0], np.cumsum(pad_T)[:-1]]).astype(np.int64)
    return np.array(flat, np.int64), pad_off, pad_T, Tk


def ref_collate_index_epoch(sizes, offsets, labels, batches, Ts=None, mutate=None):
    """dad_collate_index_epoch: per sample the values dad_collate_index writes, for every batch of the epoch; pad is
    the concatenation of the batches' [B_k][T_k] masks.  Builds pad_off and pad_T itself (epoch_layout)."""
    flat, pad_off, pad_T, Tk = epoch_layout(sizes, batches, Ts)
    parts = [ref_collate_index(sizes, offsets, labels, b, T, mutate) for b, T in zip(batches, Tk)]
    cat = lambda k: np.concatenate([p[k].reshape(-1) for p in parts])
    return {"index": flat, "pad_off": pad_off, "pad_T": pad_T, "T": Tk, "rows": cat("rows"), "lens": cat("lens"),
            "pad": cat("pad"), "labels": None if labels is None else cat("labels"), "batches": parts}


# ---- 2. the edge store ----------------------------------------------------------------------------------------------------
EDGE_SIZES = (3, 0, 1, 7, 2, 9, 1, 8, 300, 5, 1, 2, 3, 257, 256, 513, 255, 0)
EDGE_LABELS = (0, 1, 2, 3, -1, 9, 3, 2, 1, 0, 0, 1, 2, 3, 9, -1, 2, 1)
COLLATE_SHAPES = ((1, 1), (1, 2), (3, 3), (1, 7), (1, 8), (1, 9), (5, 7), (257, 1), (513, 2), (2, 300))
INDEX_SHAPES = ((5, 51), (16, 16), (1, 257), (257, 1), (19, 27), (3, 85), (7, 1), (2, 300))   # B T = 255, 256, 257, 513, ..
OUT_OF_RANGE = (-1, None, 2 ** 40, INT64_MIN)        # None: n_samples itself


def edge_values(frame, col):
    """Exact small integers in [-125, 125] (an fp16, bf16 and f32 value alike), a function of (frame, column)."""
    return ((np.asarray(frame, np.int64) * 7 + np.asarray(col, np.int64) * 3) % 251 - 125).astype(np.float32)


@functools.lru_cache(None)
def edge_store():
    """(feats f32 [frames][768], sizes, offsets, labels): sizes 0, 1 and up to 513; an empty sample between two others
    (index 1) and one whose offset is the store's frame count (the last); two unrelated frames before each utterance;
    labels -1 and 9 among 0 .. 3."""
    sizes = np.array(EDGE_SIZES, np.int64)
    offsets, row = [], 0
    for n in sizes:
        row += 2 if n else 0
        offsets.append(row)
        row += int(n)
    frames = row
    offsets = np.array(offsets, np.int64)
    assert sizes[-1] == 0 and offsets[-1] == frames and sizes[1] == 0
    feats = edge_values(np.arange(frames)[:, None], np.arange(DIM)[None, :])
    for a in (feats, sizes, offsets):
        a.setflags(write=False)
    return feats, sizes, offsets, np.array(EDGE_LABELS, np.int64)


def edge_subset():
    """Indices of a subset with duplicates (utterances that share frames), the empty samples kept."""
    return np.array([3, 3, 0, 17, 5, 1, 5, 8, 2, 3, 10, 6, 14], np.int64)


def edge_index(sizes, B, T, cap=None):
    """B sample indices for padded length T: the samples of size <= cap (default T) in a fixed stride, a sample of
    size == T first when there is one; an index repeats as soon as B exceeds the candidates (and at B >= 3 always)."""
    sizes = np.asarray(sizes)
    cap = T if cap is None else cap
    cand = [int(i) for i in np.flatnonzero(sizes <= cap)]
    assert cand
    full = [i for i in cand if sizes[i] == cap]
    out = full[:1] + [cand[(3 * k + 1) % len(cand)] for k in range(B)]
    out = out[:B]
    if B >= 3:
        out[-1] = out[0]
    return np.array(out, np.int64)


def with_out_of_range(index, n_samples):
    """The index with -1, n_samples, 2^40 and INT64_MIN mixed in between the valid entries."""
    bad = [n_samples if v is None else v for v in OUT_OF_RANGE]
    out = []
    for k, v in enumerate(np.asarray(index).tolist()):
        out.append(v)
        if k < len(bad):
            out.append(bad[k])
    return np.array(out + bad[len(index):], np.int64)


EPOCH_TS = (1, 255, 256, 257, 513)


def edge_epoch(n_samples=None):
    """The batches of the C-ABI epoch over edge_store(): T of 1, 255, 256, 257 and 513 (the pad loop's first, second
    and third trip), an empty sample inside a batch with T > 0, out-of-range indices, and a last batch of one sample."""
    _, sizes, _, _ = edge_store()
    n = len(sizes) if n_samples is None else n_samples
    by = lambda T: int(np.flatnonzero(sizes == T)[0])
    return [[by(1), 1, 6], [by(255), 17, -1, 3], [by(256), n, 0], [2 ** 40, by(257), 1, 3], [by(513), INT64_MIN, 13],
            [by(255), 16], [4]]


LOADER_SIZES = (256, 257, 513, 1, 40, 255, 2, 33, 7, 300, 64)


# ---- 4. stores past 2^31 elements and 2^32 bytes ---------------------------------------------------------------------------
BIG = {"f16": {"frames": 2796400, "boundary": 2796202, "column": 512, "wrap": 2 ** 31, "unit": "elements"},
       "f32": {"frames": 1398300, "boundary": 1398101, "column": 256, "wrap": 2 ** 32, "unit": "bytes"}}


def big_values(frame, col):
    """Values on the 2^-3 grid in [-31.75, 31.75], a function of (frame, column); exact in fp16 and f32."""
    return (((np.asarray(frame, np.int64) * 31 + np.asarray(col, np.int64) * 7) % 509 - 254) / 8.0).astype(np.float32)


def big_layout(dt):
    """(sizes, offsets) of the utterances written into the big store of type dt: two below the boundary frame, one
    straddling it (the boundary element falls inside one of its rows), two wholly above."""
    fb = BIG[dt]["boundary"]
    offsets = np.array([5, fb - 40, fb - 2, fb + 7, fb + 150], np.int64)
    sizes = np.array([3, 33, 5, 2, 33], np.int64)
    assert (offsets + sizes).max() <= BIG[dt]["frames"]
    assert BIG[dt]["boundary"] * DIM * (1 if dt == "f16" else 4) + BIG[dt]["column"] * (1 if dt == "f16" else 4) \
        == BIG[dt]["wrap"]
    return sizes, offsets


def big_rows(dt, k):
    """The right rows of utterance k: f32 [size][768]."""
    sizes, offsets = big_layout(dt)
    return big_values(np.arange(offsets[k], offsets[k] + sizes[k])[:, None], np.arange(DIM)[None, :])


def big_rows_wrapped(dt, k):
    """Utterance k's rows as a gather would return them whose element index (16-bit store) is taken mod 2^31, or whose
    byte offset (f32 store) mod 2^32: the store holds big_values inside the utterances and 0 elsewhere."""
    sizes, offsets = big_layout(dt)
    width = 1 if dt == "f16" else 4
    el = (np.arange(offsets[k], offsets[k] + sizes[k], dtype=np.int64)[:, None] * DIM + np.arange(DIM)[None, :]) * width
    el = (el % BIG[dt]["wrap"]) // width
    frame, col = el // DIM, el % DIM
    inside = np.zeros(frame.shape, bool)
    for o, n in zip(offsets, sizes):
        inside |= (frame >= o) & (frame < o + n)
    return np.where(inside, big_values(frame, col), np.float32(0))


def compact_layout(dt):
    """(sizes, offsets, frames) of the compact store that holds copies of the same utterances."""
    sizes, _ = big_layout(dt)
    offsets, row = [], 1
    for n in sizes:
        offsets.append(row)
        row += int(n) + 2
    return sizes, np.array(offsets, np.int64), row
