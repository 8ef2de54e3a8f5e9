"""The inputs the GPU tests of dad_rank_metrics run (tests/test_gpu_rank.py) and the comparison they make with
tests/rank_ref.py, kept apart so that the CPU suite can hold the list to the wrong-answer controls of rank_ref.WRONG:
each control must fail compare() on at least one case, or the list is too weak (tests/test_rank_ref_cpu.py)."""
import functools

import numpy as np

import rank_ref

# (n, m): the wave, tile and chunk edges; 4097 gives 17 row tiles and up to 8 chunks
SHAPES = ((1, 1), (2, 1), (63, 16), (64, 1), (65, 10), (255, 10), (256, 16), (257, 10), (1100, 10), (4097, 16))
PATTERNS = ("continuous", "levels3", "levels7", "all_equal", "zeros", "nonfinite", "empty", "one_member",
            "all_positive", "all_negative")
GAMMAS = (0.0, 0.4, 0.5, 0.613, 0.8, 1.0, 0.25, 0.99)
BIN_RANGE = (0.25, 0.75)     # the level patterns hold keys exactly on 0.25 and 0.75 and outside the range


def _column(pattern, n, rs):
    member = rs.random_sample(n) < 0.9
    positive = rs.random_sample(n) < 0.4
    key = rs.random_sample(n).astype(np.float32)
    if pattern == "levels3":
        key = np.array([0.25, 0.5, 0.75], np.float32)[rs.randint(0, 3, n)]
    elif pattern == "levels7":
        key = (rs.randint(1, 8, n) / 8.0).astype(np.float32)
    elif pattern == "all_equal":
        key = np.full(n, 0.625, np.float32)
    elif pattern == "zeros":
        key = np.array([-0.0, 0.0, 0.5, -0.5], np.float32)[rs.randint(0, 4, n)]
    elif pattern == "nonfinite":
        key[rs.random_sample(n) < 0.2] = np.nan
        key[rs.random_sample(n) < 0.1] = np.inf
        key[rs.random_sample(n) < 0.1] = -np.inf
    elif pattern == "empty":
        member[:] = False
    elif pattern == "one_member":
        member[:] = False
        member[rs.randint(0, n)] = True
    elif pattern == "all_positive":
        positive[:] = True
    elif pattern == "all_negative":
        positive[:] = False
    return key, (member * rank_ref.MEMBER + positive * rank_ref.POSITIVE).astype(np.uint8)


def _threshold(kind, key, flags):
    live = key[((flags & rank_ref.MEMBER) != 0) & np.isfinite(key)]
    if kind == 1 or len(live) == 0:
        return np.float32(np.nan)
    if kind == 0:
        return np.sort(live)[len(live) // 2]          # an existing key
    return np.float32(live.max() + 1.0) if kind == 2 else np.float32(live.min() - 1.0)


@functools.lru_cache(None)
def case(index):
    """{'name', 'key' [m][n], 'flags' [m][n], 'thr' [m], 'gammas', 'bins', 'bin_range'} of SHAPES[index], from its
    seed; never modified."""
    n, m = SHAPES[index]
    rs = np.random.RandomState(4100 + index)
    cols = [_column(PATTERNS[(index + j) % len(PATTERNS)], n, rs) for j in range(m)]
    key, flags = np.stack([c[0] for c in cols]), np.stack([c[1] for c in cols])
    thr = np.array([_threshold((index + j) % 4, key[j], flags[j]) for j in range(m)], np.float32)
    return {"name": "n%d_m%d" % (n, m), "key": key, "flags": flags, "thr": thr,
            "gammas": () if index % 3 == 1 else GAMMAS, "bins": (64, 0, 1)[index % 3], "bin_range": BIN_RANGE}


@functools.lru_cache(None)
def reference(index, variant=""):
    c = case(index)
    return rank_ref.rank_metrics(c["key"], c["flags"], c["thr"], c["gammas"], c["bins"], c["bin_range"], variant)


def compare(got, ref, curves=True):
    """What the GPU tests hold a result to: integers and the float32 quantiles equal, each double within the bound of
    a sum in any order.  Returns (the list of what differs, the worst ratio of a double's error to its bound)."""
    bad = []
    for name in (("order", "cum_pos", "tie_end") if curves else ()) + ("counts", "bin_counts"):
        if not np.array_equal(got[name], ref[name]):
            bad.append(name)
    q, r = np.asarray(got["quant"], np.float32), np.asarray(ref["quant"], np.float32)
    if q.shape != r.shape or not np.array_equal(np.isnan(q), np.isnan(r)) or \
            not np.array_equal(q[~np.isnan(q)].view(np.uint32), r[~np.isnan(r)].view(np.uint32)):
        bad.append("quant")
    worst = 0.0
    for name, bound in (("values", rank_ref.value_bound(ref)), ("bin_sum", rank_ref.bin_bound(ref))):
        err = np.abs(np.asarray(got[name], np.float64) - ref[name])
        if not np.all(err <= bound):
            bad.append(name)
        with np.errstate(divide="ignore", invalid="ignore"):
            ratio = np.where(bound > 0, err / bound, 0.0)
        worst = max(worst, float(ratio.max()) if ratio.size else 0.0)
    return bad, worst
