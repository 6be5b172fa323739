"""Seeded cases of the descriptor-track micro-AP (tests/uap_contract.py, csrc/uap.hip, vsc_hip/uap.py).  Only what the REFERENCE
returns on them is committed (tests/golden/uap_device.json, written by tests/golden/gen_uap_device_golden.py); the cases themselves
are rebuilt from their seeds.

A case is a dict: name; scores float64 [n] (float32 values widened, as CandidatePair.score holds them); pq / pr int64 [n] and
gq / gr int64 [g], the interned query / reference indices of the predictions and of the ground truth; ref_bits and key_bits of the
64-bit key pq << ref_bits | pr; refusal (None, or what is wrong with the case)."""
import functools

import numpy as np

TILE = 2048                                           # VSC_UAP_TILE
SIZES = (0, 1, 7, 8, 9, 127, 128, 129, 255, 256, 257, 1000, TILE - 1, TILE, TILE + 1, 2500, 3 * TILE + 5)
BIG = "big_200000x8000"
EMULATED_MAX = 2500                                   # the emulation runs one OS thread per GPU thread


def _scores(rng, n, ties, planted):
    if ties == "one":
        s = np.full(n, -0.37, np.float32)
    elif ties:
        levels = ((np.arange(max(n // 3, 1)) - n // 6) * 3e-3).astype(np.float32)      # about n / 3 groups, negative ones included
        s = levels[rng.integers(0, len(levels), n)]
    else:
        s = rng.permutation(((np.arange(n) - n // 2) * 1e-3).astype(np.float32))          # all distinct, half of them negative
    if planted and n >= 9:
        x = np.float32(0.41)
        s = s.copy()
        at = rng.permutation(n)[:8]
        s[at] = [-0.0, 0.0, 1e-45, -1e-45, x, np.nextafter(x, np.float32(1)), 3e-39, 0.0]   # zeros of both signs, denormals, one ulp apart
    return s.astype(np.float64)


def make(name, n, g_hit, g_miss, ties=False, seed=0, wide=False, planted=True):
    rng = np.random.default_rng([seed, n, g_hit, g_miss])
    pool = rng.choice(1 << 20, n + g_miss, replace=False).astype(np.int64)     # distinct (q, r) with q, r < 1024
    q, r = pool >> 10, pool & 1023
    if wide:                                                                   # indices up to 2^32 - 1: all 64 key bits in use
        q, r = (1 << 32) - 1 - q, (1 << 32) - 1 - r
    hit = rng.choice(n, g_hit, replace=False) if g_hit else np.zeros(0, np.int64)
    gsel = rng.permutation(np.r_[hit, n + np.arange(g_miss)].astype(np.int64))
    case = dict(name=name, scores=_scores(rng, n, ties, planted), pq=q[:n].copy(), pr=r[:n].copy(), gq=q[gsel], gr=r[gsel],
                ref_bits=32 if wide else 10, key_bits=64 if wide else 20, refusal=None)
    return case


def _freeze(case):
    for v in case.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return case


@functools.lru_cache(maxsize=None)
def cases(with_big=True):
    out = []
    for n in SIZES:
        for ties in (False, True):
            out.append(make(f"n{n}_{'ties' if ties else 'distinct'}", n, max(n // 5, min(n, 1)), 3, ties, seed=1))
    out.append(make("one_group", 300, 40, 2, "one", seed=2))
    out.append(make("fully_predicted", 257, 60, 0, True, seed=3))
    out.append(make("disjoint", 129, 0, 5, True, seed=4))                      # n_pos = 0
    out.append(make("g1_hit", 9, 1, 0, False, seed=5))
    out.append(make("g1_missed", 9, 0, 1, True, seed=6))
    out.append(make("all_correct", 130, 130, 0, True, seed=7))
    out.append(make("wide_keys_ties", 1000, 200, 7, True, seed=8, wide=True))
    out.append(make("wide_keys_distinct", 129, 30, 2, False, seed=9, wide=True))
    if with_big:
        out.append(make(BIG, 200000, 6000, 2000, True, seed=10))
    # what the reference refuses
    c = make("refuse_nan", 40, 8, 2, False, seed=11)
    c["scores"][17] = np.nan
    c["refusal"] = "nan"
    out.append(c)
    c = make("refuse_inf", 40, 8, 2, False, seed=12)
    c["scores"][3] = np.inf
    c["refusal"] = "inf"
    out.append(c)
    c = make("refuse_duplicate_prediction", 40, 8, 2, True, seed=13)
    c["pq"][31], c["pr"][31] = c["pq"][5], c["pr"][5]
    c["refusal"] = "duplicate prediction"
    out.append(c)
    c = make("refuse_duplicate_ground_truth", 40, 8, 2, True, seed=14)
    c["gq"][9], c["gr"][9] = c["gq"][0], c["gr"][0]
    c["refusal"] = "duplicate ground truth"
    out.append(c)
    c = make("refuse_empty_ground_truth", 40, 0, 0, True, seed=15)
    c["refusal"] = "empty ground truth"
    out.append(c)
    return tuple(_freeze(c) for c in out)


def names(max_n=None, refusals=True):
    return [c["name"] for c in cases() if (max_n is None or len(c["scores"]) <= max_n) and (refusals or c["refusal"] is None)]


def get(name):
    return next(c for c in cases() if c["name"] == name)


def keys(case):
    """-> (pred_keys, gt_keys) uint64"""
    sh = np.uint64(case["ref_bits"])
    return ((case["pq"].astype(np.uint64) << sh) | case["pr"].astype(np.uint64),
            (case["gq"].astype(np.uint64) << sh) | case["gr"].astype(np.uint64))


def pairs(case, cls):
    """-> (ground truth, predictions) as lists of cls(query_id, ref_id, score) with the video ids the reference formats"""
    gt = [cls(f"Q{q:06d}", f"R{r:06d}", 1.0) for q, r in zip(case["gq"].tolist(), case["gr"].tolist())]
    preds = [cls(f"Q{q:06d}", f"R{r:06d}", s) for q, r, s in zip(case["pq"].tolist(), case["pr"].tolist(), case["scores"].tolist())]
    return gt, preds
