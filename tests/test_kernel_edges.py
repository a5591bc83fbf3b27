"""Edge shapes of the pair, slab, threshold, compaction and recommendation kernels.

The other kernel tests feed generator output and compare the device with the project's
own C++ path, so the generator decides which kernel branches run.  Here every input is
built on purpose from a dense 0/1 matrix B[T, F1] (int64, seeded where random) to reach
one branch each -- the unstaged and mixed-staging paths of k_pair_queue16 and its u16
counter bound, k_pair_blocked's staging limit, the slab kernel's widths / long prefixes /
piece sizes / bitmap-copy build, the block kernels of the bundle threshold and F2
compaction, the recommendation kernels' rule steps and list breaks -- and the expected
result comes from B in numpy, never from another path of this project.  All values are
integers and every comparison is exact equality over the whole output.

Ops with a CPU path run on "cpu" too: that proves the builders and the references where
there is no GPU, and checks the C++ path by brute force.
"""
import functools
import math

import numpy as np
import pytest
import torch

from fastapriori_amd import ops
from fastapriori_amd.ops import primitives as prim

DEV = torch.device("cuda", 0)
BOTH = ["cpu", pytest.param("cuda", marks=pytest.mark.gpu)]
GPU = [pytest.param("cuda", marks=pytest.mark.gpu)]


# ---------------------------------------------------------------------------
# builders and references
# ---------------------------------------------------------------------------
def _csr(B):
    """Dense 0/1 rows -> (roff int64 [T + 1], ranks int32, ascending in each row)."""
    roff = np.zeros(B.shape[0] + 1, np.int64)
    np.cumsum(B.sum(1), out=roff[1:])
    return torch.from_numpy(roff), torch.from_numpy(np.nonzero(B)[1].astype(np.int32))


def _rows_to_dense(rows, F1):
    B = np.zeros((len(rows), F1), np.int64)
    for x, r in enumerate(rows):
        B[x, r] = 1
    return B


def _gram(B, w=None):
    """Upper triangle of B.T @ diag(w) @ B, int64.  The product runs in float64 (BLAS):
    every entry is an integer below 2^53, so it is exact."""
    A = B.astype(np.float64)
    L = A.T if w is None else A.T * np.asarray(w, np.float64)
    G = np.rint(L @ A).astype(np.int64)
    assert G.max(initial=0) < 1 << 53
    return np.triu(G, 1)


def _pick(rng, lo, hi, n):
    """n distinct ranks of [lo, hi)."""
    return rng.choice(np.arange(lo, hi), n, replace=False)


def _rows_of_lengths(rng, lens, lo, hi):
    return [_pick(rng, lo, hi, int(n)) for n in lens]


def _batch_lengths(rng, total, base):
    """64 row lengths of base - 1 .. base + 1 summing to total (|total - 64 base| <= 64)."""
    lens = np.full(64, base)
    d = total - 64 * base
    lens[rng.choice(64, abs(d), replace=False)] += int(np.sign(d))
    assert lens.sum() == total
    return lens


def _pairs(B, F1, dev, wrow=None, **kw):
    roff, ranks = _csr(B)
    w = None if wrow is None else torch.from_numpy(np.asarray(wrow, np.int32)).to(dev)
    got = ops.pair_counts_horizontal(roff.to(dev), ranks.to(dev), w, F1, **kw)
    assert got.shape == (F1, F1) and got.dtype == torch.int64
    return got.cpu().numpy()


# ---------------------------------------------------------------------------
# 1. unit-weight pairs: k_pair_queue16 (256-rank blocks, packed-u16 tile)
# ---------------------------------------------------------------------------
def _unit_full_rows():
    # 254 items per row (the longest row the 256-block layout admits): 16256 B per batch,
    # unstaged, diagonal tile; the last batch holds 2 rows
    B = np.zeros((130, 256), np.int64)
    B[:, :254] = 1
    return B


def _unit_long_row_sparse_batch():
    # 254 + 63 * 2 = 380 B: a staged flat batch whose row 0 has c = 254 > 64 items, so its
    # 32131 pairs go through the square-root decode
    rng = np.random.default_rng(101)
    return _rows_to_dense([np.arange(254)] + _rows_of_lengths(rng, [2] * 63, 0, 256), 256)


def _unit_staging_boundary():
    # one block; batch totals around kRowsStage = 512 with segment starts off a dword:
    # starts 0, 509, 1019, 1530, 2042, 2555 -> misalignment 0, 1, 3, 2, 2, 3
    rng = np.random.default_rng(102)
    rows = []
    for total in (509, 510, 511, 512, 513, 512):
        rows += _rows_of_lengths(rng, _batch_lengths(rng, total, 8), 0, 256)
    B = _rows_to_dense(rows, 256)
    assert B.shape[0] == 384 and set(B.sum(1)) <= {7, 8, 9}
    assert [int(B[64 * q:64 * q + 64].sum()) for q in range(6)] == [509, 510, 511, 512, 513, 512]
    return B


def _unit_mixed_staging():
    # tile (0, 1): one block's segment staged (64 * 7 = 448 B), the other not (64 * 9 = 576 B),
    # both ways round
    rng = np.random.default_rng(103)
    rows = []
    for n0, n1 in [(7, 9), (7, 9), (9, 7), (9, 7)]:
        for _ in range(64):
            rows.append(np.concatenate([_pick(rng, 0, 256, n0), _pick(rng, 256, 512, n1)]))
    B = _rows_to_dense(rows, 512)
    assert int(B[:64, :256].sum()) == 448 and int(B[:64, 256:].sum()) == 576
    assert int(B[128:192, :256].sum()) == 576 and int(B[128:192, 256:].sum()) == 448
    return B


def _unit_odd_f1():
    # F1 odd: odd row stride -> the u32 flush; block 1 holds the single rank 256
    rng = np.random.default_rng(104)
    return _rows_to_dense([np.concatenate([_pick(rng, 0, 256, 3), [256]]) for _ in range(100)], 257)


def _unit_minimal():
    return np.ones((1, 2), np.int64)


UNIT_CASES = {
    "full_rows": _unit_full_rows,
    "long_row_in_sparse_batch": _unit_long_row_sparse_batch,
    "staging_boundary": _unit_staging_boundary,
    "mixed_staging": _unit_mixed_staging,
    "odd_F1": _unit_odd_f1,
    "minimal": _unit_minimal,
}


@pytest.mark.parametrize("dev", BOTH)
@pytest.mark.parametrize("case", list(UNIT_CASES))
def test_pairs_unit_weight(native, case, dev):
    B = UNIT_CASES[case]()
    F1 = B.shape[1]
    got = _pairs(B, F1, dev, long_rows=False)
    assert np.array_equal(got, _gram(B))


def _saturated():
    # two sub-chunks of kQSubB = 511 batches (32704 rows) and 65 rows more; every row holds
    # the same 4 items, so each of the 6 pairs gains 32704 per sub-chunk: a workgroup that
    # keeps its tile has counters at 32704, then 65408 (drained to 32640), then 32705
    T = 2 * 32704 + 65
    B = np.zeros((T, 258), np.int64)
    B[:, [0, 1, 256, 257]] = 1
    ref = _gram(B)
    assert ref.sum() == 6 * T and set(ref[ref > 0]) == {T}
    return B, ref


@pytest.mark.parametrize("dev", BOTH)
@pytest.mark.parametrize("pair_wg", [1, None])
def test_pairs_saturated_counters(native, tune, pair_wg, dev):
    # pair_wg = 1: one workgroup walks all three sub-chunks of each tile in turn, so the
    # counters of a kept tile reach 32704 + 32704; the default leaves the schedule to the queue
    B, ref = _saturated()
    if pair_wg is not None:
        tune(pair_wg=pair_wg)
    got = _pairs(B, 258, dev, long_rows=False)
    assert np.array_equal(got, ref)


# ---------------------------------------------------------------------------
# 2. blocked / weighted pairs: k_pair_blocked (128-rank blocks, kBSpan = 1024 staged bytes)
# ---------------------------------------------------------------------------
def _blocked_full_128():
    return np.ones((70, 128), np.int64), [None, np.ones(70, np.int32)]


def _blocked_full_300():
    # blocks of 128, 128 and 44 ranks; two batches (64 + 1 rows); weights with zeros
    return np.ones((65, 300), np.int64), [np.array([0, 1, 5], np.int32)[np.arange(65) % 3]]


def _blocked_staging_boundary():
    rng = np.random.default_rng(201)
    rows = []
    for total in (1023, 1024, 1025):
        rows += _rows_of_lengths(rng, _batch_lengths(rng, total, 16), 0, 128)
    B = _rows_to_dense(rows, 128)
    assert [int(B[64 * q:64 * q + 64].sum()) for q in range(3)] == [1023, 1024, 1025]
    return B, [None, rng.integers(0, 4, 192).astype(np.int32)]


BLOCKED_CASES = {
    "full_rows_128": _blocked_full_128,
    "full_rows_300_weights_0_1_5": _blocked_full_300,
    "staging_boundary": _blocked_staging_boundary,
}


@pytest.mark.parametrize("dev", BOTH)
@pytest.mark.parametrize("case", list(BLOCKED_CASES))
def test_pairs_blocked(native, case, dev):
    B, weights = BLOCKED_CASES[case]()
    F1 = B.shape[1]
    for w in weights:
        got = _pairs(B, F1, dev, wrow=w)          # long_rows=True: 128-rank blocks either way
        assert np.array_equal(got, _gram(B, w)), "unit rows" if w is None else "weighted rows"


# ---------------------------------------------------------------------------
# 3. slab level kernel: k_count_slab_rec through count_level
# ---------------------------------------------------------------------------
EXT_SIZES = (1, 7, 8, 9, 16, 17)     # pieces hold <= 8 extensions: 1 piece, 1, 1, 2, 2, 3


def _slab_rows(rng, T, F1):
    B = (rng.random((T, F1)) < 0.3).astype(np.int64)
    B[np.arange(T) % 10 < 3] = 1          # 30 % planted full rows: long prefixes have support
    B[B.sum(1) < 2, :2] = 1               # the kernels rely on rows of >= 2 items
    return B


def _candidates(rng, pool, m, G):
    """Candidates in apriori_gen's form over the item pool: G distinct prefixes of m ids in
    lexicographic order, group g with EXT_SIZES[g % 6] ascending extensions above its
    prefix's last id."""
    pool = np.sort(np.asarray(pool))
    low = pool[:pool.size - max(EXT_SIZES)]
    assert math.comb(low.size, m) >= 2 * G
    seen = set()
    while len(seen) < G:
        seen.add(tuple(sorted(rng.choice(low, m, replace=False).tolist())))
    prefix = np.array(sorted(seen), np.int32).reshape(G, m)
    ext, ext_off = [], np.zeros(G + 1, np.int64)
    for g in range(G):
        above = pool[pool > prefix[g, -1]]
        ext.append(np.sort(rng.choice(above, EXT_SIZES[g % len(EXT_SIZES)], replace=False)))
        ext_off[g + 1] = ext_off[g] + ext[-1].size
    return prefix, ext_off, np.concatenate(ext).astype(np.int32)


def _support(B, prefix, ext_off, ext):
    out = np.zeros(ext.size, np.int64)
    for g in range(prefix.shape[0]):
        has = B[:, prefix[g]].all(1)
        e = ext[ext_off[g]:ext_off[g + 1]]
        out[ext_off[g]:ext_off[g + 1]] = (B[:, e] & has[:, None]).sum(0)
    return out


LDS_DEFAULT = None
LDS_12K = 12 * 1024
# id: (T, F1, pool items, m, groups, slab_lds_bytes, slab_cls, slab width, several passes)
# Widths by csrc/host/fa_slab.h over 12 KiB - 256 B of rank map (F1 = 128): n items and C
# candidates take width 16 while 144 n + 4 C <= 12032, else width 8 while 80 n + 4 C <= 12032,
# else width 4, whose capacity (12032 - 48 n) / 4 splits larger levels into passes.
SLAB_CASES = {
    "T1_m14":            (1,    64,  40,  14, 12,  LDS_DEFAULT, 0, 16, False),
    "T64_m12_cls2":      (64,   64,  40,  12, 12,  LDS_DEFAULT, 2, 16, False),
    "T65_m13":           (65,   64,  40,  13, 12,  LDS_DEFAULT, 2, 16, False),
    "T1025_m2_w16":      (1025, 128, 40,  2,  30,  LDS_12K,     0, 16, False),
    "T1023_m3_w8_cls2":  (1023, 128, 100, 3,  60,  LDS_12K,     2, 8,  False),
    "T1024_m3_w4":       (1024, 128, 120, 3,  78,  LDS_12K,     0, 4,  False),
    "T1024_m3_w4_cls2":  (1024, 128, 120, 3,  78,  LDS_12K,     2, 4,  False),
    "T2049_m2_passes":   (2049, 128, 120, 2,  200, LDS_12K,     0, 4,  True),
    "T2049_m3_passes_cls2": (2049, 128, 120, 3, 200, LDS_12K,   2, 4,  True),
    "T2049_m12_w16_cls0": (2049, 64, 40,  12, 18,  LDS_DEFAULT, 0, 16, False),
}


@functools.lru_cache(maxsize=None)
def _slab_case(case):
    T, F1, n_pool, m, G = SLAB_CASES[case][:5]
    rng = np.random.default_rng(300 + sorted(SLAB_CASES).index(case))
    B = _slab_rows(rng, T, F1)
    pool = rng.choice(F1, n_pool, replace=False)          # the other items: used by no candidate
    prefix, ext_off, ext = _candidates(rng, pool, m, G)
    ref = _support(B, prefix, ext_off, ext)
    assert ref.any()
    return B, prefix, ext_off, ext, ref


@pytest.mark.parametrize("dev", BOTH)
@pytest.mark.parametrize("case", list(SLAB_CASES))
def test_slab_level(native, tune, case, dev):
    T, F1, _, m, _, lds, cls, sw, multi = SLAB_CASES[case]
    B, prefix, ext_off, ext, ref = _slab_case(case)
    roff, ranks = _csr(B)
    n_used, C = np.union1d(prefix, ext).size, ext.size
    assert n_used < F1 and set(np.diff(ext_off)) == set(EXT_SIZES)
    tune(slab_cls=cls)
    if lds is not None:
        tune(slab_lds_bytes=lds)
    # the case's parameters give the width it is named for (the rule of csrc/host/fa_slab.h)
    want_sw, cap = prim.slab_width(n_used, C, prim.dl_lds_budget(F1))
    assert want_sw == sw and (C > cap) == multi, (n_used, C, want_sw, cap)
    if dev == "cpu":
        bm, W = ops.build_bitmaps(roff, ranks, None, T, F1)
        got = ops.count_candidates(bm, W, torch.from_numpy(prefix), ext_off, torch.from_numpy(ext), None)
    else:
        got = ops.count_level(roff.to(DEV), ranks.to(DEV), None, T, F1, prefix, ext_off, ext, None, kernel="slab")
        assert got is not None
        plan = dict(prim.LAST_LEVEL_PLAN)
        assert plan["sw"] == sw and (plan["passes"] > 1) == multi and plan["used"] == n_used, plan
        assert plan["cls"] == (1 if cls == 2 and m <= 12 else 0), plan
    assert got.dtype == torch.int64 and np.array_equal(got.cpu().numpy(), ref)


# ---------------------------------------------------------------------------
# 4. F2 compaction: fa_hip_pairs_compact (k_pairs_keep_count / k_pairs_scan / k_pairs_emit)
# ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _compact_counts(F1):
    rng = np.random.default_rng(400 + F1)
    B = (rng.random((40, F1)) < 0.5).astype(np.int64)
    B[0] = 1                                   # every pair occurs: counts >= 1
    iu = np.triu_indices(F1, 1)
    G = _gram(B)
    return G, iu, G[iu]


@pytest.mark.parametrize("dev", GPU)
@pytest.mark.parametrize("keep", ["none", "all", "half"])
@pytest.mark.parametrize("flat", [False, True])
@pytest.mark.parametrize("F1", [2, 3, 256, 257, 1024, 1025, 1300])
def test_pairs_compact(F1, flat, keep, dev):
    G, iu, tri = _compact_counts(F1)
    mc = {"none": int(tri.max()) + 1, "all": int(tri.min()), "half": int(np.median(tri))}[keep]
    sel = tri >= mc
    if keep != "half":
        assert sel.all() == (keep == "all") and sel.any() == (keep == "all")
    elif F1 > 3:
        assert 0.3 < sel.mean() < 0.7
    if flat:
        pc = torch.from_numpy(tri.astype(np.int32)).to(DEV)
    else:
        # the pair kernel's matrix: row stride F1 + (F1 & 1); whatever lies outside the upper
        # triangle (lower triangle, diagonal, padding column) would be kept if it were read
        ld = F1 + (F1 & 1)
        buf = np.full((F1, ld), mc + 7, np.int32)
        buf[iu] = tri
        pc = torch.from_numpy(buf).to(DEV)[:, :F1]
        assert pc.stride(0) == ld
    rows, cnt, n = prim.pairs_compact(pc, F1, mc, flat=flat)
    n = int(n.item())
    assert n == int(sel.sum())
    assert np.array_equal(rows[:n].cpu().numpy(), np.stack([iu[0][sel], iu[1][sel]], 1).astype(np.int32))
    assert np.array_equal(cnt[:n].cpu().numpy(), tri[sel].astype(np.int32))


# ---------------------------------------------------------------------------
# 5. bundle threshold: fa_hip_dl_threshold (one workgroup up to 4096 candidates, else
#    k_dlt_count / k_dlt_scan / k_dlt_emit in 1024-candidate blocks that restart per level)
# ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _threshold_levels(Cs, widths):
    """Per level: C candidate rows of `width` ascending ids and their supports in B.  Level
    l draws its ids from its own 20 items of B, whose densities lie around 0.6 ** (1 / width):
    the supports of every level then spread around 0.6 T, and one threshold cuts them all."""
    rng = np.random.default_rng(500 + sum(Cs) + len(Cs))
    T, per = 300, 20
    mid = np.repeat([0.6 ** (1.0 / w) for w in widths], per)
    B = (rng.random((T, per * len(Cs))) < mid + (1 - mid) * rng.uniform(-0.8, 0.8, mid.size)).astype(np.int64)
    has = B.astype(bool)
    levels = []
    for l, (C, w) in enumerate(zip(Cs, widths)):
        rows = np.stack([rng.choice(per, w, replace=False) for _ in range(C)]) + per * l
        rows = np.sort(rows, 1).astype(np.int32)
        levels.append((rows, has[:, rows].all(2).sum(0).astype(np.int32)))
    return levels


@pytest.fixture(scope="module")
def dl_state():
    return prim.DeviceLevelState(DEV)


THRESHOLD_SETS = [((1,), (3,)), ((1023,), (3,)), ((1024,), (4,)), ((1025,), (3,)), ((4096,), (5,)),
                  ((4097,), (3,)), ((1, 1024, 3100), (3, 4, 14))]


@pytest.mark.parametrize("dev", GPU)
@pytest.mark.parametrize("keep", ["none", "all", "half"])
@pytest.mark.parametrize("Cs,widths", THRESHOLD_SETS, ids=lambda v: "-".join(map(str, v)))
def test_dl_threshold(dl_state, Cs, widths, keep, dev):
    levels = _threshold_levels(Cs, widths)
    allc = np.concatenate([c for _, c in levels])
    mc = {"none": int(allc.max()) + 1, "all": max(int(allc.min()), 0), "half": int(np.median(allc))}[keep]
    if keep == "half" and len(allc) > 1:
        assert 0.3 < (allc >= mc).mean() < 0.7
    # the bundle's counts: the levels one after the other, entries that belong to no level
    # (kept if read) before, between and after them
    S, L, k0 = dl_state, len(levels), 3
    pad, parts, bases, at = np.full(3, mc + 5, np.int32), [], [], 0
    for _, c in levels:
        parts += [pad, c]
        bases.append(at + pad.size)
        at += pad.size + c.size
    counts = torch.from_numpy(np.concatenate(parts + [pad])).to(DEV)
    rows_t = [torch.from_numpy(r).to(DEV) for r, _ in levels]          # kept alive to the end
    S.desc[:] = 0
    for l, (r, c) in enumerate(levels):
        d = S.desc[l]
        d["rows"], d["m"], d["n"], d["C"], d["base"] = rows_t[l].data_ptr(), r.shape[1] - 1, 1, c.size, bases[l]
    S.fsz.fill_(-1)
    rows, cnt, rows_off, cnt_off = prim.dl_threshold(S, L, counts, mc, k0)
    fsz = S.fsz.cpu().numpy()
    rows, cnt = rows.cpu().numpy(), cnt.cpu().numpy()
    for l, (r, c) in enumerate(levels):
        sel = c >= mc
        n, w = int(sel.sum()), r.shape[1]
        assert fsz[k0 + l] == n, (l, fsz[k0:k0 + L])
        assert np.array_equal(cnt[cnt_off[l]:cnt_off[l] + n], c[sel]), l
        assert np.array_equal(rows[rows_off[l]:rows_off[l] + n * w].reshape(n, w), r[sel]), l
    assert (fsz[:k0] == -1).all() and (fsz[k0 + L:] == -1).all()
    del rows_t


# ---------------------------------------------------------------------------
# 6. recommendation: k_recommend / k_recommend_indexed / fa_recommend_cpu
# ---------------------------------------------------------------------------
def _first_match(rules, basket):
    """The reference: the consequent of the first rule whose antecedent is inside the
    basket and whose consequent is not, else -1."""
    have = set(basket)
    for ante, cons in rules:
        if set(ante) <= have and cons not in have:
            return cons
    return -1


def _ante_matches(rules, basket):
    return [r for r, (ante, _) in enumerate(rules) if set(ante) <= set(basket)]


@functools.lru_cache(maxsize=None)
def _rule_table(R, F1):
    """(rules [(antecedent ascending, consequent)], baskets, scenario names).  Random rules
    and baskets live on the low items; the 12 highest items e0..e10, H are reserved for the
    planted rules, so the planted baskets meet exactly the rules named below."""
    rng = np.random.default_rng(600 + 1000 * R + F1)
    lo = F1 - 12
    e, H = list(range(lo, lo + 11)), F1 - 1

    def rand_rule():
        it = rng.choice(lo, int(rng.integers(2, 5)), replace=False)
        return tuple(sorted(it[1:].tolist())), int(it[0])

    rules = [rand_rule() for _ in range(R)]
    baskets, names = [], []

    def add(name, items):
        names.append(name)
        baskets.append(sorted(set(items)))

    add("empty", [])
    add("all items", range(F1))
    if R == 1:
        rules[0] = ((e[0], e[1]), e[2])
        add("match", [e[0], e[1]])
        add("antecedent longer than the basket", [e[0]])
        add("consequent in the basket", [e[0], e[1], e[2]])
    else:
        last = 63 if R == 65 else R - 1
        rules[3] = ((e[0],), e[1])                  # rejected when e1 is in the basket ...
        rules[last] = ((e[0],), e[2])               # ... then this one, steps later, is the first match
        rules[1] = ((e[3], e[4]), e[5])
        rules[20] = ((e[8],), e[2])                 # e8's list hits rule 20, e9's list then rule 10
        rules[10] = ((e[9],), e[3])
        add("earlier match rejected by its consequent", [e[0], e[1]])
        assert _ante_matches(rules, baskets[-1]) == [3, last] and _first_match(rules, baskets[-1]) == e[2]
        add("first match", [e[0]])
        add("antecedent longer than the basket", [e[3]])
        assert _ante_matches(rules, baskets[-1]) == []
        add("two-item antecedent", [e[3], e[4]])
        add("its consequent in the basket", [e[3], e[4], e[5]])
        add("later list, smaller rule", [e[8], e[9]])
        assert _ante_matches(rules, baskets[-1]) == [10, 20] and _first_match(rules, baskets[-1]) == e[3]
        add("later list past the best hit", [e[0], e[9]])
        assert _ante_matches(rules, baskets[-1]) == [3, 10, last]
        if R >= 65:
            rules[64] = ((e[6], e[7]), e[0])
            add("only rule 64 matches", [e[6], e[7]])
            assert _ante_matches(rules, baskets[-1]) == [64] and _first_match(rules, baskets[-1]) == e[0]
        if R >= 200:
            # 80 rules end in H: its list spans two 64-rule steps
            xs = rng.integers(0, lo, 80)
            for k in range(80):
                rules[100 + k] = ((int(xs[k]), H), int((xs[k] + 1 + rng.integers(0, lo - 1)) % lo))
            for k in (0, 63, 64, 70, 79):
                ante, cons = rules[100 + k]
                add(f"hub rule {k}", ante)
                add(f"hub rule {k}, consequent in the basket", ante + (cons,))
            add("hub alone", [H])
    # random baskets: rows of a seeded dense B over all items
    Bk = (rng.random((6, F1)) < 0.3).astype(np.int64)
    for x in range(6):
        add(f"random {x}", np.flatnonzero(Bk[x]).tolist())
    assert all(len(a) >= 1 and list(a) == sorted(set(a)) and c not in a for a, c in rules)
    return rules, baskets, names


def _rules_tensors(rules, dev):
    ante_off = np.zeros(len(rules) + 1, np.int64)
    np.cumsum([len(a) for a, _ in rules], out=ante_off[1:])
    ante = np.array([i for a, _ in rules for i in a], np.int32)
    cons = np.array([c for _, c in rules], np.int32)
    return tuple(torch.from_numpy(v).to(dev) for v in (ante_off, ante, cons))


@pytest.mark.parametrize("dev", BOTH)
@pytest.mark.parametrize("indexed", [False, True], ids=["scan", "indexed"])
@pytest.mark.parametrize("M", [1, 4, 5])
@pytest.mark.parametrize("F1", [31, 32, 33, 70])
@pytest.mark.parametrize("R", [1, 64, 65, 200])
def test_recommend(native, R, F1, M, indexed, dev):
    rules, baskets, names = _rule_table(R, F1)
    want = [_first_match(rules, b) for b in baskets]
    assert -1 in want and max(want) >= 0
    ante_off, ante, cons = _rules_tensors(rules, dev)
    index = prim.recommend_index(ante_off, ante, F1) if indexed else None
    if indexed and R >= 200:
        assert int(torch.diff(index[0]).max()) > 64          # one item's list holds > 64 rules
    # M baskets per call (one wave each, 4 waves a workgroup); the last call wraps round
    K = len(baskets)
    for k0 in range(0, K, M):
        ids = [(k0 + j) % K for j in range(M)]
        boff = np.zeros(M + 1, np.int64)
        np.cumsum([len(baskets[i]) for i in ids], out=boff[1:])
        bask = np.array([x for i in ids for x in baskets[i]], np.int32)
        got = ops.recommend(ante_off, ante, cons, F1, torch.from_numpy(boff).to(dev),
                            torch.from_numpy(bask).to(dev), index=index)
        assert got.dtype == torch.int32
        assert got.cpu().tolist() == [want[i] for i in ids], [names[i] for i in ids]


# ---------------------------------------------------------------------------
# 7. one-workgroup chunked scans (fa_hip.h wg_scan_chunks): k_scan_small, called directly,
#    and level 0 of the device loop (section 8).  Every chunked scan -- also
#    k_dl_pieces_scan and k_dlt_scan, whose chunk loop takes a second step only past
#    262 144 parent rows or a million candidates, too large for an edge test -- is the
#    same function with another load / store, so its chunk boundaries are walked here.
# ---------------------------------------------------------------------------
SCAN_NS = [0, 1, 63, 64, 65, 1023, 1024, 1025, 2048, 3000]


@functools.lru_cache(maxsize=None)
def _scan_input(K, n, big):
    rng = np.random.default_rng(700 + 10 * n + K + (5 if big else 0))
    v = rng.integers(0, 1001, (n, K)).astype(np.int64)
    if big:
        # The kernel scans 64 consecutive counts of a sequence in int32 (one wave) and
        # carries int64 from there on, so the values near 2^30 sit one per 64 elements, at
        # a random place each: 2^30 + 63 * 1000 < 2^31, and the 47 of them pass 2^32.
        for k in range(K):
            at = np.arange(0, n, 64) + rng.integers(0, 64, (n + 63) // 64)
            at = at[at < n]
            v[at, k] = (1 << 30) - rng.integers(0, 1000, at.size)
        assert v.sum(0).min() > 1 << 32
    return v.astype(np.int32)


def _scan_small_check(K, n, big, with_base):
    v = _scan_input(K, n, big)
    base = np.array([(7 << 33) + 11, 5][:K], np.int64) if with_base else np.zeros(K, np.int64)
    want = np.concatenate([base[None], base + np.cumsum(v.astype(np.int64), 0)])     # [n + 1, K]
    src = torch.from_numpy(v.reshape(-1)).to(DEV) if n else torch.zeros(1, dtype=torch.int32, device=DEV)
    out = torch.full((K * (n + 1),), -1, dtype=torch.int64, device=DEV)
    cursor = torch.from_numpy(base).to(DEV) if with_base else None     # the base in, the total out
    rc = ops._native.hip().fa_hip_scan_small(K, src.data_ptr(), n, out.data_ptr(), prim._p(cursor),
                                             torch.cuda.current_stream(DEV).cuda_stream)
    assert rc == 0
    assert np.array_equal(out.cpu().numpy().reshape(n + 1, K), want)
    if with_base:
        assert np.array_equal(cursor.cpu().numpy(), want[n])


@pytest.mark.gpu
@pytest.mark.parametrize("with_base", [False, True], ids=["nobase", "base"])
@pytest.mark.parametrize("n", SCAN_NS)
@pytest.mark.parametrize("K", [1, 2])
def test_scan_small(K, n, with_base):
    _scan_small_check(K, n, False, with_base)


@pytest.mark.gpu
@pytest.mark.parametrize("with_base", [False, True], ids=["nobase", "base"])
@pytest.mark.parametrize("K", [1, 2])
def test_scan_small_int64_carry(K, with_base):
    _scan_small_check(K, 3000, True, with_base)


# ---------------------------------------------------------------------------
# 8. level 0 of the device loop, nothing past it (max_levels = 1): k_dl_decide0 up to
#    4 * kDsBlk parent rows (by n_bound; fa_limits.h), k_ds_blocks / k_ds_decide0 / k_ds_add
#    in kDsBlk-row blocks past it.  The reference is the host generator on the same rows.
# ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _level0_case(n):
    """F_2-shaped parent rows: the pairs (i, j), i < j <= i + 6, a seeded ~20 % of them
    removed, the first n in lexicographic order.  Rows have 0..5 candidates, many none.
    Returns (rows int32 [n, 2], F1, candidates per row int64 [n], candidate rows [C, 3])."""
    rng = np.random.default_rng(800 + n)
    items = n // 4 + 8                               # 6 * 0.8 pairs per item: enough for n
    i = np.repeat(np.arange(items), 6)
    rows = np.stack([i, i + np.tile(np.arange(1, 7), items)], 1)[rng.random(i.size) >= 0.2][:n]
    rows = np.ascontiguousarray(rows, np.int32)
    assert rows.shape == (n, 2)
    F1 = int(rows.max()) + 1
    assert F1 < 32768
    prefix, ext_off, ext = ops.host.apriori_gen(rows)
    per = np.diff(ext_off)
    cnt = np.zeros(n, np.int64)
    cnt[prefix] = per
    cand = np.concatenate([np.repeat(rows[prefix], per, 0), ext[:, None]], 1).astype(np.int32).reshape(-1, 3)
    assert cnt.max(initial=0) <= 5 and len(cand) < 4 * n + 4
    return rows, F1, cnt, cand


LEVEL0_CASES = [(n, n, False) for n in (3, 1023, 1024, 1025, 2049)] + \
               [(n, 16385, True) for n in (3, 4095, 4096, 4097, 8193, 16385)]


@pytest.mark.gpu
@pytest.mark.parametrize("n,n_bound,from_device", LEVEL0_CASES)
def test_dl_level0(dl_state, n, n_bound, from_device):
    rows, F1, cnt, cand = _level0_case(n)
    assert (n_bound > 4 * prim.limits().kDsBlk) == (n_bound == 16385) and (n > prim.limits().kDsBlk) == (n > 4096)
    if n > 1000:
        assert (cnt == 0).mean() > 0.1 and set(range(5)) <= set(cnt.tolist())
    S, K, C = dl_state, prim.dl(), len(cand)
    P0 = torch.from_numpy(rows).to(DEV)
    n_dev = torch.tensor([n], dtype=torch.int64, device=DEV) if from_device else None
    c = prim.dl_bundle_gen(S, P0.data_ptr(), prim._p(n_dev), 0 if from_device else n, n_bound, 2, F1, C + 1,
                           prim.dl_lds_budget(F1), 2.0, 1, torch.cuda.current_stream(DEV).cuda_stream)
    assert not c[K.kDlOverBound]
    assert c[K.kDlNl] == n and c[K.kDlCl] == C
    assert c[K.kDlGl] == int((cnt > 0).sum())
    ws = S.ws.data_ptr()
    off = S.ws[int(S.info[2]) - ws:][:8 * (n + 1)].view(torch.int64).cpu().numpy()
    assert np.array_equal(off, np.concatenate([[0], np.cumsum(cnt)]))
    got = S.ws[int(S.info[3]) - ws:][:12 * C].view(torch.int32).cpu().numpy().reshape(C, 3)
    assert np.array_equal(got, cand)
    del P0
