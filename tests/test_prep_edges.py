"""Edge shapes of the row-preparation kernels (csrc/hip/prep.hip and the wave bitmap build
of count.hip): token histogram, frequent counts per row, the compression tier chain, the
fused two-pass compression with the pair kernel's blocked layout, row hashing, the
vertical bitmap builds and row trimming.

The other tests of these kernels feed generator output and compare the device with the
project's own C++ path, so the generator decides which tier or branch runs.  Here every
input is built on purpose from per-row token lists (seeded where random): an input CSR
(off int64, items int32 over a vocabulary V, tokens distinct within a row) and a lut
(id -> rank, or -1).  The expected result comes from the dense matrix B[n, F1], B[t, r] = 1
iff row t holds a token with lut == r, in numpy, never from another path of this project.
All values are integers and every comparison is exact equality over the whole output.
Every builder asserts that it reaches the edge it is named for; a builder that steers a
dispatch asserts the gate's inequality; a gate that is a kernel limit is read by name from
prim.limits() (csrc/host/fa_limits.h) inside the builder, and the literal shapes keep the
case on the limit.

Ops with a CPU path run on "cpu" too: that proves the builders and the references where
there is no GPU.  The device-only families (compress_rows, item_map / blocked bitmaps) have
an unmarked test each that runs the builders and checks the reference's own invariants.
"""
import functools
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from fastapriori_amd import ops
from fastapriori_amd.ops import primitives as prim
from fastapriori_amd.tuning import TUNING

BOTH = ["cpu", pytest.param("cuda", marks=pytest.mark.gpu)]
GPU = [pytest.param("cuda", marks=pytest.mark.gpu)]

# B is built dense up to this many cells; the cases above it take the same quantities
# from the sparse lists (each says so where it is built)
DENSE_CELLS = 1 << 26


# ---------------------------------------------------------------------------
# builders and references
# ---------------------------------------------------------------------------
def _gram(B):
    """Upper triangle of B.T @ B, int64.  The product runs in float64 (BLAS): every entry
    is an integer below 2^53, so it is exact."""
    A = B.astype(np.float64)
    G = np.rint(A.T @ A).astype(np.int64)
    assert G.max(initial=0) < 1 << 53
    return np.triu(G, 1)


def _csr(B):
    """Dense 0/1 rows -> (roff int64 [T + 1], ranks int32, ascending in each row)."""
    roff = np.zeros(B.shape[0] + 1, np.int64)
    np.cumsum(B.sum(1, dtype=np.int64), out=roff[1:])
    return roff, np.nonzero(B)[1].astype(np.int32)


def _make_lut(rng, V, F1):
    """(lut int32 [V], freq: the id of every rank, infreq: the ids without a rank)."""
    ids = rng.permutation(V)
    lut = np.full(V, -1, np.int32)
    lut[ids[:F1]] = np.arange(F1, dtype=np.int32)
    return lut, ids[:F1].copy(), np.sort(ids[F1:])


def _row(rng, freq, infreq, L, c, ranks=(), tail=False):
    """A row of L distinct tokens, c of them frequent (the given ranks among them), in
    random order; tail: the frequent tokens last."""
    L, c = int(L), int(c)
    forced = np.asarray(ranks, np.int64)
    assert forced.size <= c <= min(L, freq.size) and L - c <= infreq.size
    rest = np.setdiff1d(np.arange(freq.size), forced)
    fr = freq[np.concatenate([forced, rng.choice(rest, c - forced.size, replace=False)])]
    inf = rng.choice(infreq, L - c, replace=False)
    if tail:
        return np.concatenate([rng.permutation(inf), rng.permutation(fr)]).astype(np.int32)
    return rng.permutation(np.concatenate([fr, inf])).astype(np.int32)


def _pack(rows):
    off = np.zeros(len(rows) + 1, np.int64)
    np.cumsum([len(r) for r in rows], out=off[1:])
    items = np.concatenate([np.asarray(r, np.int32) for r in rows] + [np.zeros(0, np.int32)]).astype(np.int32)
    return off, items


def _rand_rows(rng, lens, V):
    """Rows of the given lengths, each a random set of distinct ids of [0, V) in random
    order (vectorised: the first lens[t] entries of a random permutation per row)."""
    lens = np.asarray(lens, np.int64)
    assert lens.max(initial=0) <= V
    perm = np.argsort(rng.random((lens.size, V)), axis=1).astype(np.int32)
    items = perm[np.arange(V)[None, :] < lens[:, None]]
    off = np.zeros(lens.size + 1, np.int64)
    np.cumsum(lens, out=off[1:])
    return off, items


def _case(off, items, lut, F1, **extra):
    off, items, lut = np.asarray(off, np.int64), np.asarray(items, np.int32), np.asarray(lut, np.int32)
    n = off.size - 1
    assert off[0] == 0 and off[-1] == items.size and (np.diff(off) >= 0).all()
    assert items.size == 0 or (0 <= items.min() and items.max() < lut.size)
    assert lut.max(initial=-1) < F1
    return SimpleNamespace(off=off, items=items, lut=lut, F1=F1, n=n, nnz=int(items.size), L=np.diff(off),
                           dense=n * F1 <= DENSE_CELLS, **extra)


def _from_rows(rows, lut, F1, **extra):
    off, items = _pack(rows)
    return _case(off, items, lut, F1, **extra)


def _reference(case, dense=None):
    """c, kept, roff, ranks and the length histogram of a case, from the dense B (and B
    itself, Bk = B[kept]); dense=False: the same from the sparse lists."""
    dense = case.dense if dense is None else dense
    n, F1 = case.n, case.F1
    rowid = np.repeat(np.arange(n), case.L)
    r = case.lut[case.items].astype(np.int64)
    m = r >= 0
    if dense:
        B = np.zeros((n, F1), np.uint8)
        B[rowid[m], r[m]] = 1
        assert int(B.sum(dtype=np.int64)) == int(m.sum())          # tokens are distinct within a row
        c = B.sum(1, dtype=np.int64)
        kept = np.flatnonzero(c >= 2)
        Bk = B[kept]
        ranks = np.nonzero(Bk)[1].astype(np.int32)
    else:
        B = Bk = None
        c = np.bincount(rowid[m], minlength=n).astype(np.int64)
        kept = np.flatnonzero(c >= 2)
        sel = m & (c[rowid] >= 2)
        ranks = r[sel][np.lexsort((r[sel], rowid[sel]))].astype(np.int32)
    roff = np.zeros(kept.size + 1, np.int64)
    np.cumsum(c[kept], out=roff[1:])
    hist = np.bincount(np.minimum(c[kept], 255), minlength=256).astype(np.int64)
    return SimpleNamespace(B=B, Bk=Bk, c=c, kept=kept.astype(np.int32), roff=roff, ranks=ranks, hist=hist,
                           T=int(kept.size), nnz=int(roff[-1]))


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


# ---------------------------------------------------------------------------
# 1. txn_freq_count: fa_hip_txn_freq_count picks a kernel by mean row length
# ---------------------------------------------------------------------------
TFC_THREAD_MAX = 8     # prep.hip fa_hip_txn_freq_count: nnz > 8 * n leaves the thread-per-row kernel
TFC_WV_MAX = 48        # ... and nnz > 48 * n the wave-per-64-rows kernel (k_txn_freq_count_wv)


def _tfc_kernel(case):
    if case.nnz > TFC_THREAD_MAX * case.n and case.nnz <= TFC_WV_MAX * case.n:
        return "wv"
    return "wave" if case.nnz > TFC_WV_MAX * case.n else "thread"


def _tfc_thread(n):
    # rows of 0, 1 and 8 tokens, all infrequent / all frequent / mixed
    rng = np.random.default_rng(1100 + n)
    lut, freq, infreq = _make_lut(rng, 40, 20)
    specs = [(0, 0), (1, 0), (1, 1), (8, 0), (8, 8), (8, 3)]
    rows = [_row(rng, freq, infreq, *specs[(t + n) % len(specs)]) for t in range(n)]
    case = _from_rows(rows, lut, 20)
    assert case.nnz <= TFC_THREAD_MAX * case.n and _tfc_kernel(case) == "thread"
    return case


def _group_lens(rng, total, nonempty=False):
    """64 row lengths summing to total (random; nonempty: every row >= 1)."""
    if nonempty:
        return 1 + rng.multinomial(total - 64, np.full(64, 1 / 64))
    return rng.multinomial(total, np.full(64, 1 / 64))


def _tfc_wv(tail):
    # 64-row groups of 0, 1, 511, 512, 513 and 1100 tokens, one row of 200 tokens in a group of
    # otherwise empty rows, filler groups of 30-token rows that keep the mean inside the
    # gate, and `tail` rows of a last partial group
    rng = np.random.default_rng(1200 + tail)
    V = 600
    lut, _, _ = _make_lut(rng, V, 300)
    groups = [np.zeros(64, np.int64)]
    one = np.zeros(64, np.int64)
    one[37] = 1
    groups.append(one)
    for total in (511, 512, 513, 1100):
        lens = _group_lens(rng, total)
        lens[10] += lens[9]                     # an empty row inside the group
        lens[9] = 0
        groups.append(lens)
    single = np.zeros(64, np.int64)
    single[5] = 200
    groups.append(single)
    groups += [np.full(64, 30, np.int64)] * 3
    lens = np.concatenate(groups + [np.full(tail, 10, np.int64)])
    off, items = _rand_rows(rng, lens, V)
    case = _case(off, items, lut, 300)
    tot = [int(case.L[64 * g:64 * g + 64].sum()) for g in range(7)]
    assert tot == [0, 1, 511, 512, 513, 1100, 200]
    assert case.n % 64 == tail and TFC_THREAD_MAX * case.n < case.nnz <= TFC_WV_MAX * case.n
    assert _tfc_kernel(case) == "wv"
    # rows that straddle a 64-token window and the 512-token step of their group; empty rows
    # inside the groups
    g = 5
    s = off[64 * g:64 * g + 64] - off[64 * g]
    e = off[64 * g + 1:64 * g + 65] - off[64 * g]
    assert ((s < 512) & (e > 512)).any() and ((s // 64 != (e - 1) // 64) & (e > s)).any()
    assert (case.L[64 * 2:64 * 6] == 0).any()
    return case


def _tfc_wave():
    rng = np.random.default_rng(1300)
    lens = np.array([0, 1, 255, 256, 257, 513, 256, 0, 513])
    lut, _, _ = _make_lut(rng, 600, 300)
    off, items = _rand_rows(rng, lens, 600)
    case = _case(off, items, lut, 300)
    assert case.nnz > TFC_WV_MAX * case.n and _tfc_kernel(case) == "wave"
    return case


def _tfc_grid_cap():
    # 32768 + 5 rows of 49..52 tokens: the grid stops at 8192 workgroups of 4 waves, so the
    # waves of the first 5 rows take a second row
    rng = np.random.default_rng(1400)
    n = 32768 + 5
    lut, _, _ = _make_lut(rng, 128, 64)
    off, items = _rand_rows(rng, rng.integers(49, 53, n), 128)
    case = _case(off, items, lut, 64)
    assert case.L.min() == 49 and case.L.max() == 52 and case.nnz > TFC_WV_MAX * case.n
    assert (case.n + 3) // 4 > 8192 and case.n > 8192 * 4
    return case


TFC_CASES = {
    "thread_n1": lambda: _tfc_thread(1), "thread_n255": lambda: _tfc_thread(255),
    "thread_n256": lambda: _tfc_thread(256), "thread_n257": lambda: _tfc_thread(257),
    "wv_groups_tail1": lambda: _tfc_wv(1), "wv_groups_tail63": lambda: _tfc_wv(63),
    "wave_lengths": _tfc_wave, "wave_grid_cap": _tfc_grid_cap,
}


@pytest.mark.parametrize("dev", BOTH)
@pytest.mark.parametrize("name", list(TFC_CASES))
def test_txn_freq_count(native, name, dev):
    case = TFC_CASES[name]()
    ref = _reference(case)
    got = ops.txn_freq_count(_t(case.off, dev), _t(case.items, dev), _t(case.lut, dev))
    assert got.dtype == torch.int32
    assert np.array_equal(got.cpu().numpy(), ref.c)


# ---------------------------------------------------------------------------
# 2. compress: the tier chain by mean row length
# ---------------------------------------------------------------------------
CMP_STAGED64_MEAN = 16.0     # primitives.py COMPRESS_STAGED64_MEAN_LEN: nnz > 16 * n -> the 64-token staged tier
CMP_WAVE_MEAN = 48.0         # tuning.py compress_wave_mean_len: nnz > 48 * n (and F1 <= kCwMaxF1) -> every row by k_compress_wave


def _cmp_tier(case, F1arg):
    if F1arg is not None and F1arg <= prim.limits().kCwMaxF1 and case.nnz > CMP_WAVE_MEAN * case.n:
        return "wave"
    return "staged64" if case.nnz > CMP_STAGED64_MEAN * case.n else "staged16"


def _spans(case, ref):
    """Input tokens between the first and the last kept row of every 256-kept-row workgroup."""
    out = []
    for x0 in range(0, ref.T, 256):
        x1 = min(x0 + 256, ref.T)
        out.append(int(case.off[ref.kept[x1 - 1] + 1] - case.off[ref.kept[x0]]))
    return out


def _cmp_short(T):
    # L in {2, 15, 16, 17} with c in {2, L}, rows whose two frequent tokens are the last two,
    # dropped rows in between; exactly T kept rows
    rng = np.random.default_rng(2100 + T)
    lut, freq, infreq = _make_lut(rng, 80, 40)
    keep = [(2, 2), (15, 2), (15, 15), (16, 2), (16, 16), (17, 2), (17, 17)]
    drop = [(0, 0), (1, 1), (5, 0), (16, 1), (17, 1)]
    rows, k = [], 0
    while k < T:
        if len(rows) % 3 == 2:
            rows.append(_row(rng, freq, infreq, *drop[len(rows) % len(drop)]))
            continue
        L, c = keep[k % len(keep)]
        rows.append(_row(rng, freq, infreq, L, c, tail=(k % 2 == 1)))
        k += 1
    case = _from_rows(rows, lut, 40)
    ref = _reference(case)
    assert ref.T == T and case.nnz <= CMP_STAGED64_MEAN * case.n
    if T >= 7:
        assert set(case.L[ref.kept]) == {2, 15, 16, 17}
    return case, 40, "staged16"


def _cmp_span(kept_len, drop_len, spans, f1arg, tier):
    # per workgroup: 256 kept rows of kept_len tokens and 255 dropped rows between them, so
    # that the input span from the first to the last kept row holds spans[g] tokens; empty
    # rows after each workgroup (outside every span) pull the mean into the tier's gate
    rng = np.random.default_rng(2200 + spans[0])
    lut, freq, infreq = _make_lut(rng, 600, 300)
    rows = []
    for span in spans:
        extra = span - 256 * kept_len - 255 * drop_len
        assert 0 <= extra <= 64
        for k in range(256):
            rows.append(_row(rng, freq, infreq, kept_len, rng.integers(2, kept_len + 1)))
            if k < 255:
                rows.append(_row(rng, freq, infreq, drop_len + (extra if k == 100 else 0), k % 2))
        rows += [np.zeros(0, np.int32)] * 300
    case = _from_rows(rows, lut, 300)
    ref = _reference(case)
    assert ref.T == 256 * len(spans) and _spans(case, ref) == list(spans)
    assert _cmp_tier(case, f1arg) == tier
    return case, f1arg, tier


def _cmp_long_flags(f1arg):
    # short-mean data with rows of 17, 64, 65 and 200 tokens: k_compress_regs<64>, then by
    # flag the wave tier (F1 given) or the LDS tier (F1 = None)
    rng = np.random.default_rng(2300)
    lut, freq, infreq = _make_lut(rng, 600, 300)
    rows = []
    for L, c in [(17, 17), (17, 2), (64, 64), (64, 2), (64, 30), (65, 65), (65, 2), (200, 200), (200, 2),
                 (65, 1), (64, 1), (200, 0)]:
        rows += [_row(rng, freq, infreq, 3, k % 4) for k in range(11)]
        rows.append(_row(rng, freq, infreq, L, c))
    case = _from_rows(rows, lut, 300)
    ref = _reference(case)
    assert case.nnz <= CMP_STAGED64_MEAN * case.n
    kl, kc = case.L[ref.kept], ref.c[ref.kept]
    for L in (17, 64, 65, 200):                                     # kept with c = 2 and c = L, dropped with c < 2
        assert {2, L} <= set(kc[kl == L].tolist()), L
    assert {64, 65, 200} <= set(case.L[ref.c < 2].tolist())
    return case, f1arg, "staged16"


CMP_U16_BELOW = 0xFFFF       # prep.hip fa_hip_compress_staged64: 0 < F1 < 0xFFFF stages the span as u16 (0xFFFF = not frequent)


def _cmp_staged64_lengths(f1, f1arg, u16):
    # 16 < mean <= 48: L in {17, 63, 64, 65, 200} with c in {2, L / 2, L}; F1 = 300 and F1 = 65534
    # (top rank 65533, next to the sentinel) stage the span as u16, F1 = 65535 and F1 = None as u32
    rng = np.random.default_rng(2400 + f1)
    lut, freq, infreq = _make_lut(rng, f1 + 300, f1)
    rows = []
    for L in (17, 63, 64, 65, 200):
        for c in (2, L // 2, L):
            rows.append(_row(rng, freq, infreq, L, c, ranks=(0, f1 - 1)))
            rows += [_row(rng, freq, infreq, 20, k) for k in (0, 1, 7, 20)]
    case = _from_rows(rows, lut, f1)
    assert CMP_STAGED64_MEAN * case.n < case.nnz <= CMP_WAVE_MEAN * case.n
    assert _cmp_tier(case, f1arg) == "staged64"
    assert (f1arg is not None and 0 < f1arg < CMP_U16_BELOW) == u16
    ref = _reference(case)
    assert {17, 63, 64, 65, 200} <= set(case.L[ref.kept].tolist()) 
    assert ref.Bk[case.L[ref.kept] != 20][:, [0, f1 - 1]].all() and (case.L[ref.kept] != 20).sum() == 15
    return case, f1arg, "staged64"


def _cmp_wave(f1):
    # mean > 48: every row through k_compress_wave, M = ceil(F1 / 4096) words per lane; rows
    # that hold the ranks at the word and lane boundaries
    rng = np.random.default_rng(2500 + f1)
    lut, freq, infreq = _make_lut(rng, f1 + 700, f1)
    edge = [r for r in (0, 63, 64, 4095, 4096, f1 - 1) if r < f1]
    rows = []
    for L in (49, 256, 257, 600):
        rows.append(_row(rng, freq, infreq, L, min(L, f1), ranks=sorted(set(edge))))
        rows.append(_row(rng, freq, infreq, L, min(L, f1) // 2, ranks=(f1 - 1,)))
        rows.append(_row(rng, freq, infreq, L, 2))
        rows.append(_row(rng, freq, infreq, L, 1))                   # dropped
    case = _from_rows(rows, lut, f1)
    assert case.nnz > CMP_WAVE_MEAN * case.n and _cmp_tier(case, f1) == "wave"
    ref = _reference(case)
    assert set(case.L[ref.kept].tolist()) == {49, 256, 257, 600} and (ref.c == 1).sum() == 4
    assert ref.Bk[:, edge].all(1).sum() >= 4 and ref.Bk[:, f1 - 1].sum() >= 8     # a row per length holds every edge rank
    assert (f1 + 4095) // 4096 == {64: 1, 4096: 1, 4097: 2, 65536: 16}[f1]
    assert (f1 == prim.limits().kCwMaxF1) == (f1 == 65536)
    return case, f1, "wave"


def _cmp_wave_many():
    # 32768 + 5 kept rows: the grid stops at 8192 workgroups, so five waves take a second
    # row and their LDS bitmap must be clean again
    rng = np.random.default_rng(2600)
    n = 32768 + 5
    lut, _, _ = _make_lut(rng, 128, 64)
    off, items = _rand_rows(rng, rng.integers(49, 53, n), 128)
    case = _case(off, items, lut, 64)
    ref = _reference(case)
    assert ref.T == n and case.nnz > CMP_WAVE_MEAN * case.n and (n + 3) // 4 > 8192
    return case, 64, "wave"


def _cmp_wide():
    # F1 = 66000 > kCwMaxF1: no wave tier.  Rows of 65, 16384 and 16385 tokens go by flag to
    # k_compress_lds, which sorts up to kLongMax tokens and leaves the last row to torch
    rng = np.random.default_rng(2700)
    f1 = 66000
    lut, freq, infreq = _make_lut(rng, 70000, f1)
    rows = [_row(rng, freq, infreq, 65, 60, ranks=(0, f1 - 1)), _row(rng, freq, infreq, 16384, 15000, ranks=(0, f1 - 1)),
            _row(rng, freq, infreq, 16385, 16385, ranks=(0, f1 - 1)), _row(rng, freq, infreq, 100, 1)]
    case = _from_rows(rows, lut, f1)
    assert sorted(case.L.tolist())[-2:] == [prim.limits().kLongMax, prim.limits().kLongMax + 1]
    assert f1 > prim.limits().kCwMaxF1 and _cmp_tier(case, f1) == "staged64"
    return case, f1, "staged64"


CMP_CASES = {
    "staged16_T1": lambda: _cmp_short(1), "staged16_T255": lambda: _cmp_short(255),
    "staged16_T256": lambda: _cmp_short(256), "staged16_T257": lambda: _cmp_short(257),
    # kCSpan tokens: staged at 8191 and 8192, read row by row at 8193
    "staged16_spans": lambda: _cmp_span(16, 16, (8191, 8192, 8193), 300, "staged16"),
    "staged16_long_rows_wave": lambda: _cmp_long_flags(300),
    "staged16_long_rows_lds": lambda: _cmp_long_flags(None),
    "staged64_u16": lambda: _cmp_staged64_lengths(300, 300, True),
    "staged64_u16_F65534": lambda: _cmp_staged64_lengths(65534, 65534, True),
    "staged64_u32_F65535": lambda: _cmp_staged64_lengths(65535, 65535, False),
    "staged64_u32_Fnone": lambda: _cmp_staged64_lengths(300, None, False),
    # SPAN = 16384 tokens for both element types
    "staged64_spans_u16": lambda: _cmp_span(40, 24, (16383, 16384, 16385), 300, "staged64"),
    "staged64_spans_u32": lambda: _cmp_span(40, 24, (16383, 16384, 16385), None, "staged64"),
    "wave_F64": lambda: _cmp_wave(64), "wave_F4096": lambda: _cmp_wave(4096),
    "wave_F4097": lambda: _cmp_wave(4097), "wave_F65536": lambda: _cmp_wave(65536),
    "wave_second_row": _cmp_wave_many,
    "wide_F66000_lds_torch": _cmp_wide,
}


@pytest.mark.parametrize("dev", BOTH)
@pytest.mark.parametrize("name", list(CMP_CASES))
def test_compress_tiers(native, name, dev):
    assert TUNING.compress_wave_mean_len == CMP_WAVE_MEAN and prim.COMPRESS_STAGED64_MEAN_LEN == CMP_STAGED64_MEAN
    case, f1arg, tier = CMP_CASES[name]()
    assert _cmp_tier(case, f1arg) == tier
    ref = _reference(case)
    assert ref.T > 0
    got = ops.compress(_t(case.off, dev), _t(case.items, dev), _t(case.lut, dev), _t(ref.kept, dev),
                       _t(ref.roff, dev), f1arg)
    assert got.dtype == torch.int32
    assert np.array_equal(got.cpu().numpy(), ref.ranks)


# ---------------------------------------------------------------------------
# 3. compress_rows: k_cmp_agg / the three-kernel scan / k_cmp_emit and the fused layout
# ---------------------------------------------------------------------------
# kCmpSpan: a workgroup's 256 rows are staged up to that many tokens; kCmpMidPerWave; kScanChunk
PROBE_ROWS = 1 << 18     # primitives.py DEDUP_PROBE_ROWS


def _wg_tokens(case):
    return [int(case.off[min(r0 + 256, case.n)] - case.off[r0]) for r0 in range(0, case.n, 256)]


def _mid_per_wave(case, ref):
    """Kept rows of 17..64 tokens in every wave of 64 input rows (the rows cmp_mid sorts in
    a staged workgroup, up to 8 per wave)."""
    mid = (ref.c >= 2) & (case.L >= 17) & (case.L <= 64)
    pad = np.zeros((-case.n) % 64, bool)
    return np.concatenate([mid, pad]).reshape(-1, 64).sum(1)


def _short_rows(rng, freq, infreq, k, lo=0, hi=16):
    rows = []
    for _ in range(k):
        L = int(rng.integers(lo, hi + 1))
        rows.append(_row(rng, freq, infreq, L, rng.integers(max(0, L - infreq.size), min(L, freq.size) + 1)))
    return rows


def _fused_sizes(n):
    rng = np.random.default_rng(3100 + n)
    lut, freq, infreq = _make_lut(rng, 60, 30)
    return _from_rows(_short_rows(rng, freq, infreq, n), lut, 30)


def _fused_none_kept():
    rng = np.random.default_rng(3200)
    lut, freq, infreq = _make_lut(rng, 60, 30)
    rows = [_row(rng, freq, infreq, k % 18, k % 2 if k % 18 else 0) for k in range(300)]
    case = _from_rows(rows, lut, 30)
    assert _reference(case).T == 0
    return case


def _fused_empty_workgroups():
    # workgroups 0 and 2 keep no row
    rng = np.random.default_rng(3300)
    lut, freq, infreq = _make_lut(rng, 60, 30)
    rows = []
    for g in range(4):
        if g % 2 == 0:
            rows += [_row(rng, freq, infreq, k % 17, min(k % 17, k % 2)) for k in range(256)]
        else:
            rows += _short_rows(rng, freq, infreq, 256)
    case = _from_rows(rows, lut, 30)
    ref = _reference(case)
    per = np.bincount(ref.kept // 256, minlength=4)
    assert per[0] == 0 and per[2] == 0 and per[1] > 0 and per[3] > 0
    return case


def _fused_lengths():
    # L in {0, 1, 2, 16, 17, 32, 33, 64, 65, 255} with c from 0 to L, in two different orders
    # (two workgroups); rows of L > 16 with c = 2 and with c < 2
    rng = np.random.default_rng(3400)
    lut, freq, infreq = _make_lut(rng, 600, 300)
    specs = sorted({(L, c) for L in (0, 1, 2, 16, 17, 32, 33, 64, 65, 255) for c in (0, 1, 2, L // 2, L - 1, L)
                    if 0 <= c <= L})
    rows = []
    for g in range(2):
        order = rng.permutation(len(specs))
        rows += [_row(rng, freq, infreq, *specs[i]) for i in order]
        rows += _short_rows(rng, freq, infreq, 256 - len(specs), 0, 4)
    case = _from_rows(rows, lut, 300)
    assert case.n == 512 and max(_wg_tokens(case)) <= prim.limits().kCmpSpan
    ref = _reference(case)
    for r0 in (0, 256):
        L, c = case.L[r0:r0 + 256], ref.c[r0:r0 + 256]
        assert {0, 1, 2, 16, 17, 32, 33, 64, 65, 255} <= set(L.tolist())
        for want in (2, 16, 17, 32, 33, 64, 65, 255):
            assert {0, 1, 2, want - 1, want} <= set(c[L == want].tolist()), want
        assert ((L > 16) & (c == 2)).any() and ((L > 16) & (c < 2)).any()
    assert _mid_per_wave(case, ref).max() >= 1
    return case


def _mid_row(rng, freq, infreq, lo, hi, k):
    L = (lo, hi, int(rng.integers(lo, hi + 1)))[k % 3]
    return _row(rng, freq, infreq, L, (2, L, L // 2)[(k // 3 + k) % 3])


def _fused_mid_counts():
    # one workgroup whose waves hold 7, 8, 9 and 64 kept rows of 17..64 tokens: the ninth
    # and later rows of a wave come out of the overflow tiers
    rng = np.random.default_rng(3500)
    lut, freq, infreq = _make_lut(rng, 600, 300)
    rows = []
    for nmid in (7, 8, 9):
        wave = [_mid_row(rng, freq, infreq, 17, 64, k) for k in range(nmid)]
        wave += [_row(rng, freq, infreq, 20, k % 2) for k in range(3)]          # L > 16, c < 2: no mid row
        wave += _short_rows(rng, freq, infreq, 64 - len(wave), 0, 3)
        rows += [wave[i] for i in rng.permutation(64)]
    rows += [_row(rng, freq, infreq, 17 + k % 4, 2 + k % 3) for k in range(64)]
    case = _from_rows(rows, lut, 300)
    assert _mid_per_wave(case, _reference(case)).tolist() == [7, 8, 9, 64]
    assert _wg_tokens(case)[0] <= prim.limits().kCmpSpan
    return case


def _fused_mid_slots():
    # n32 rows of 17..32 tokens (two per sort slot, one per 32-lane half) against n64 rows of
    # 33..64 tokens (one per slot) in one wave each: halves only, halves and then a long
    # row in one pair of slots, long rows only
    rng = np.random.default_rng(3600)
    lut, freq, infreq = _make_lut(rng, 600, 300)
    rows, want = [], []
    for n32 in (0, 1, 2, 3):
        for n64 in (0, 1, 5):
            wave = [_mid_row(rng, freq, infreq, 17, 32, k) for k in range(n32)]
            wave += [_mid_row(rng, freq, infreq, 33, 64, k + n32) for k in range(n64)]
            wave += _short_rows(rng, freq, infreq, 64 - len(wave), 0, 5)
            rows += [wave[i] for i in rng.permutation(64)]
            want.append((n32, n64))
    case = _from_rows(rows, lut, 300)
    ref = _reference(case)
    k32 = ((ref.c >= 2) & (case.L >= 17) & (case.L <= 32)).reshape(-1, 64).sum(1)
    k64 = ((ref.c >= 2) & (case.L >= 33) & (case.L <= 64)).reshape(-1, 64).sum(1)
    assert list(zip(k32.tolist(), k64.tolist())) == want and max(_wg_tokens(case)) <= prim.limits().kCmpSpan
    assert (k32 + k64).max() <= prim.limits().kCmpMidPerWave
    return case


def _fused_wg_tokens():
    # workgroups of 4095, 4096 and 4097 tokens: at 4097 nothing is staged, so the rows of
    # more than 16 tokens all overflow and the short rows store directly
    rng = np.random.default_rng(3700)
    lut, freq, infreq = _make_lut(rng, 600, 300)
    rows = []
    for total in (4095, 4096, 4097):
        lens = np.full(256, 15)
        lens[rng.choice(64, 6, replace=False)] = [17, 20, 32, 33, 40, 64]      # one wave: they share sort slots
        d = total - lens.sum()
        short = np.flatnonzero(lens == 15)
        step = 1 if d > 0 else -1
        lens[rng.choice(short, abs(d), replace=False)] += step
        assert lens.sum() == total and lens.min() >= 14
        rows += [_row(rng, freq, infreq, L, (2, L, L // 2, 1)[k % 4]) for k, L in enumerate(lens)]
    case = _from_rows(rows, lut, 300)
    assert _wg_tokens(case) == [4095, 4096, 4097]
    # the rows of 17..64 tokens of a workgroup lie in its first wave, two or more of them of
    # <= 32 tokens: in the staged workgroups they share a sort slot, one per 32-lane half
    ref = _reference(case)
    mid = (ref.c >= 2) & (case.L >= 17)
    assert all(mid[r0:r0 + 64].sum() == mid[r0:r0 + 256].sum() >= 4 for r0 in (0, 256, 512))
    assert all((mid & (case.L <= 32))[r0:r0 + 64].sum() >= 2 for r0 in (0, 256, 512))
    return case


def _fused_full_output():
    # 256 rows of 16 frequent tokens: 4096 staged tokens in and 4096 out
    rng = np.random.default_rng(3800)
    lut, freq, infreq = _make_lut(rng, 600, 300)
    rows = [_row(rng, freq, infreq, 16, 16) for _ in range(256)] + _short_rows(rng, freq, infreq, 40)
    case = _from_rows(rows, lut, 300)
    ref = _reference(case)
    assert _wg_tokens(case)[0] == prim.limits().kCmpSpan and int(ref.c[:256].sum()) == prim.limits().kCmpSpan
    return case


def _fused_blocks(f1, T):
    # nb = ceil(F1 / 256) blocks of 256 ranks; exactly T kept rows (T = 64 q and 64 q + 1:
    # the batch bases), dropped rows in between
    rng = np.random.default_rng(3900 + f1)
    lut, freq, infreq = _make_lut(rng, f1 + 20, f1)
    rows, k = [], 0
    while k < T:
        if len(rows) % 4 == 3:
            L = int(rng.integers(0, 17))
            rows.append(_row(rng, freq, infreq, L, min(L, int(rng.integers(0, 2)))))
            continue
        c = int(rng.integers(2, min(f1, 16) + 1))
        forced = (f1 - 1,) if k % 5 == 0 else (0,) if k % 5 == 1 else ()
        rows.append(_row(rng, freq, infreq, min(16, c + int(rng.integers(0, 4))), c, ranks=forced))
        k += 1
    case = _from_rows(rows, lut, f1)
    ref = _reference(case)
    assert ref.T == T and ref.Bk[:, f1 - 1].any() and ref.Bk[:, 0].any()
    assert (f1 + 255) // 256 == {2: 1, 256: 1, 257: 2, 2048: 8}[f1]
    if f1 == 257:                                                   # rank 256 alone in block 1
        assert ref.Bk[:, 256:].shape[1] == 1 and 0 < ref.Bk[:, 256].sum() < T
    return case


def _fused_no_layout():
    # F1 = 2049: nine blocks, so no block counts and no layout; one row of 300 frequent items
    # (histogram bin 255) and rows of exactly 254 and 255
    rng = np.random.default_rng(4000)
    lut, freq, infreq = _make_lut(rng, 2100, 2049)
    rows = _short_rows(rng, freq, infreq, 100)
    rows.insert(40, _row(rng, freq, infreq, 310, 300, ranks=(0, 2047, 2048)))
    rows.insert(50, _row(rng, freq, infreq, 254, 254))
    rows.insert(60, _row(rng, freq, infreq, 260, 255))
    case = _from_rows(rows, lut, 2049)
    ref = _reference(case)
    assert ref.hist[254] == 1 and ref.hist[255] == 2 and ref.c.max() == 300
    return case


def _fused_two_blocks():
    # F1 = 512: rows of 255 items in block 0, of 130 + 125, of 254 + 1, of 254 (histogram bins
    # 254 and 255 hit exactly), and kept rows with no item in block 0 or none in block 1
    rng = np.random.default_rng(4100)
    lut, freq, infreq = _make_lut(rng, 900, 512)
    lo, hi = np.arange(256), np.arange(256, 512)
    planted = [
        (255, np.concatenate([rng.choice(lo, 255, replace=False)])),
        (260, np.concatenate([rng.choice(lo, 130, replace=False), rng.choice(hi, 125, replace=False)])),
        (255, np.concatenate([rng.choice(lo, 254, replace=False), [511]])),
        (300, np.concatenate([rng.choice(lo, 127, replace=False), rng.choice(hi, 127, replace=False)])),
        (5, rng.choice(hi, 3, replace=False)), (16, rng.choice(hi, 16, replace=False)),
        (4, rng.choice(lo, 2, replace=False)), (40, rng.choice(hi, 30, replace=False)),
        (40, rng.choice(lo, 30, replace=False)),
    ]
    rows = _short_rows(rng, freq, infreq, 120)
    for k, (L, rk) in enumerate(planted):
        rows.insert(7 + 11 * k, _row(rng, freq, infreq, L, rk.size, ranks=rk))
    case = _from_rows(rows, lut, 512)
    ref = _reference(case)
    assert ref.hist[254] == 1 and ref.hist[255] == 3 and ref.c.max() == 255
    b0, b1 = ref.Bk[:, :256].sum(1), ref.Bk[:, 256:].sum(1)
    assert b0.max() == 255 and ((b0 == 130) & (b1 == 125)).any() and ((b0 == 254) & (b1 == 1)).any()
    assert (b0 == 0).any() and (b1 == 0).any()
    return case


def _fused_block_scan_chunks():
    # 131072 + 300 rows of 2..3 tokens with F1 = 2048: nb * nwg = 8 * 514 > 4096, the block
    # sequence of the scan takes two chunks.  B would hold 2.7e8 cells: the reference comes
    # from the sparse lists (_reference(dense=False), _layout_sparse, _pairs_sparse)
    rng = np.random.default_rng(4200)
    n, V = 131072 + 300, 2048
    lens = rng.integers(2, 4, n)
    a = rng.integers(0, V, n)
    step = rng.integers(1, 700, n)
    off = np.zeros(n + 1, np.int64)
    np.cumsum(lens, out=off[1:])
    j = np.arange(off[-1]) - np.repeat(off[:-1], lens)
    items = ((np.repeat(a, lens) + j * np.repeat(step, lens)) % V).astype(np.int32)      # distinct: 3 * 700 < V
    lut = rng.permutation(V).astype(np.int32)
    case = _case(off, items, lut, V)
    nwg = (n + 255) // 256
    assert not case.dense and 8 * nwg > prim.limits().kScanChunk >= nwg
    return case


def _fused_all_scan_chunks():
    # 4096 * 256 + 257 rows of 2..3 tokens with V = F1 = 3: 4098 workgroups, so all four
    # sequences of the scan take two chunks.  (B has only three columns, so it stays dense.)
    rng = np.random.default_rng(4300)
    n = 4096 * 256 + 257
    lens = rng.integers(2, 4, n)
    off, items = _rand_rows(rng, lens, 3)
    lut = np.array([1, 2, 0], np.int32)
    case = _case(off, items, lut, 3)
    assert (n + 255) // 256 > prim.limits().kScanChunk and case.dense
    return case


def _fused_probe():
    # the dedup probe hashes the first 2^18 kept rows, those of <= 16 items: rows of 16 and
    # 17 items on both sides of kept row 2^18, all other rows of two tokens (many equal)
    rng = np.random.default_rng(4400)
    n, V = PROBE_ROWS + 200, 40
    a = rng.integers(0, V, n)
    b = (a + 1 + rng.integers(0, V - 1, n)) % V
    rows_at = {PROBE_ROWS - 4: 16, PROBE_ROWS - 3: 17, PROBE_ROWS - 1: 16, PROBE_ROWS: 16, PROBE_ROWS + 1: 17,
               PROBE_ROWS + 5: 16, 10: 17, 11: 16}
    lens = np.full(n, 2)
    for t, L in rows_at.items():
        lens[t] = L
    off = np.zeros(n + 1, np.int64)
    np.cumsum(lens, out=off[1:])
    items = np.zeros(off[-1], np.int32)
    two = np.flatnonzero(lens == 2)
    items[off[two]], items[off[two] + 1] = a[two], b[two]
    for t, L in rows_at.items():
        items[off[t]:off[t + 1]] = rng.permutation(V)[:L]
    lut = rng.permutation(V).astype(np.int32)
    case = _case(off, items, lut, V)
    ref = _reference(case)
    assert ref.T == n and all(ref.c[t] == L for t, L in rows_at.items())
    return case


FUSED_CASES = {
    "n0": lambda: _fused_sizes(0), "n1": lambda: _fused_sizes(1), "n255": lambda: _fused_sizes(255),
    "n256": lambda: _fused_sizes(256), "n257": lambda: _fused_sizes(257), "n513": lambda: _fused_sizes(513),
    "none_kept": _fused_none_kept, "empty_workgroups": _fused_empty_workgroups,
    "lengths": _fused_lengths, "mid_7_8_9_64": _fused_mid_counts, "mid_slots": _fused_mid_slots,
    "wg_tokens_4095_4096_4097": _fused_wg_tokens, "full_output": _fused_full_output,
    "F2_T64": lambda: _fused_blocks(2, 64), "F256_T65": lambda: _fused_blocks(256, 65),
    "F257_T128": lambda: _fused_blocks(257, 128), "F2048_T129": lambda: _fused_blocks(2048, 129),
    "F2049_no_layout": _fused_no_layout, "F512_blocks": _fused_two_blocks,
    "scan_block_chunks": _fused_block_scan_chunks, "scan_all_chunks": _fused_all_scan_chunks,
    "probe": _fused_probe,
}


def _excl(v):
    out = np.zeros(v.size + 1, np.int64)
    np.cumsum(v, out=out[1:])
    return out


def _layout_bases(cnt, T):
    nb, nbatch = cnt.shape[0], (T + 63) // 64
    ex = _excl(cnt.reshape(-1))
    return np.array([ex[b * T + 64 * q] for b in range(nb) for q in range(nbatch)], np.int64)


def _layout_dense(Bk, F1):
    """(cnt [nb, T], lr, base) of the blocked layout, from B[kept]."""
    T, nb = Bk.shape[0], (F1 + 255) // 256
    blocks = [Bk[:, 256 * b:256 * b + 256] for b in range(nb)]
    cnt = np.stack([blk.sum(1, dtype=np.int64) for blk in blocks]) if nb else np.zeros((0, T), np.int64)
    lr = np.concatenate([np.nonzero(blk)[1] for blk in blocks] + [np.zeros(0, np.int64)]).astype(np.uint8)
    return cnt, lr, _layout_bases(cnt, T)


def _layout_sparse(roff, ranks, F1):
    T, nb = roff.size - 1, (F1 + 255) // 256
    x = np.repeat(np.arange(T), np.diff(roff))
    b = ranks.astype(np.int64) >> 8
    cnt = np.bincount(b * T + x, minlength=nb * T).reshape(nb, T).astype(np.int64)
    lr = (ranks[np.lexsort((ranks, x, b))] & 255).astype(np.uint8)
    return cnt, lr, _layout_bases(cnt, T)


def _pairs_sparse(roff, ranks, F1):
    """Upper-triangle pair counts of short sorted rows: items d apart in one row, d = 1, 2, ..."""
    G = np.zeros((F1, F1), np.int64)
    x = np.repeat(np.arange(roff.size - 1), np.diff(roff))
    for d in range(1, int(np.diff(roff).max(initial=0))):
        same = x[:-d] == x[d:]
        np.add.at(G, (ranks[:-d][same], ranks[d:][same]), 1)
    return G


def _fused_reference(case):
    ref = _reference(case)
    if case.F1 <= 256 * prim.limits().kCmpMaxNB:
        ref.cnt, ref.lr, ref.base = (_layout_dense(ref.Bk, case.F1) if case.dense
                                     else _layout_sparse(ref.roff, ref.ranks, case.F1))
        ref.pairs = _gram(ref.Bk) if case.dense else _pairs_sparse(ref.roff, ref.ranks, case.F1)
    return ref


def _np_dmix64(z):
    # prep.hip dmix64 on uint64 arrays (wrapping arithmetic)
    z = z + np.uint64(0x9E3779B97F4A7C15)
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def _np_row_hash(roff, ranks):
    """(h1, h2) of prep.hip k_row_hash for every row, in uint64 arithmetic."""
    T = roff.size - 1
    lens = np.diff(roff)
    rk = ranks.astype(np.int64).astype(np.uint32).astype(np.uint64)
    a = np.full(T, 0x243F6A8885A308D3, np.uint64)
    b = np.full(T, 0x13198A2E03707344, np.uint64)
    with np.errstate(over="ignore"):
        for j in range(int(lens.max(initial=0))):
            live = lens > j
            r = rk[np.where(live, roff[:-1] + j, 0)] if rk.size else np.zeros(T, np.uint64)
            a = np.where(live, _np_dmix64(a ^ r), a)
            b = np.where(live, _np_dmix64(b + r * np.uint64(0xD6E8FEB86659FD93)), b)
        a = _np_dmix64(a ^ lens.astype(np.uint64))
    return (a >> np.uint64(1)).astype(np.int64), (b >> np.uint64(1)).astype(np.int64)


def _probe_reference(ref):
    nmax = min(ref.T, PROBE_ROWS)
    roff = ref.roff[:nmax + 1]
    sel = np.flatnonzero(np.diff(roff) <= 16)
    # rows of more than 16 items are not hashed: hash the short ones only (clip the others)
    sub_off = _excl(np.diff(roff)[sel])
    idx = np.repeat(roff[sel], np.diff(roff)[sel]) + (np.arange(sub_off[-1]) - np.repeat(sub_off[:-1], np.diff(roff)[sel]))
    h1, _ = _np_row_hash(sub_off, ref.ranks[idx])
    return int(sel.size), int(np.unique(h1 & (prim.limits().kProbeBits - 1)).size)


@pytest.mark.parametrize("name", list(FUSED_CASES))
def test_fused_reference_invariants(name):
    """The builders and the numpy reference alone: rows ascending, roff[-1] == B[kept].sum(),
    the layout's segments tile [0, nnz) exactly once, sparse and dense references agree."""
    case = FUSED_CASES[name]()
    ref = _fused_reference(case)
    T, nnz = ref.T, ref.nnz
    assert (np.diff(ref.kept) > 0).all() and (ref.c[ref.kept] >= 2).all() and ref.hist.sum() == T
    assert ref.ranks.size == nnz and ref.roff[0] == 0
    if case.dense:
        assert nnz == int(ref.Bk.sum(dtype=np.int64))
        if case.n <= 1 << 18:
            sp = _reference(case, dense=False)
            assert all(np.array_equal(getattr(sp, k), getattr(ref, k)) for k in ("c", "kept", "roff", "ranks", "hist"))
    x = np.repeat(np.arange(T), np.diff(ref.roff))
    assert ((np.diff(ref.ranks) > 0) | (np.diff(x) > 0)).all()          # ranks ascend inside every row
    if case.F1 > 256 * prim.limits().kCmpMaxNB:
        return
    nb, nbatch = ref.cnt.shape[0], (T + 63) // 64
    assert ref.lr.size == nnz and ref.base.size == nb * nbatch and np.array_equal(ref.cnt.sum(0), np.diff(ref.roff))
    # segment (b, q) = [base, base + the block-b items of batch q): in order, end to start
    pad = np.zeros((nb, nbatch * 64 - T), np.int64)
    seg = np.concatenate([ref.cnt, pad], 1).reshape(nb, nbatch, 64).sum(2).reshape(-1)
    assert np.array_equal(ref.base, _excl(seg)[:-1]) and int(seg.sum()) == nnz
    if case.dense and T <= 1 << 12:
        sp = _layout_sparse(ref.roff, ref.ranks, case.F1)
        assert all(np.array_equal(u, v) for u, v in zip(sp, (ref.cnt, ref.lr, ref.base)))
        assert np.array_equal(_pairs_sparse(ref.roff, ref.ranks, case.F1), ref.pairs)
    if name == "probe":
        n, filled = _probe_reference(ref)
        assert n == PROBE_ROWS - 2 and filled < n


@pytest.mark.parametrize("dev", GPU)
@pytest.mark.parametrize("name", list(FUSED_CASES))
def test_compress_rows_fused(name, dev):
    case = FUSED_CASES[name]()
    ref = _fused_reference(case)
    F1, T, nnz = case.F1, ref.T, ref.nnz
    probe = {} if name == "probe" else None
    kept, roff, ranks, hist, layout = ops.compress_rows(_t(case.off, dev), _t(case.items, dev), _t(case.lut, dev), F1,
                                                        probe=probe)
    assert kept.dtype == torch.int32 and roff.dtype == torch.int64 and ranks.dtype == torch.int32
    assert np.array_equal(kept.cpu().numpy(), ref.kept)
    assert np.array_equal(roff.cpu().numpy(), ref.roff)
    assert np.array_equal(ranks.cpu().numpy(), ref.ranks)
    assert np.array_equal(np.asarray(hist), ref.hist)
    if probe is not None:
        want_n, want_filled = _probe_reference(ref)
        assert (probe["n"], probe["filled"]) == (want_n, want_filled)
    if F1 > 256 * prim.limits().kCmpMaxNB or case.n == 0:
        assert layout is None
        return
    nb, nbatch = (F1 + 255) // 256, (T + 63) // 64
    assert ref.cnt.max(initial=0) < 256
    cnt = layout.cnt.cpu().numpy()
    assert cnt.dtype == np.uint8 and np.array_equal(cnt[:nb * T], ref.cnt.reshape(-1).astype(np.uint8))
    assert not cnt[nb * T:].any()                                   # the pair kernel's read-ahead padding
    # the layout holds below 256 items per kept row (pair_counts_horizontal drops it otherwise)
    assert ref.c.max(initial=0) < 256
    assert np.array_equal(layout.lr.cpu().numpy()[:nnz], ref.lr)
    base = layout.base.cpu().numpy()
    assert np.array_equal(base[:nb * nbatch], ref.base) and not base[nb * nbatch:].any()
    got = ops.pair_counts_horizontal(roff, ranks, None, F1, long_rows=False, bcnt=layout)
    assert got.shape == (F1, F1) and got.dtype == torch.int64
    assert np.array_equal(got.cpu().numpy(), ref.pairs)


# ---------------------------------------------------------------------------
# 4. row_hash: k_row_hash / fa_cpu_row_hash
# ---------------------------------------------------------------------------
def _hash_rows():
    rng = np.random.default_rng(5000)
    top = 2 ** 31 - 1
    rows = [[0], [top], [0, top], [5, 9], [5, 9, 11], [5, 9], np.sort(rng.choice(1000, 16, replace=False)),
            np.sort(rng.choice(1000, 17, replace=False)), np.sort(rng.choice(5000, 300, replace=False)), [9, 5]]
    rows.append(np.concatenate([rows[8], [top]]))
    return rows


@pytest.mark.parametrize("dev", BOTH)
def test_row_hash(native, dev):
    rows = _hash_rows()
    roff, ranks = _pack(rows)
    assert sorted(set(np.diff(roff))) == [1, 2, 3, 16, 17, 300, 301]
    w1, w2 = _np_row_hash(roff, ranks)
    h1, h2 = ops.row_hash(_t(roff, dev), _t(ranks, dev))
    assert h1.dtype == torch.int64 and h2.dtype == torch.int64
    assert np.array_equal(h1.cpu().numpy(), w1) and np.array_equal(h2.cpu().numpy(), w2)
    assert (w1 >= 0).all() and (w2 >= 0).all()
    # equal sets give equal hashes; a row and its one-item extension, or its reversal, differ
    assert (w1[3], w2[3]) == (w1[5], w2[5])
    assert w1[3] != w1[4] and w2[3] != w2[4] and w1[8] != w1[10] and w2[8] != w2[10] and w1[3] != w1[9]


# ---------------------------------------------------------------------------
# 5. build_bitmaps: the wave build of count.hip (k_build_bitmaps_w) and k_build_bitmaps
# ---------------------------------------------------------------------------
BM_TILE = 8192           # primitives.py bitmap_geometry: WT = 2^clamp(log2(8192 // F1), 2, 5), R = min(F1, 8192 // WT)
BM_WT = {1: 32, 256: 32, 257: 16, 512: 16, 1024: 8, 1025: 4, 2048: 4, 2049: 4}


def _pack_bits(cols_by_rank, Wp):
    """[F1, ncols] 0/1 -> int64 [F1, Wp], bit c & 63 of word c >> 6, zero padding."""
    F1, ncols = cols_by_rank.shape
    bits = np.zeros((F1, Wp * 64), np.uint8)
    bits[:, :ncols] = cols_by_rank
    return np.packbits(bits, axis=1, bitorder="little").view(np.int64).reshape(F1, Wp)


@functools.lru_cache(maxsize=None)
def _bm_rows(F1):
    """64 WT + 1 rows over F1 items: about five items per row, rows of one item and of more
    than 64 items, and one 64-row group (rows 64..127) whose ranks exceed two 64-rank windows."""
    rng = np.random.default_rng(6000 + F1)
    T = 64 * BM_WT[F1] + 1
    B = (rng.random((T, F1)) < min(0.5, 5.0 / F1)).astype(np.uint8)
    # no empty row: compressed rows hold at least one item, and the wave build relies on it
    # (fa_hip.h window_starts: "rows non-empty, so starts are distinct"); at F1 = 1 every row
    # is therefore the single item
    B[np.arange(T), rng.integers(0, F1, T)] = 1
    B[3] = 0
    B[3, F1 - 1] = 1
    assert (B.sum(1) >= 1).all()
    if F1 > 64:
        B[5, rng.choice(F1, 70, replace=False)] = 1
        B[70, rng.choice(F1, min(F1, 200), replace=False)] = 1
        assert B[5].sum() > 64 and B[64:128].sum() > 128
    if F1 == 2049:
        B[7, [2047, 2048]] = 1
    B[0, 0] = B[T - 1, F1 - 1] = B[T - 1, 0] = 1
    return B


def _bm_ncols(F1):
    wt = BM_WT[F1]
    return sorted({1, 63, 64, 65, 64 * wt - 1, 64 * wt, 64 * wt + 1})


BM_PLAIN = [(F1, nc) for F1 in (1, 256, 257, 512, 1024, 1025, 2048, 2049) for nc in _bm_ncols(F1)]


def _bm_geometry_checks(F1, ncols, wave):
    W, Wp, WT, R = prim.bitmap_geometry(F1, ncols)
    assert WT == BM_WT[F1] and R == min(F1, BM_TILE // WT) and Wp % 64 == 0 and W == (ncols + 63) // 64
    # fa_hip_build_bitmaps takes the wave build when every rank's row fits one tile: R >= F1
    # (and F1 * WT * 8 bytes of LDS <= 64 KiB, count.hip fa_hip_build_bitmaps_wave)
    assert (R >= F1 and F1 * WT * 8 <= 64 * 1024) == wave
    return W, Wp


@pytest.mark.parametrize("dev", BOTH)
@pytest.mark.parametrize("F1,ncols", BM_PLAIN)
def test_build_bitmaps(native, F1, ncols, dev):
    B = _bm_rows(F1)[:ncols]
    W, Wp = _bm_geometry_checks(F1, ncols, wave=F1 <= 2048)
    want = _pack_bits(B.T, Wp)
    roff, ranks = _csr(B)
    roff, ranks = _t(roff, dev), _t(ranks, dev)
    bm, gotW = ops.build_bitmaps(roff, ranks, None, ncols, F1)
    assert gotW == W and bm.shape == (F1, Wp) and bm.dtype == torch.int64
    assert np.array_equal(bm.cpu().numpy(), want)
    if dev == "cuda" and prim.blocked_bitmaps_ok(None, F1, ncols):
        blk, _ = ops.build_bitmaps(roff, ranks, None, ncols, F1, blocked=True)
        assert torch.equal(blk.cpu(), prim.to_blocked(torch.from_numpy(want)))
    elif dev == "cuda":
        assert F1 == 2049


def _bm_src(rng, T, ncols):
    """Weight-class layout: repeated rows and -1 padding columns."""
    src = rng.integers(0, T, ncols).astype(np.int32)
    src[rng.random(ncols) < 0.2] = -1
    src[0], src[-1] = T - 1, -1
    if ncols > 70:
        src[60:68] = 5                                             # one row in eight columns across a word
        src[1] = 0
    return src


@pytest.mark.parametrize("dev", BOTH)
@pytest.mark.parametrize("F1,ncols", [(257, 65), (257, 1025), (2049, 255), (2049, 257)])
def test_build_bitmaps_src(native, F1, ncols, dev):
    # src forces the thread-per-row kernel (k_build_bitmaps) at every F1
    B = _bm_rows(F1)
    rng = np.random.default_rng(6500 + F1 + ncols)
    src = _bm_src(rng, B.shape[0], ncols)
    assert (src < 0).any() and np.unique(src[src >= 0]).size < (src >= 0).sum()
    _, Wp = _bm_geometry_checks(F1, ncols, wave=F1 <= 2048)
    cols = np.where(src[:, None] >= 0, B[np.maximum(src, 0)], 0).astype(np.uint8)
    roff, ranks = _csr(B)
    bm, _ = ops.build_bitmaps(_t(roff, dev), _t(ranks, dev), _t(src, dev), ncols, F1)
    assert np.array_equal(bm.cpu().numpy(), _pack_bits(cols.T, Wp))


BM_MAPPED = [(k, with_src) for k in (1, 64, 65) for with_src in (False, True)]


def _bm_mapped(k):
    """300 items, k of them selected (first and last rank included when k > 1): item_map
    (rank -> output row, -1 = skip) and used (the selected ranks, ascending)."""
    rng = np.random.default_rng(6700 + k)
    B = _bm_rows(512)[:300, :300].copy()
    B[:, 299] |= B[:, 0] ^ (np.arange(300) % 3 == 0)
    B[np.arange(300), rng.integers(0, 300, 300)] = 1                # the cut left empty rows: none may be (see _bm_rows)
    assert (B.sum(1) >= 1).all()
    used = np.array([299]) if k == 1 else np.sort(np.concatenate([[0, 299], rng.choice(np.arange(1, 299), k - 2, replace=False)]))
    item_map = np.full(300, -1, np.int32)
    item_map[used] = np.arange(k, dtype=np.int32)
    return B, used.astype(np.int32), item_map


@pytest.mark.parametrize("k,with_src", BM_MAPPED)
def test_bitmap_mapped_reference_invariants(k, with_src):
    """The item_map builder and reference alone (the op is device-only)."""
    B, used, item_map = _bm_mapped(k)
    assert used.size == k and (np.diff(used) > 0).all() and (k == 1 or (used[0] == 0 and used[-1] == 299))
    assert np.array_equal(np.flatnonzero(item_map >= 0), used) and np.array_equal(item_map[used], np.arange(k))
    want = _pack_bits(B[:, used].T, 64)
    # every bit of the reference is a cell of B: column popcounts
    pop = np.array([bin(int(w) & (2 ** 64 - 1)).count("1") for w in want.reshape(-1)]).reshape(want.shape).sum(1)
    assert np.array_equal(pop, B[:, used].sum(0)) and B[:, used].any()


@pytest.mark.parametrize("dev", GPU)
@pytest.mark.parametrize("k,with_src", BM_MAPPED)
def test_build_bitmaps_item_map(k, with_src, dev):
    # without src the wave build maps ranks through item_map; an identity src forces k_build_bitmaps
    B, used, item_map = _bm_mapped(k)
    ncols = B.shape[0]
    roff, ranks = _csr(B)
    src = _t(np.arange(ncols, dtype=np.int32), dev) if with_src else None
    bm, W = ops.build_bitmaps(_t(roff, dev), _t(ranks, dev), src, ncols, k, item_map=_t(item_map, dev),
                              used=_t(used, dev))
    _, Wp, _, _ = prim.bitmap_geometry(k, ncols)
    assert bm.shape == (k, Wp) and np.array_equal(bm.cpu().numpy(), _pack_bits(B[:, used].T, Wp))


# ---------------------------------------------------------------------------
# 6. trim_rows: k_trim_scan_count / k_trim_emit (64-row waves over 64-rank windows)
# ---------------------------------------------------------------------------
# kTrimAliveLds: alive flags in LDS up to F1 = 32768


def _rows_dense(rng, lens, F1):
    B = np.zeros((len(lens), F1), np.uint8)
    for x, L in enumerate(lens):
        B[x, rng.choice(F1, int(L), replace=False)] = 1
    return B


def _trim_sizes(T):
    rng = np.random.default_rng(7000 + T)
    B = _rows_dense(rng, rng.integers(1, 12, T), 100)
    return B, (rng.random(100) < 0.6).astype(np.int8)


def _trim_groups():
    # 64-row groups of 255, 256, 257, 511, 512, 513 and 1100 ranks, one row of 200 items among
    # 1-item rows, 64-item rows aligned to the windows, a group and then a whole workgroup
    # (256 rows) in which nothing survives, and a last partial group
    rng = np.random.default_rng(7100)
    F1 = 300
    alive = np.zeros(F1, np.int8)
    alive[rng.choice(280, 150, replace=False)] = 1                  # ranks 280.. are dead
    lens = [_group_lens(rng, t, nonempty=True) for t in (255, 256, 257, 511, 512, 513, 1100)]
    single = np.ones(64, np.int64)
    single[20] = 200
    lens += [single, np.full(64, 64)]
    B = _rows_dense(rng, np.concatenate(lens), F1)
    dead = np.zeros((64 + 256, F1), np.uint8)
    for x in range(dead.shape[0]):
        dead[x, 280 + rng.choice(20, 1 + x % 5, replace=False)] = 1
    B = np.concatenate([B, dead[:64], _rows_dense(rng, rng.integers(1, 9, 64 * 2), F1), dead[64:],
                        _rows_dense(rng, rng.integers(1, 30, 37), F1)])
    tot = [int(B[64 * g:64 * g + 64].sum()) for g in range(9)]
    assert tot == [255, 256, 257, 511, 512, 513, 1100, 263, 4096] and (B.sum(1) >= 1).all()
    surv = (B & alive).sum(1)
    assert surv[64 * 9:64 * 10].max() == 0
    wg = np.flatnonzero([surv[r:r + 256].max() == 0 for r in range(0, B.shape[0] - 255, 256)])
    assert wg.size == 1 and B.shape[0] % 64 == 37
    return B, alive


def _trim_long():
    # rows keeping 254, 255, 256 and 300 items (the histogram clamps at bin 255)
    rng = np.random.default_rng(7200)
    F1 = 400
    alive = np.zeros(F1, np.int8)
    alive[:320] = 1
    B = _rows_dense(rng, rng.integers(1, 6, 70), F1)
    for x, k in zip((3, 20, 21, 66), (254, 255, 256, 300)):
        B[x] = 0
        B[x, rng.choice(320, k, replace=False)] = 1
        B[x, 320 + rng.choice(80, 30, replace=False)] = 1
    assert sorted((B & alive).sum(1))[-4:] == [254, 255, 256, 300]
    return B, alive


def _trim_wide(F1):
    # the alive table in LDS (F1 = 32768) and in global memory (32769), alive ranks 0 and F1 - 1
    rng = np.random.default_rng(7300 + F1)
    alive = (rng.random(F1) < 0.5).astype(np.int8)
    alive[0] = alive[F1 - 1] = 1
    alive[1] = alive[F1 - 2] = 0
    B = _rows_dense(rng, rng.integers(1, 40, 70), F1)
    alive[2] = alive[3] = 1
    for x, rk in enumerate([[0, F1 - 1], [1, F1 - 2, F1 - 1], [1], [0, 1], [0, F1 - 2, F1 - 1], [0, 2, 3]]):
        B[x] = 0
        B[x, rk] = 1
    assert (B[:6] & alive).sum(1).tolist() == [2, 1, 0, 1, 2, 3]
    assert (F1 <= prim.limits().kTrimAliveLds) == (F1 == 32768)
    return B, alive


TRIM_CASES = {f"T{T}": functools.partial(_trim_sizes, T) for T in (1, 63, 64, 65, 255, 256, 257)}
TRIM_CASES.update({"groups": _trim_groups, "long_rows": _trim_long,
                   "F32768_lds_alive": lambda: _trim_wide(32768), "F32769_global_alive": lambda: _trim_wide(32769)})


@pytest.mark.parametrize("dev", BOTH)
@pytest.mark.parametrize("weighted", [False, True], ids=["unit", "weights"])
@pytest.mark.parametrize("min_len", [1, 3])
@pytest.mark.parametrize("name", list(TRIM_CASES))
def test_trim_rows(native, name, min_len, weighted, dev):
    B, alive = TRIM_CASES[name]()
    T, F1 = B.shape
    assert (B.sum(1) >= 1).all()                                    # input rows are never empty
    A = B & alive.astype(np.uint8)[None, :]
    c = A.sum(1, dtype=np.int64)
    w = None
    if weighted:
        w = np.array([3, 0, 1, 7, 2], np.int32)[np.arange(T) % 5]    # weights with zeros
    keep = (c >= min_len) & (True if w is None else w > 0)
    if T >= 63:
        assert (c == min_len - 1).any() and (c == min_len).any()
    kept_ref = np.flatnonzero(keep)
    nroff_ref = _excl(c[kept_ref])
    roff, ranks = _csr(B)
    kept, nroff, nranks, nw, hist = ops.trim_rows(_t(roff, dev), _t(ranks, dev), _t(alive, dev), min_len,
                                                  None if w is None else _t(w, dev))
    assert np.array_equal(kept.cpu().numpy(), kept_ref.astype(np.int32))
    assert np.array_equal(nroff.cpu().numpy(), nroff_ref)
    assert np.array_equal(nranks.cpu().numpy(), np.nonzero(A[kept_ref])[1].astype(np.int32))
    assert (nw is None) if w is None else np.array_equal(nw.cpu().numpy(), w[kept_ref])
    assert np.array_equal(hist.cpu().numpy(), np.bincount(np.minimum(c[kept_ref], 255), minlength=256))


# ---------------------------------------------------------------------------
# 7. histogram: k_histogram (four LDS copies, one LDS copy, global atomics)
# ---------------------------------------------------------------------------
# kLdsBins: LDS bins up to V = 16384, four copies while 4 V <= 4096


@pytest.mark.parametrize("dev", BOTH)
@pytest.mark.parametrize("nnz", [0, 1, 3, 4, 4099])
@pytest.mark.parametrize("V", [1, 1024, 1025, 16384, 16385])
def test_histogram(native, V, nnz, dev):
    rng = np.random.default_rng(8000 + V + nnz)
    items = rng.integers(0, V, nnz).astype(np.int32)
    if nnz >= 3:
        items[:3] = [0, V - 1, V - 1]
    bins = prim.limits().kLdsBins
    assert (V * 4 <= bins // 4) == (V <= 1024) and (V <= bins) == (V <= 16384)
    got = ops.histogram(_t(items, dev), V)
    assert got.dtype == torch.int64 and np.array_equal(got.cpu().numpy(), np.bincount(items, minlength=V))


@pytest.mark.parametrize("dev", BOTH)
@pytest.mark.parametrize("V", [1024, 16384, 16385])
def test_histogram_unaligned_view(native, V, dev):
    # a view that starts 4 bytes off a 16-byte boundary: the scalar-load variant
    rng = np.random.default_rng(8100 + V)
    items = rng.integers(0, V, 4100).astype(np.int32)
    whole = torch.empty(items.size, dtype=torch.int32, device=dev)
    whole.copy_(torch.from_numpy(items))
    view = whole[1:]
    assert whole.data_ptr() % 16 == 0 and view.data_ptr() % 16 == 4 and view.is_contiguous()
    got = ops.histogram(view, V)
    assert np.array_equal(got.cpu().numpy(), np.bincount(items[1:], minlength=V))


@pytest.mark.parametrize("dev", BOTH)
@pytest.mark.parametrize("V", [5, 1025, 16385])
def test_histogram_one_id(native, V, dev):
    items = np.full(70001, V - 2, np.int32)
    got = ops.histogram(_t(items, dev), V)
    assert np.array_equal(got.cpu().numpy(), np.bincount(items, minlength=V))


@pytest.mark.parametrize("dev", BOTH)
def test_histogram_grid_cap(native, dev):
    # 2048 * 4096 + 7 tokens: the grid stops at 2048 workgroups (prep.hip fa_hip_histogram),
    # so every thread loops, and 7 tokens are left to the scalar tail
    rng = np.random.default_rng(8200)
    nnz, V = 2048 * 4096 + 7, 1000
    items = rng.integers(0, V, nnz).astype(np.int32)
    assert (nnz + 4095) // 4096 > 2048 and nnz % 4 == 3
    got = ops.histogram(_t(items, dev), V)
    assert np.array_equal(got.cpu().numpy(), np.bincount(items, minlength=V))
