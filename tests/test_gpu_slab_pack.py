"""The slab kernel under the thinner row padding (count.hip k_count_slab_rec<.., kPad>;
csrc/host/fa_slab.h: one 16-B pad slot per 2^s rows) and the tail rule that uses it
(gen.hip k_dl_decide / dl_tail, TUNING.dl_tail_bundle).

Kernel: hand-written piece records over dense 0/1 rows B[T, F1], so every shape is chosen
here -- the number of slab rows around the pad groups' edges, prefixes of 1 .. 13 ids (13:
the long-prefix records), a candidate present in every row of several slabs.  Every count
is compared by exact equality with numpy (AND of the columns, sum of the row weights) and
with the s = 0 kernel on the same records.  The accumulators start right behind the rows'
footprint, so a build or a reader that places a row elsewhere changes candidate counts.
Lane deal: the dealt plan holds the same records and counts the same.  Tail rule: the device
chain and post step against the host mirror, then mined runs against the C++ CPU miner."""
import functools

import numpy as np
import pytest
import torch

from fastapriori_amd.ops import primitives as prim
from test_gen_edges import bundle_case, run_bundle
from test_kernel_edges import _csr

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)


# ---- hand-written records ----------------------------------------------------------------
def _case(seed, n_used, T, ms=(1, 2, 3, 5, 12, 13), pieces=150, full_rows=False):
    """B [T, F1], the rank -> slab-row map (three ranks unused), pieces [(prefix rows, ext rows)]."""
    rng = np.random.default_rng(seed)
    F1 = n_used + 3
    used = np.sort(rng.choice(F1, n_used, replace=False))
    B = (rng.random((T, F1)) < 0.8).astype(np.int64)
    B[np.arange(T) % 4 < 2] = 1                       # planted full rows: long prefixes keep support
    B[B.sum(1) < 2, :2] = 1                           # the kernels rely on rows of >= 2 items
    if full_rows:
        B[:] = 1
    out = []
    for i in range(pieces):
        m = ms[i % len(ms)]
        pre = np.sort(rng.choice(n_used, m, replace=n_used < m))
        ext = rng.choice(n_used, 1 + (i * 5) % 8, replace=True)
        out.append((pre.tolist(), ext.tolist()))
    # the last slab row is a prefix and an extension of the last pieces, row 0 of the first
    out[0] = ([0], [n_used - 1, 0])
    out[-1] = ([n_used - 1], [0, n_used - 1])
    return B, used, out


def _records(pcs):
    """3 x int4 per piece (count.hip k_count_slab_rec) and gpre, the long prefixes' slab rows."""
    rec = np.zeros((len(pcs), 12), np.uint32)
    gpre, e0 = [], 0
    for i, (pre, ext) in enumerate(pcs):
        m, long_ = len(pre), len(pre) > 12
        rec[i, 0] = e0
        rec[i, 1] = len(ext) | (m << 8) | (int(long_) << 16)
        ids = np.zeros(4, np.uint32)
        ids[:min(m, 4)] = pre[:4]
        rec[i, 2], rec[i, 3] = ids[0] | (ids[1] << 16), ids[2] | (ids[3] << 16)
        x = np.zeros(8, np.uint32)
        x[:len(ext)] = ext
        rec[i, 4:8] = x[0::2] | (x[1::2] << 16)
        if long_:
            rec[i, 8] = len(gpre)
            gpre += pre
        else:
            p = np.zeros(8, np.uint32)
            p[:max(m - 4, 0)] = pre[4:]
            rec[i, 8:12] = p[0::2] | (p[1::2] << 16)
        e0 += len(ext)
    return rec.view(np.int32), np.array(gpre + [0], np.int32), e0


def _reference(B, used, pcs, wcol=None):
    w = np.ones(B.shape[0], np.int64) if wcol is None else wcol
    ref = []
    for pre, ext in pcs:
        has = B[:, used[pre]].all(1)
        ref += [int((w * (has & (B[:, used[e]] > 0))).sum()) for e in ext]
    return np.array(ref, np.int64)


def _launch(B, used, pcs, sw, pad, accb, build="contig", wword=None, n_wg=None, ncols=None):
    """One fa_hip_count_slab_rec_cls launch at layout (sw, pad) over the first ncols rows."""
    T, F1 = B.shape
    ncols = T if ncols is None else ncols
    n_used = len(used)
    rec, gpre, C = _records(pcs)
    item_map = np.full(F1, -1, np.int32)
    item_map[used] = np.arange(n_used, dtype=np.int32)
    src = bm = None
    if build == "src":
        perm = np.random.default_rng(ncols).permutation(T)[:ncols].astype(np.int32)
        perm[::97] = -1                               # empty columns
        Bc = np.where((perm >= 0)[:, None], B[np.maximum(perm, 0)], 0)
        src = torch.from_numpy(perm).to(DEV)
        roff, ranks = _csr(B)
    else:
        Bc = B[:ncols]
        roff, ranks = _csr(Bc)
    if build == "bitmap":
        W = (ncols + 63) // 64
        Wp = (W + 63) // 64 * 64
        bits = np.zeros((n_used, Wp * 64), np.uint8)
        bits[:, :ncols] = Bc[:, used].T
        bm = torch.from_numpy(np.packbits(bits, axis=1, bitorder="little").view(np.int64).copy()).to(DEV)
    roff, ranks = roff.to(DEV), ranks.to(DEV)
    d_rec, d_gpre, d_map = (torch.from_numpy(a.copy()).to(DEV) for a in (rec, gpre, item_map))
    out = torch.zeros(C, dtype=torch.int32, device=DEV)
    layout = prim.slab_layout(sw, pad)
    mode, nacc = prim._slab_acc_mode(accb, wword is not None, C)
    contig = build == "contig"
    lds = prim.slab_rows_bytes(sw, pad, n_used) + ((nacc + 3) & ~3) * 4 + (prim.slab_map_lds(F1) if contig else 0)
    assert lds <= 64 * 1024
    nslabs = ((ncols + 63) // 64 + sw - 1) // sw
    prim._hip_call("fa_hip_count_slab_rec_cls", prim._p(roff), prim._p(ranks), prim._p(src), ncols, prim._p(d_map), F1,
                   n_used, prim._p(d_gpre), prim._p(d_rec), len(pcs), C, prim._p(wword), out.data_ptr(), layout,
                   min(nslabs, n_wg or nslabs), prim._p(bm), Wp if bm is not None else 0, prim._stream(ranks), None,
                   None, mode)
    torch.cuda.synchronize()
    return out.cpu().numpy().astype(np.int64), Bc


@functools.lru_cache(maxsize=None)
def _edge_case(n_used):
    return _case(n_used, n_used, 16 * 64 * 2 + 70)        # two slabs and a part at width 16; four and a part at 8


@pytest.mark.parametrize("n_used", [1, 3, 4, 5, 8, 9, 63, 64, 65])
@pytest.mark.parametrize("sw", [8, 16])
def test_pad_group_edges(sw, n_used):
    # the rows around every pad group's edge (groups of 2, 4 and 8 rows), byte counters; the last
    # row is read as a prefix and as an extension, counter 0 sits behind its footprint
    B, used, pcs = _edge_case(n_used)
    ref = _reference(B, used, pcs)
    base, _ = _launch(B, used, pcs, sw, 0, 1)
    assert np.array_equal(base, ref) and ref.max() > 255
    for pad in (1, 2, 3):
        got, _ = _launch(B, used, pcs, sw, pad, 1)
        assert np.array_equal(got, ref), (pad,)


@functools.lru_cache(maxsize=None)
def _build_case():
    return _case(7, 37, 16 * 64 * 2 + 70)


@pytest.mark.parametrize("accb", [1, 2, 4])
@pytest.mark.parametrize("build", ["contig", "src", "bitmap"])
@pytest.mark.parametrize("sw", [8, 16])
def test_every_build_and_accumulator(sw, build, accb):
    B, used, pcs = _build_case()
    for pad in (1, 2, 3):
        got, Bc = _launch(B, used, pcs, sw, pad, accb, build)
        assert np.array_equal(got, _reference(Bc, used, pcs)), (pad,)
    base, Bc = _launch(B, used, pcs, sw, 0, accb, build)
    assert np.array_equal(base, _reference(Bc, used, pcs))


@pytest.mark.parametrize("sw", [8, 16])
def test_column_counts_around_one_slab(sw):
    B, used, pcs = _case(11, 21, 64 * sw + 1, pieces=40)
    for ncols in (1, 63, 64, 65, 64 * sw - 1, 64 * sw + 1):
        ref = _reference(B[:ncols], used, pcs)
        for pad in (0, 1, 2, 3):
            got, _ = _launch(B, used, pcs, sw, pad, 1, ncols=ncols)
            assert np.array_equal(got, ref), (ncols, pad)


@pytest.mark.parametrize("build", ["contig", "src", "bitmap"])
def test_weighted_rows(build):
    B, used, pcs = _build_case()
    T = B.shape[0]
    w = np.random.default_rng(3).integers(1, 9, (T + 63) // 64).astype(np.int32)   # one weight per 64-column word
    wt = torch.from_numpy(w).to(DEV)
    wcol = np.repeat(w, 64)[:T].astype(np.int64)
    for sw, pad in ((16, 2), (8, 1), (16, 3)):
        got, Bc = _launch(B, used, pcs, sw, pad, 1, build, wword=wt)
        assert np.array_equal(got, _reference(Bc, used, pcs, wcol)), (sw, pad)


@pytest.mark.parametrize("accb", [1, 2])
def test_more_slabs_than_workgroups_and_full_slabs(accb):
    # every row holds every item: each candidate gains 1024 per 16-word slab, nine slabs under
    # two workgroups -- a byte counter spills on every add, a u16 one carries 4,096 and more
    B, used, pcs = _case(5, 9, 16 * 64 * 9, ms=(1, 2, 12, 13), pieces=70, full_rows=True)
    ref = _reference(B, used, pcs)
    assert (ref == B.shape[0]).all()
    for pad in (1, 2, 3):
        got, _ = _launch(B, used, pcs, 16, pad, accb, n_wg=2)
        assert np.array_equal(got, ref), (pad,)


# ---- lane deal ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def dl_state():
    return prim.DeviceLevelState(DEV)


def _plan_records(plan, pieces):
    return plan["rec"][:12 * pieces].cpu().numpy().view(np.uint32).reshape(-1, 12)


@pytest.mark.parametrize("pad", [0, 1, 2, 3])
def test_lane_deal_under_each_layout(dl_state, tune, pad):
    # lat40: whole 256-record windows of the lane deal.  The deal only moves records inside a
    # window, whatever column function it was given: the same multiset per window, equal counts
    S, K = dl_state, prim.dl()
    Fb, ch = bundle_case("lat40_F70", 1)
    c, P0 = run_bundle(S, Fb, ch, 1, 1.0)
    C, n_used = len(ch[0][2]), int(c[K.kDlNUsed])
    T = 2100
    rng = np.random.default_rng(3)
    B = (rng.random((T, Fb)) < 0.3).astype(np.int64)
    B[np.ix_(np.arange(T) % 8 < 2, np.unique(ch[0][0]))] = 1
    B[B.sum(1) < 2, :2] = 1
    ref = B.astype(bool)[:, ch[0][2]].all(2).sum(0).astype(np.int64)
    roff, ranks = _csr(B)
    roff, ranks = roff.to(DEV), ranks.to(DEV)
    S.rows_hint = T
    got, recs = {}, {}
    try:
        for deal in (False, True):
            tune(lane_deal_min_rows=0 if deal else -1)
            plan = prim.dl_plan(S, 1, Fb, n_used, C, prim.dl_lds_budget(Fb), DEV, accb=1.0, pad=pad)
            assert plan["sw"] == 16 and plan["pad"] == pad
            got[deal] = prim.dl_count(S, plan, roff, ranks, None, T, Fb, None).cpu().numpy().astype(np.int64)
            pieces = int(S.ctl[K.kDlPieces].item())
            recs[deal] = _plan_records(plan, pieces)
            assert prim.LAST_LEVEL_PLAN["pad"] == pad
    finally:
        S.rows_hint = 0
    assert np.array_equal(got[False], ref) and np.array_equal(got[True], ref)
    a, b = recs[False], recs[True]
    assert a.shape == b.shape and a.shape[0] >= 512 and not np.array_equal(a, b)      # the deal moved records
    for w0 in range(0, a.shape[0], 256):
        key = lambda r: sorted(map(tuple, r[w0:w0 + 256].tolist()))                    # noqa: E731
        assert key(a) == key(b), w0
    del P0


# ---- the device rule ---------------------------------------------------------------------
def _chain(S, max_levels, growth, lds, tail, tail_levels=0):
    """fa_hip_dl_level0 + fa_hip_dl_more with the post step over lat13_F70 (13 ranks' pairs:
    C(13, k) candidates at level k, 8,100 in all, then none), planning only: with no rows
    (ncols 0) the post step's count is a no-op.  -> (control block, levels' C, layout, cap)."""
    Fb, ch = bundle_case("lat13_F70")
    P0 = torch.from_numpy(np.ascontiguousarray(ch[0][0], dtype=np.int32)).to(DEV)
    n, m0 = P0.shape
    c_bound = int(lds // 4)
    b = S.post_buffers(Fb, int(lds), n + int(lds), 0)       # (room for a packed bundle: a byte per candidate)
    P = S.post
    P.item_map, P.rec, P.part, P.out = (b[k].data_ptr() for k in ("item_map", "rec", "part", "out"))
    P.rec_cap, P.part_cap, P.out_cap = b["c_cap"], b["part"].numel(), b["c_cap"]
    P.gpre, P.gpre_cap = b["gpre"].data_ptr(), b["gpre"].numel()
    P.roff = P.ranks = P.src = P.wword = None
    P.ncols, P.lds_kernel, P.lds_budget = 0, float(lds + prim.slab_map_lds(Fb)), float(lds)
    P.accb = 1.0
    P.c1 = P.alive = P.len_hist = None
    P.T = P.nnz = P.trim_ok = 0
    P.trim_min_rows, P.k = 1 << 40, m0 + 1
    st = torch.cuda.current_stream(DEV).cuda_stream
    c = prim.dl_bundle_gen(S, P0.data_ptr(), None, n, n, m0, Fb, c_bound, lds, growth, max_levels, st, post=True,
                           accb=4.0, tail_accb=1.0 if tail else 0.0, tail_levels=tail_levels)
    torch.cuda.synchronize()
    L = int(c[prim.dl().kDlLevels])
    assert int(P.done) >= 1 and int(P.C) == int(S.desc["C"][:L].sum())
    return c, [int(x) for x in S.desc["C"][:L]], prim.slab_layout_split(int(P.sw)), int(P.cap), float(P.accb)


# lds bytes: the 8,100 candidates of the whole chain fit one packed pass of 13 rows at no pad
# shift (9,790), at s = 3, 2, 1 only, and with every row padded (9,980); the unpacked rule
# takes levels 3-5 (2,288 candidates in u32 at width 4) everywhere
@pytest.mark.parametrize("lds", [9790, 9800, 9840, 9880, 9980])
@pytest.mark.parametrize("max_levels,tail_levels", [(31, 0), (5, 5), (5, 0)])
def test_device_rule_matches_the_host_mirror(dl_state, lds, max_levels, tail_levels):
    S, K = dl_state, prim.dl()
    growth = 5.0
    _, ch = bundle_case("lat13_F70")
    Cs_all = [len(cand) for _, _, cand in ch]
    assert sum(Cs_all) == 8100 and Cs_all[-1] == 0 and max(Cs_all) <= lds // 4
    c_off, Cs_off, lay_off, cap_off, accb_off = _chain(S, max_levels, growth, lds, False)
    c, Cs, lay, cap, accb = _chain(S, max_levels, growth, lds, True, tail_levels)
    n_used = int(c[K.kDlNUsed])
    assert n_used == 13 and Cs_off == Cs_all[:3]
    # the chain's acceptance replayed: a level joins while the unpacked rule or the packed one holds the total
    tot, Lc = Cs_all[0], 1
    while Lc < max_levels and Cs_all[Lc] > 0 and Cs_all[Lc] <= growth * Cs_all[Lc - 1]:
        t = tot + Cs_all[Lc]
        sw_p, cap_p, _ = prim.slab_pack_width(n_used, t, lds, 1)
        if not (t <= prim.slab_width(n_used, t, lds, 4)[1] or (sw_p == 16 and cap_p >= t)):
            break
        tot, Lc = t, Lc + 1
    stopped_empty = Lc < max_levels and Cs_all[Lc] == 0
    ends = stopped_empty or (tail_levels > 0 and Lc == tail_levels)
    want = prim.dl_tail_plan(Cs_all[:Lc], n_used, lds, 4, 1, ends)
    assert (len(Cs), lay[0], lay[1], cap) == want, (Cs, lay, cap, want)
    assert bool(c[K.kDlEmpty]) == (stopped_empty and len(Cs) == Lc)
    if len(Cs) == Lc and Lc > 3:
        # kept whole: width 16, bytes, the smallest pad shift that holds the total
        assert lay[0] == 16 and accb == 1.0 and cap >= sum(Cs) == int(c[K.kDlTotal])
        assert lay[1] == {9800: 3, 9840: 2, 9880: 1}.get(lds, 0) or sum(Cs) < 8100
    else:
        # cut back: the bundle, its layout and accumulators are the run's with the rule off
        assert (Cs, lay, cap, accb) == (Cs_off, lay_off, cap_off, accb_off)
        assert int(c[K.kDlTotal]) == sum(Cs) and int(c[K.kDlLastC]) == Cs[-1] and int(c[K.kDlLevels]) == 3
    # whole: the chain that runs out of candidates where its 8,100 fit, the five levels
    # (5,720) that reach --max-level at every budget here; never the chain cut at five levels
    assert (len(Cs) > 3) == (lds > 9790 if max_levels == 31 else tail_levels == 5)


# ---- mined runs --------------------------------------------------------------------------
MS = 0.001
# the unpacked rule's u32 capacity at width 8 holds levels 3-4 of the 40,000-row shard (932 used
# items; 8,798 + 7,815 candidates) and not level 5 with them; all 26,940 candidates of levels
# 3-10 fit one packed pass in bytes at s = 2 (152,000 - 123,024 = 28,976; s = 1: 25,248)
LDS_FITS = 152000
# no pad shift holds the 20,000-row shard's 26,683 candidates (936 used items: 140,000 - 121,680
# = 18,320), but the packed rule lets the chain run past the unpacked rule's stop after level 3
LDS_SHORT = 140000


@functools.lru_cache(maxsize=None)
def _mined(n):
    from fastapriori_amd.models.apriori import FastApriori, MinerConfig
    from fastapriori_amd.parallel.comm import Comm
    from fastapriori_amd.utils.io import generate_shard
    from fastapriori_amd.utils.metrics import Logger
    cpu = generate_shard(n, Comm(), "cpu", 10.0, 4.0, 2000, 1000, 4)
    ref = FastApriori(MS, config=MinerConfig(min_support=MS), logger=Logger(0, enabled=False)).run(cpu)
    return cpu, ref


def _run(cpu, max_level=0):
    from fastapriori_amd.models.apriori import FastApriori, MinerConfig
    from fastapriori_amd.utils.metrics import Logger
    m = FastApriori(MS, config=MinerConfig(min_support=MS, max_level=max_level), logger=Logger(0, enabled=False))
    res = m.run(cpu.to(DEV))
    assert "fallbacks" not in m.stats, m.stats
    return res, m.stats


def _same(got, ref, levels=None):
    n = len(ref.levels) if levels is None else levels
    assert len(got.levels) == n
    for x, y in zip(got.levels, ref.levels[:n]):
        assert np.array_equal(x, y)
    for x, y in zip(got.counts, ref.counts[:n]):
        assert np.array_equal(x, y)


def test_mined_tail_in_one_bundle(tune):
    cpu, ref = _mined(40_000)
    nF1, deep = len(ref.levels[0]), len(ref.levels)
    assert deep >= 8 and max(int(np.max(c)) for c in ref.counts[2:]) > 255
    tune(dl_acc8_min_rows=0, slab_lds_bytes=LDS_FITS + prim.slab_map_lds(nF1), dl_tail_bundle=False)
    got0, st0 = _run(cpu)
    tune(dl_tail_bundle=True)
    got, st = _run(cpu)
    print(st0["device_bundle_shapes"], st["device_bundle_shapes"], st["device_bundle_pads"])
    assert st0["device_bundles"] >= 2 and st0["device_bundle_shapes"][0][:2] == (3, 2)
    assert all(p == 0 for p in st0["device_bundle_pads"])
    # one bundle: every level from 3 on, 16-word slabs, bytes, one pad slot per four rows
    info = st["level_info"]
    assert st["device_bundles"] == 1 and sorted(info) == [3], st
    k0, L, C, used, sw, accb = st["device_bundle_shapes"][0]
    assert (k0, sw, accb) == (3, 16, 1) and L >= deep - 2 and st["device_bundle_pads"] == [2]
    assert info[3] == dict(kernel="slab_dev", bundled=L, C=C, used=used, sw=16, pad=2, acc_bytes=1)
    assert prim.slab_pack_width(used, C, LDS_FITS, 1) == (16, LDS_FITS - prim.slab_rows_bytes(16, 2, used), 2)
    _same(got, ref)
    _same(got0, ref)
    assert got.as_dict() == ref.as_dict()
    # --max-level inside the tail: the bundle ends the run there, one packed pass again
    got_c, st_c = _run(cpu, max_level=deep - 1)
    assert st_c["device_bundles"] == 1 and st_c["device_bundle_shapes"][0][1] == deep - 3
    assert st_c["device_bundle_pads"][0] >= 1
    _same(got_c, ref, deep - 1)


def test_mined_tail_that_does_not_fit_is_cut_as_before(tune):
    cpu, ref = _mined(20_000)
    nF1 = len(ref.levels[0])
    tune(dl_acc8_min_rows=0, slab_lds_bytes=LDS_SHORT + prim.slab_map_lds(nF1), dl_tail_bundle=False)
    got0, st0 = _run(cpu)
    tune(dl_tail_bundle=True)
    got, st = _run(cpu)
    print(st0["device_bundle_shapes"], st["device_bundle_shapes"])
    assert st["device_bundle_shapes"] == st0["device_bundle_shapes"] and st["device_bundles"] >= 2
    assert st["device_bundle_shapes"][0][:2] == (3, 1)        # (the packed test alone would take level 4 too)
    assert all(p == 0 for p in st["device_bundle_pads"]) and st["level_info"] == st0["level_info"]
    for k in ("device_multipass", "device_levels", "device_bitmap_levels"):
        assert st.get(k) == st0.get(k), k
    _same(got, ref)
    assert got.as_dict() == got0.as_dict() == ref.as_dict()
    # below TUNING.dl_acc8_min_rows rows the rule is off
    tune(slab_lds_bytes=LDS_FITS + prim.slab_map_lds(nF1), dl_acc8_min_rows=1 << 20)
    got1, st1 = _run(cpu)
    assert st1["device_bundles"] >= 2 and all(p == 0 for p in st1["device_bundle_pads"])
    _same(got1, ref)


def _rank(n, tune_spec):
    from fastapriori_amd.models.apriori import FastApriori, MinerConfig
    from fastapriori_amd.parallel.comm import init_comm, shutdown_comm
    from fastapriori_amd.tuning import TUNING
    from fastapriori_amd.utils.io import generate_shard
    from fastapriori_amd.utils.metrics import Logger
    TUNING.apply(tune_spec)
    comm = init_comm("cuda")
    try:
        sh = generate_shard(n, comm, comm.device, 10.0, 4.0, 2000, 1000, seed=4)
        m = FastApriori(MS, comm, MinerConfig(min_support=MS), Logger(comm.rank, enabled=False))
        c0 = comm.comm_calls
        res = m.run(sh)
        return dict(sets=res.as_dict(), bundles=int(m.stats.get("device_bundles", 0)),
                    pads=m.stats.get("device_bundle_pads"), calls=comm.comm_calls - c0, world=comm.world_size,
                    levels=[s[:3] for s in m.stats["device_bundle_shapes"]], rows=int(sh.n_lines))
    finally:
        shutdown_comm(comm)


def test_two_ranks_match_one():
    from fastapriori_amd.parallel.launch import spawn_local
    _, ref = _mined(40_000)
    spec = f"dl_acc8_min_rows=0,slab_lds_bytes={LDS_FITS + prim.slab_map_lds(len(ref.levels[0]))}"
    one = spawn_local(_rank, 1, 40_000, spec, env={"FA_DIST_BACKEND": "gloo"})[0]
    assert one["bundles"] == 1 and one["pads"] == [2] and one["sets"] == ref.as_dict()
    for o in spawn_local(_rank, 2, 40_000, spec, env={"FA_DIST_BACKEND": "gloo"}):
        assert o["world"] == 2 and o["sets"] == one["sets"]
        assert o["bundles"] == 1 and o["pads"] == [2]
        assert o["calls"] <= 4 + o["bundles"], o


@pytest.mark.parametrize("on", [False, True], ids=["below", "at"])
def test_two_uneven_ranks_bundle_alike(on):
    # 40,001 rows: ranks of 20,000 and 20,001.  The rule's row threshold lies between the two
    # shards (and once at the smaller one): the decision follows the lines per rank, 20,000 on
    # both, never a rank's own shard, so both ranks cut the same bundles -- the same all-reduces
    from fastapriori_amd.parallel.launch import spawn_local
    _, ref = _mined(40_000)
    thr = 20_000 if on else 20_001
    spec = f"dl_acc8_min_rows={thr},slab_lds_bytes={LDS_FITS + prim.slab_map_lds(len(ref.levels[0]))}"
    one = spawn_local(_rank, 1, 40_001, spec, env={"FA_DIST_BACKEND": "gloo"})[0]
    outs = spawn_local(_rank, 2, 40_001, spec, env={"FA_DIST_BACKEND": "gloo"})
    assert sorted(o["rows"] for o in outs) == [20_000, 20_001] and min(o["rows"] for o in outs) < 20_001
    for o in outs:
        assert o["sets"] == one["sets"] and o["levels"] == outs[0]["levels"] and o["pads"] == outs[0]["pads"]
        assert o["calls"] <= 4 + o["bundles"], o
        assert (o["bundles"] == 1 and o["pads"][0] >= 1) if on else (o["bundles"] >= 2 and not any(o["pads"])), o
