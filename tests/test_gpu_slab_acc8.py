"""Single-writer byte accumulators of the slab kernel (count.hip k_count_slab_rec<.., 1>;
accb = 1 in csrc/host/fa_slab.h's terms).

Every count is compared, by exact equality over the whole output, with the u32 mode of the
same kernel and with the number of rows of a dense 0/1 matrix B[T, F1] that hold the
candidate, computed from B in numpy.  The shapes are the ones at which a byte counter can go
wrong: a partial last counter word, the four bytes of a word owned by different threads and
waves, sums that reach 255, pass it by one, or arrive as 256 and more in one add, one
workgroup that walks several all-ones slabs, every slab width and build, a divided piece
list, weighted rows (which must fall back to u32), and a small mined run.  The device plan's
pieces are read back and checked for the invariant the mode rests on (each candidate in
exactly one piece).
"""
import functools

import numpy as np
import pytest
import torch

from fastapriori_amd import ops
from fastapriori_amd.ops import _native
from fastapriori_amd.ops import primitives as prim
from test_gen_edges import bundle_case, accepted, run_bundle
from test_kernel_edges import SLAB_CASES, _csr, _slab_case, _support
from test_slab_acc8_rule import _groups, piece_ranges_partition

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
F1 = 96


def _rows(rng, T, dens=0.35):
    B = (rng.random((T, F1)) < dens).astype(np.int64)
    B[np.arange(T) % 8 < 2] = 1               # planted full rows: every candidate has support
    B[B.sum(1) < 2, :2] = 1                   # the kernels rely on rows of >= 2 items
    return B


def _level(B, prefix, ext_off, ext, accb, wword=None, src=None, ncols=None):
    roff, ranks = _csr(B)
    T = B.shape[0] if ncols is None else ncols
    got = ops.count_level(roff.to(DEV), ranks.to(DEV), src, T, F1, prefix, ext_off, ext, wword, kernel="slab",
                          accb=accb)
    assert got is not None and got.dtype == torch.int64
    return got.cpu().numpy(), dict(prim.LAST_LEVEL_PLAN)


@pytest.fixture
def one_wg():
    """One workgroup walks every slab (fa_hip_debug_slab_max_wg), so a counter lives across slabs."""
    hip = _native.hip()
    hip.fa_hip_debug_slab_max_wg(1)
    yield
    hip.fa_hip_debug_slab_max_wg(0)


# ---- counter words: C = 1, 2, 3, 5, 4k + 1; one extension per piece ---------------------
@pytest.mark.parametrize("sizes", [(1,), (2,), (3,), (1, 4), (8, 8, 1), (3,) + (1,) * 254],
                         ids=["C1", "C2", "C3", "C5", "C17", "C257_n_ext_1"])
def test_partial_counter_words_and_single_extension_pieces(tune, one_wg, sizes):
    # C257: after one piece of three, 254 pieces of one extension each: the bytes of a
    # counter word belong to four threads, and words 15, 31, .. to two waves; one workgroup
    # counts the three slabs of T = 2100 rows, so every thread updates its byte on every slab
    tune(slab_cls=0)
    rng = np.random.default_rng(len(sizes))
    B = _rows(rng, 2100)
    prefix, ext_off, ext = _groups(rng, F1, 2, sizes)
    C = int(ext.size)
    assert C == sum(sizes) and (C < 4 or C % 4 == 1)
    ref = _support(B, prefix, ext_off, ext)
    assert ref.min() >= 2100 // 4 > 255                   # every counter spills
    got8, plan = _level(B, prefix, ext_off, ext, 1)
    got32, _ = _level(B, prefix, ext_off, ext, 4)
    assert plan["passes"] == 1 and plan["C"] == C
    assert np.array_equal(got32, ref) and np.array_equal(got8, ref)


# ---- 255, 255 + 1, 256 in one add; all-ones slabs under one workgroup ------------------
def test_counter_boundaries_with_one_workgroup(tune, one_wg):
    # one workgroup counts all four 1024-row slabs (width 16), so a byte lives across
    # slabs.  Prefix items 0, 1 are in every row; extension e's rows per slab:
    #   2: 255, 0, 0, 0     stays at 255 until the final flush
    #   3: 255, 1, 0, 0     255 + 1: spills 256, then nothing is left
    #   4: 0, 256, 0, 0     256 in one add
    #   5: 255, 1, 255, 1   spills 256 twice
    #   6: 254, 1, 1, 0     254 -> 255 -> spills 256
    #   7: 1024 in every slab (all ones): every add spills
    #   8: 0, 0, 0, 255     a byte first written on the last slab
    tune(slab_cls=0)
    per_slab = {2: (255, 0, 0, 0), 3: (255, 1, 0, 0), 4: (0, 256, 0, 0), 5: (255, 1, 255, 1), 6: (254, 1, 1, 0),
                7: (1024,) * 4, 8: (0, 0, 0, 255)}
    T = 4 * 1024
    B = np.zeros((T, F1), np.int64)
    B[:, :2] = 1
    for e, ns in per_slab.items():
        for s, n in enumerate(ns):
            r0 = 1024 * s + (17 if n < 1024 else 0)       # n rows of slab s
            B[r0:r0 + n, e] = 1
    prefix = np.array([[0, 1]], np.int32)
    ext = np.array(sorted(per_slab), np.int32)
    ext_off = np.array([0, ext.size], np.int64)
    ref = _support(B, prefix, ext_off, ext)
    assert ref.tolist() == [sum(per_slab[e]) for e in sorted(per_slab)]
    got8, plan = _level(B, prefix, ext_off, ext, 1)
    got32, _ = _level(B, prefix, ext_off, ext, 4)
    assert plan["sw"] == 16 and plan["passes"] == 1
    assert np.array_equal(got32, ref) and np.array_equal(got8, ref)


# ---- every width and build, straight through the launch --------------------------------
@functools.lru_cache(maxsize=None)
def _direct_case():
    rng = np.random.default_rng(77)
    B = _rows(rng, 4166)                                   # 4166 = 2 * 64 * 32 + 70
    prefix, ext_off, ext = _groups(rng, F1, 3, (1, 8, 9, 17, 2, 1, 1, 5) * 6)
    return B, prefix, ext_off, ext


def _direct(B, ncols, prefix, ext_off, ext, sw, accb, build):
    """One launch of fa_hip_count_slab_rec_cls at slab width sw over the first ncols columns:
    plan.cpp's records (they do not depend on the width), then ops.primitives._slab_count."""
    C = int(ext.size)
    rc, info, passes, buf = prim.level_plan_host(prefix, ext_off, ext, F1, (ncols + 63) // 64, cls=0, accb=accb)
    assert rc == 0 and int(info[6]) == 1
    n_used = int(info[3])
    assert n_used * (sw + 2) * 8 + C * 4 + 256 < 64 * 1024
    dbuf = torch.from_numpy(buf.copy()).to(DEV)
    base = dbuf.data_ptr()
    o_im, o_used, o_gpre, o_rec = (int(info[i]) for i in (12, 13, 15, 20))
    src = None
    if build == "src":
        # column j gathers row perm[j]; -1 columns are empty
        perm = np.random.default_rng(ncols).permutation(B.shape[0])[:ncols].astype(np.int32)
        perm[::97] = -1
        Bc = np.where((perm >= 0)[:, None], B[np.maximum(perm, 0)], 0)
        src = torch.from_numpy(perm).to(DEV)
        roff, ranks = _csr(B)
    else:
        Bc = B[:ncols]
        roff, ranks = _csr(Bc)
    roff, ranks = roff.to(DEV), ranks.to(DEV)
    bm = None
    if build == "bitmap":
        bm, _ = prim.build_bitmaps(roff, ranks, None, ncols, n_used, dbuf[o_im:o_im + F1],
                                   dbuf[o_used:o_used + n_used])
    out = torch.zeros(C, dtype=torch.int32, device=DEV)
    a, b, e0 = passes.tolist()[0]
    prim._slab_count(roff=prim._p(roff), ranks=prim._p(ranks), src=prim._p(src), ncols=ncols, item_map=base + 4 * o_im,
                     F1=F1, n_used=n_used, gpre=base + 4 * o_gpre, rec=base + 4 * (o_rec + 12 * a), G=b - a, C=C,
                     wword=None, out=out.data_ptr(), sw=sw, st=prim._stream(ranks), round_acc=True,
                     map_bytes=prim.slab_map_lds(F1), bm=prim._p(bm), bm_ld=prim.bitmap_ld(bm), accb=accb)
    torch.cuda.synchronize()
    return out.cpu().numpy().astype(np.int64), _support(Bc, prefix, ext_off, ext)


@pytest.mark.parametrize("build", ["contig", "src", "bitmap"])
@pytest.mark.parametrize("sw", [4, 8, 16, 32])
def test_every_width_and_build(sw, build):
    B, prefix, ext_off, ext = _direct_case()
    # below one slab; then at least two slabs and a part of one (no multiple of 64 * SW for any
    # width), with enough rows that the counts pass a byte
    for ncols in (50, max(2 * 64 * sw + 70, 1350)):
        got8, ref = _direct(B, ncols, prefix, ext_off, ext, sw, 1, build)
        got32, _ = _direct(B, ncols, prefix, ext_off, ext, sw, 4, build)
        assert np.array_equal(got32, ref), (ncols, "u32")
        assert np.array_equal(got8, ref), (ncols, "bytes")
    assert ref.max() > 255


# ---- the edge cases of the slab kernel's own tests, counted in bytes --------------------
@pytest.mark.parametrize("case", list(SLAB_CASES))
def test_slab_edge_cases_in_bytes(tune, case):
    # widths 16 / 8 / 4 by the rule, class layout on (cls 2), long prefixes, and levels cut
    # into several passes (bitmap build)
    T, F, _, m, _, lds, cls, _, _ = SLAB_CASES[case]
    B, prefix, ext_off, ext, ref = _slab_case(case)
    roff, ranks = _csr(B)
    tune(slab_cls=cls)
    if lds is not None:
        tune(slab_lds_bytes=lds)
    got = ops.count_level(roff.to(DEV), ranks.to(DEV), None, T, F, prefix, ext_off, ext, None, kernel="slab", accb=1)
    plan = dict(prim.LAST_LEVEL_PLAN)
    want_sw, cap = prim.slab_width(plan["used"], ext.size, prim.dl_lds_budget(F), 1)
    assert plan["sw"] == want_sw and (plan["passes"] > 1) == (ext.size > cap)
    assert plan["cls"] == (1 if cls == 2 and m <= 12 else 0), plan
    assert np.array_equal(got.cpu().numpy(), ref)


def test_class_layout_in_bytes_over_several_slabs(tune):
    tune(slab_cls=2)
    rng = np.random.default_rng(5)
    B = _rows(rng, 3000, dens=0.6)
    prefix, ext_off, ext = _groups(rng, F1, 3, (1, 8, 9, 17, 2, 3) * 20)
    ref = _support(B, prefix, ext_off, ext)
    got8, plan = _level(B, prefix, ext_off, ext, 1)
    assert plan["cls"] == 1 and ref.max() > 255
    assert np.array_equal(got8, ref)


# ---- divided piece list ---------------------------------------------------------------
def test_piece_parts_sum_to_the_whole(tune):
    tune(slab_cls=0)
    rng = np.random.default_rng(9)
    B = _rows(rng, 2100)
    prefix, ext_off, ext = _groups(rng, F1, 2, (1, 8, 9, 17, 2, 3) * 40)     # > 128 pieces: both parts count
    ref = _support(B, prefix, ext_off, ext)
    hip = _native.hip()
    parts = []
    try:
        for p in (0, 1):
            assert hip.fa_hip_set_piece_part(p, 2) == 0
            parts.append(_level(B, prefix, ext_off, ext, 1)[0])
    finally:
        hip.fa_hip_set_piece_part(0, 1)
    assert parts[0].any() and parts[1].any()
    assert not (parts[0].astype(bool) & parts[1].astype(bool) & (ref == 0)).any()
    assert np.array_equal(parts[0] + parts[1], ref)


# ---- weighted rows: u32, whatever is asked ----------------------------------------------
def test_weighted_rows_fall_back_to_u32():
    rng = np.random.default_rng(13)
    T = 1500
    B = _rows(rng, T)
    prefix, ext_off, ext = _groups(rng, F1, 2, (1, 8, 9, 17, 2, 3) * 5)
    w = rng.integers(1, 9, (T + 63) // 64).astype(np.int32)          # one weight per 64-column word
    wcol = np.repeat(w, 64)[:T].astype(np.int64)
    ref = np.zeros(ext.size, np.int64)
    for g in range(prefix.shape[0]):
        has = B[:, prefix[g]].all(1)
        e = ext[ext_off[g]:ext_off[g + 1]]
        ref[ext_off[g]:ext_off[g + 1]] = ((B[:, e] & has[:, None]) * wcol[:, None]).sum(0)
    wt = torch.from_numpy(w).to(DEV)
    got8, _ = _level(B, prefix, ext_off, ext, 1, wword=wt)
    got32, _ = _level(B, prefix, ext_off, ext, 4, wword=wt)
    assert np.array_equal(got32, ref) and np.array_equal(got8, ref)


# ---- the device plan: each candidate in exactly one piece ------------------------------
@pytest.fixture(scope="module")
def dl_state():
    return prim.DeviceLevelState(DEV)


def _device_records(plan_rec, pieces):
    return plan_rec[:12 * pieces].cpu().numpy().view(np.uint32).reshape(-1, 12)


@pytest.mark.parametrize("deal", [False, True], ids=["plain", "lane_deal"])
@pytest.mark.parametrize("name,max_levels,growth", [("lat20_F70", 2, 5.0), ("lat40_F70", 1, 1.0)])
def test_device_plan_pieces_partition_the_candidates(dl_state, tune, name, max_levels, growth, deal):
    # lat20: parent rows with 0 .. 18 extensions (pieces of every size, rows of 1, 2 and 3
    # pieces); lat40: whole 256-record windows of the lane deal.  Then the plan counted in
    # bytes over dense rows.
    S, K = dl_state, prim.dl()
    Fb, ch = bundle_case(name, max_levels)
    L, _ = accepted(ch, max_levels, growth)
    c, P0 = run_bundle(S, Fb, ch, max_levels, growth)
    assert c[K.kDlLevels] == L
    C = int(sum(len(cand) for _, _, cand in ch[:L]))
    T = 2100
    rng = np.random.default_rng(3)
    B = (rng.random((T, Fb)) < 0.3).astype(np.int64)
    B[np.ix_(np.arange(T) % 8 < 2, np.unique(ch[0][0]))] = 1
    B[B.sum(1) < 2, :2] = 1
    has = B.astype(bool)
    ref = np.concatenate([has[:, cand].all(2).sum(0) for _, _, cand in ch[:L]]).astype(np.int64)
    roff, ranks = _csr(B)
    tune(lane_deal_min_rows=0 if deal else -1)
    S.rows_hint = T
    try:
        plan = prim.dl_plan(S, L, Fb, int(c[K.kDlNUsed]), C, prim.dl_lds_budget(Fb), DEV, accb=1.0)
        got = prim.dl_count(S, plan, roff.to(DEV), ranks.to(DEV), None, T, Fb, None).cpu().numpy()
        pieces = int(S.ctl[K.kDlPieces].item())
    finally:
        S.rows_hint = 0
    per = np.concatenate([cnt for _, cnt, _ in ch[:L]])
    assert pieces == int(((per + 7) // 8).sum())
    piece_ranges_partition(_device_records(plan["rec"], pieces), [(0, pieces, 0)], C)
    assert ref.max() > 255 and np.array_equal(got.astype(np.int64), ref)
    del P0


def test_device_window_plans_partition_their_windows(dl_state):
    # window plans (levels.hip fa_hip_dl_plan_window_bits) of a one-level bundle: a window
    # [w0, w1) that cuts parent rows' extension lists; its pieces tile [0, w1 - w0)
    S, K = dl_state, prim.dl()
    Fb, ch = bundle_case("lat20_F70", 1)
    c, P0 = run_bundle(S, Fb, ch, 1, 1.0)
    C = len(ch[0][2])
    st = torch.cuda.current_stream(DEV).cuda_stream
    lib = _native.hip()
    item_map = torch.empty(Fb, dtype=torch.int32, device=DEV)
    rec = torch.empty(12 * C + 12, dtype=torch.int32, device=DEV)
    part = torch.empty(8 * (len(ch[0][0]) // 256 + 1) + 16, dtype=torch.int32, device=DEV)
    gpre = torch.empty(1, dtype=torch.int32, device=DEV)
    for w0, w1 in ((0, 5), (5, 300), (300, 301), (301, C)):
        _native.check(lib.fa_hip_dl_plan_window_bits(S.desc.ctypes.data, 1, prim._p(S.ctl), Fb, None, prim._p(item_map),
                                                     prim._p(rec), C, prim._p(part), part.numel(), prim._p(gpre),
                                                     gpre.numel(), w0, w1, 16, st), "fa_hip_dl_plan_window_bits")
        pieces = int(S.ctl[K.kDlPieces].item())
        piece_ranges_partition(_device_records(rec, pieces), [(0, pieces, 0)], w1 - w0)
    del P0


# ---- a small mined run -----------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _mined_ref():
    from fastapriori_amd.models.apriori import FastApriori, MinerConfig
    from fastapriori_amd.parallel.comm import Comm
    from fastapriori_amd.utils.io import generate_shard
    from fastapriori_amd.utils.metrics import Logger
    cpu = generate_shard(200_000, Comm(), "cpu", 10.0, 4.0, 2000, 1000, 4)
    ref = FastApriori(0.002, config=MinerConfig(min_support=0.002), logger=Logger(0, enabled=False)).run(cpu)
    return cpu, ref


@pytest.mark.parametrize("mode", ["every_bundle", "width_upgrade", "width_upgrade_small_lds"])
def test_mined_run_with_byte_bundles(tune, mode):
    # dl_acc8_bundles = 1: every bundle accepted and counted at one byte per candidate;
    # = 2: bundled as without the knob, bytes only where they move a bundle's slab up to
    # width 16 -- none at the default LDS budget (the first bundle is at width 16 already);
    # with the budget shrunk so that u32 leaves width 16 for the first bundle, that bundle
    from fastapriori_amd.models.apriori import FastApriori, MinerConfig
    from fastapriori_amd.ops.host import apriori_gen
    from fastapriori_amd.utils.metrics import Logger
    cpu, ref = _mined_ref()
    nF1 = len(ref.levels[0])
    tune(dl_acc8_bundles=1 if mode == "every_bundle" else 2, dl_acc8_min_rows=0, lane_deal_min_rows=-1)
    if mode == "width_upgrade_small_lds":
        f2 = np.ascontiguousarray(ref.levels[1], dtype=np.int32)
        pi, eo, ex = apriori_gen(f2)
        C3, U = int(ex.size), int(np.union1d(f2[pi].ravel(), ex).size)
        shrunk = U * 144 + 4 * (min(C3, 8192) - 1)        # width 16 holds one u32 too few
        assert prim.slab_width(U, C3, shrunk, 4)[0] in (8, 4) and prim.slab_width(U, C3, shrunk, 1)[0] == 16
        tune(slab_lds_bytes=shrunk + prim.slab_map_lds(nF1))
    m = FastApriori(0.002, config=MinerConfig(min_support=0.002), logger=Logger(0, enabled=False))
    got = m.run(cpu.to(DEV))
    st = m.stats
    assert st.get("device_bundles", 0) >= 1 and "fallbacks" not in st, st
    shapes = st["device_bundle_shapes"]                   # (k0, levels, C, used, sw, accumulator bytes)
    print(mode, shapes)
    assert shapes[0][0] == 3 and shapes[0][4] == 16, shapes
    recs = sorted((r for r in m.log.records if r.get("phase") == "level" and r["k"] >= 3), key=lambda r: r["k"])
    assert recs[0]["k"] == 3 and recs[0]["slab_words"] == 16, recs[0]
    if mode == "every_bundle":
        assert m._dl_accb == 1.0 and all(s[5] == 1 for s in shapes), shapes
    elif mode == "width_upgrade":
        assert m._dl_accb == 4.0 and all(s[5] == 4 for s in shapes), shapes
    else:
        assert m._dl_accb == 4.0 and shapes[0][5] == 1, shapes
        # bundled as u32 bundles it: the same levels per bundle as with the knob off
        tune(dl_acc8_bundles=0)
        m0 = FastApriori(0.002, config=MinerConfig(min_support=0.002), logger=Logger(0, enabled=False))
        m0.run(cpu.to(DEV))
        assert [s[:4] for s in m0.stats["device_bundle_shapes"]] == [s[:4] for s in shapes]
        assert m0.stats["device_bundle_shapes"][0][4] in (8, 4)
        # below TUNING.dl_acc8_min_rows rows the bundles stay as the rule gave them
        tune(dl_acc8_bundles=2, dl_acc8_min_rows=1 << 20)
        m1 = FastApriori(0.002, config=MinerConfig(min_support=0.002), logger=Logger(0, enabled=False))
        m1.run(cpu.to(DEV))
        assert m1.stats["device_bundle_shapes"] == m0.stats["device_bundle_shapes"]
    assert [len(x) for x in got.levels] == [len(x) for x in ref.levels]
    for x, y in zip(got.levels, ref.levels):
        assert np.array_equal(x, y)
    for x, y in zip(got.counts, ref.counts):
        assert np.array_equal(x, y)
    assert got.as_dict() == ref.as_dict() and max(int(np.max(c)) for c in ref.counts[2:]) > 255
