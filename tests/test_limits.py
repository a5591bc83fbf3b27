"""The kernels' capacity limits and pads (csrc/host/fa_limits.h) through libfa_host.so's
fa_limits export: Python holds no copy of them, so the table here is the oracle -- the
values prep.hip, count.hip, gen.hip, parse.hip, plan.cpp, ops/primitives.py and
models/apriori.py each used to write out.  The GPU test checks from the outside that a
launcher and the table agree: the launcher takes its argument at the table's value (the
result compared with numpy) and returns an error one past it."""
import numpy as np
import pytest
import torch

VALUES = dict(
    kLdsBins=16384, kF1RankMax=2048, kSkLog=14, kSkGridMax=256, kF1ExactMaxCand=8192, kCSpan=8192, kLongMax=16384,
    kCwMaxWords=16, kCwMaxF1=65536, kProbeBits=1 << 22, kProbeMaxRows=1 << 24, kTrimAliveLds=32768, kTrimHist=256,
    kTrimStripes=64, kCmpHist=256, kCmpStripes=64, kCmpSpan=4096, kCmpMidPerWave=8, kCmpMaxNB=8, kScanChunk=4096,
    kPW=16, kPairAhead=3, kPairPadBatches=50, kPairLrPad=1024, kPairCntSpare=64, kMaxBlockExt=1024, kSlabThreads=1024,
    kWinPlanes=11, kWinMaxItems=2047,
    kAgMarkMinWords=128, kDsBlk=4096, kHistCap=8192,
    kSkA0=0x9E3779B1, kSkA1=0x85EBCA77)


def test_every_exported_limit_has_its_value(native):
    from fastapriori_amd.ops import primitives as Pm
    L = Pm.limits()
    assert L.table == VALUES
    assert all(getattr(L, n) == v for n, v in VALUES.items())
    assert L is Pm.limits()                          # read once


def test_derived_limits(native):
    from fastapriori_amd.ops import primitives as Pm
    L = Pm.limits()
    assert L.kPairPadBatches == L.kPairAhead * L.kPW + 2 == 3 * L.kPW + 2
    assert L.kWinMaxItems == 2 ** L.kWinPlanes - 1
    assert L.kCwMaxF1 == L.kCwMaxWords * 4096
    assert L.kF1ExactMaxCand * 2 == 1 << L.kSkLog
    assert L.kCmpHist == L.kTrimHist
    assert Pm.DEDUP_PROBE_ROWS <= L.kProbeMaxRows
    assert [Pm.ag_mark_words(F1) for F1 in (1, 4096, 4097, 32768)] == [128, 128, 129, 1024]


# ---------------------------------------------------------------------------
# launchers against the table (GPU).  Every call, the rejected ones too, gets valid
# tensors of the sizes its arguments ask for.
# ---------------------------------------------------------------------------
def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _f1_rank(prim, L, over):
    # the accepting side (V = kF1RankMax) is test_f1_rank.py's V = 2048 case
    assert over
    V = L.kF1RankMax + 1
    hist = _dev(np.full(V, 3, np.int64))
    lut = torch.empty(V, dtype=torch.int32, device="cuda")
    pack = torch.empty(2 * V + 1, dtype=torch.int64, device="cuda")
    return lambda: prim._hip_call("fa_hip_f1_rank", hist.data_ptr(), V, 2, 0, lut.data_ptr(), pack.data_ptr(),
                                  prim._stream(hist)), None


def _win_alive(prim, L, over):
    # 2^kWinPlanes - 1 items: counts up to 2047 in the bit planes.  The items are the rows of
    # a 16-row bitmap taken again and again; column c of row r is set when c >= 8 r, so
    # column c counts the items of rows <= c / 8, and the last columns all of them
    n_items, F, W, ld = L.kWinMaxItems + over, 16, 3, 64
    ncols = 64 * W
    bits = np.arange(ncols)[None, :] >= 8 * np.arange(F)[:, None]
    words = np.zeros((F, ld * 64), np.uint8)
    words[:, :ncols] = bits
    bm = _dev(np.packbits(words, axis=1, bitorder="little").view(np.int64))
    rows = (np.arange(n_items) % F).astype(np.int32)
    rows_d = _dev(rows)
    alive = torch.zeros(W, dtype=torch.int64, device="cuda")
    cnt = torch.zeros(W, dtype=torch.int32, device="cuda")
    k = n_items - n_items // F                       # every row but the last
    count = bits[rows].sum(0)
    assert count.max() == n_items and (count >= k).any() and not (count >= k).all()

    def check():
        want = np.packbits(count >= k, bitorder="little").view(np.uint64)
        assert np.array_equal(alive.cpu().numpy().view(np.uint64), want)
        assert cnt.cpu().tolist() == [bin(int(w)).count("1") for w in want]

    return lambda: prim._hip_call("fa_hip_win_alive", bm.data_ptr(), ld, rows_d.data_ptr(), n_items, W, int(k),
                                  alive.data_ptr(), cnt.data_ptr(), prim._stream(bm)), check


def _rows_csr(rng, n, V, max_len, fixed=()):
    lens = rng.integers(0, max_len + 1, n)
    for row, length in fixed:
        lens[row] = length
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    items = np.concatenate([rng.choice(V, int(x), replace=False) for x in lens] + [np.zeros(0, np.int64)])
    return off, items.astype(np.int32)


def _compress_wave(prim, L, over):
    # the accepting side (F1 = kCwMaxF1) is test_prep_edges.py's wave_F65536 case
    assert over
    rng = np.random.default_rng(7)
    off, items = _rows_csr(rng, 8, 32, 6)
    lut = np.arange(32, dtype=np.int32)
    kept = np.arange(8, dtype=np.int32)
    t = [_dev(a) for a in (off, items, lut, kept, off)] + [torch.empty(max(items.size, 1), dtype=torch.int32,
                                                                       device="cuda")]
    return lambda: prim._hip_call("fa_hip_compress_wave", t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(), None, 8,
                                  t[3].data_ptr(), t[4].data_ptr(), t[5].data_ptr(), L.kCwMaxF1 + 1, None,
                                  prim._stream(t[0])), None


def _cmp_agg(prim, L, over):
    # kCmpMaxNB blocks of 256 ranks, the top rank in the last one; 300 rows: two workgroups
    nb, n = L.kCmpMaxNB + over, 300
    F1, nwg = 256 * L.kCmpMaxNB, 2
    rng = np.random.default_rng(11)
    off, items = _rows_csr(rng, n, F1 + 100, 6, fixed=[(5, 4), (299, 3)])
    items[off[5]:off[6]] = np.arange(F1 - 1, F1 - 5, -1)            # row 5: the top ranks
    lut = np.where(np.arange(F1 + 100) < F1, np.arange(F1 + 100), -1).astype(np.int32)
    agg = torch.zeros(3 * nwg, dtype=torch.int32, device="cuda")
    aggb = torch.zeros(nb * nwg, dtype=torch.int32, device="cuda")
    hist = torch.zeros(L.kCmpStripes, L.kCmpHist, dtype=torch.int32, device="cuda")
    t = [_dev(a) for a in (off, items, lut)]

    def check():
        r = lut[items]
        row = np.repeat(np.arange(n), np.diff(off))
        c = np.bincount(row[r >= 0], minlength=n)
        kept = c >= 2
        wg = np.arange(n) // 256
        want = np.stack([np.bincount(wg[kept], minlength=nwg), np.bincount(wg, c * kept, minlength=nwg),
                         np.zeros(nwg)], 1).astype(np.int64)
        assert np.array_equal(agg.cpu().numpy().reshape(nwg, 3), want)
        ok = (r >= 0) & kept[row]
        blocks = np.zeros((nb, nwg), np.int64)
        np.add.at(blocks, (r[ok] >> 8, wg[row[ok]]), 1)
        assert blocks[nb - 1].sum() > 0
        assert np.array_equal(aggb.cpu().numpy().reshape(nb, nwg), blocks)
        assert np.array_equal(hist.sum(0).cpu().numpy(), np.bincount(c[kept], minlength=L.kCmpHist))

    return lambda: prim._hip_call("fa_hip_cmp_agg", t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(), n,
                                  agg.data_ptr(), hist.data_ptr(), aggb.data_ptr(), nb, prim._stream(agg)), check


LAUNCHERS = [(_f1_rank, 1), (_win_alive, 0), (_win_alive, 1), (_compress_wave, 1), (_cmp_agg, 0), (_cmp_agg, 1)]


@pytest.mark.gpu
@pytest.mark.parametrize("build,over", LAUNCHERS, ids=[f"{b.__name__[1:]}{'_over' if o else ''}" for b, o in LAUNCHERS])
def test_launcher_limit_is_the_tables(build, over):
    from fastapriori_amd.ops import primitives as prim
    call, check = build(prim, prim.limits(), over)
    if over:
        with pytest.raises(RuntimeError, match="failed with HIP error code 1"):
            call()
        return
    call()
    check()
