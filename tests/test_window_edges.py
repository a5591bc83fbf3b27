"""Edge shapes of the window-by-window level path: count.hip k_win_alive / k_win_compact
(ops.primitives.window_bitmap), levels.hip k_dl_chunk_bits (ops.primitives.dl_window_plan) and
ops.primitives.dl_count_multipass.

The other tests of this path are whole mining runs of 150 000 .. 400 000 generated rows, which
fail as "a level-7 count differs", and five random window_bitmap shapes.  Here every input is
built on purpose -- bitmaps whose column c holds exactly c mod (n + 1) of the window's items,
alive masks placed on the word, wave and workgroup edges of the compaction, lattices of placed
ranks as candidates, dense rows B[T, F1] -- and the expected result comes from numpy by the
definition, never from another path of this project.  All values are integers or bits and every
comparison is exact equality over the whole output, padding included.

1. k_win_alive, called directly (fa_hip_win_alive)
2. k_win_compact, directly (fa_hip_win_compact, hand-made alive masks) and through window_bitmap
3. k_dl_chunk_bits (fa_hip_dl_chunk_bits)
4. dl_window_plan
5. dl_count_multipass against brute force

The unmarked tests build every input and check on the CPU that it has the property its case is
named for; the GPU tests then only run the kernels on them.
"""
import functools

import numpy as np
import pytest
import torch

from fastapriori_amd.ops import _native
from fastapriori_amd.ops import primitives as prim
from test_gen_edges import DEV, bundle_case, run_bundle, dl_state            # noqa: F401  (dl_state: a fixture)
from test_gpu_kernels import _unpack_rows
from test_kernel_edges import _csr

LAYOUTS = [(i, o) for i in (False, True) for o in (False, True)]             # (input blocked, output blocked)


# ---------------------------------------------------------------------------
# bitmaps
# ---------------------------------------------------------------------------
def _pack(bits, Wp):
    """bool [n, ncols] -> uint64 [n, Wp], column c = bit c & 63 of word c >> 6, zero past ncols."""
    n, ncols = bits.shape
    assert ncols <= 64 * Wp
    b = np.zeros((n, Wp * 64), np.uint8)
    b[:, :ncols] = bits
    return np.packbits(b, axis=1, bitorder="little").view(np.uint64)


def _popc(words):
    return np.unpackbits(np.ascontiguousarray(words).view(np.uint8).reshape(words.size, 8), axis=1).sum(1).astype(np.int64)


def _to_blocked(wrd):
    """[F, Wp] -> the 8-word blocked layout [Wp / 8, F, 8]."""
    F, Wp = wrd.shape
    return np.ascontiguousarray(wrd.reshape(F, Wp // 8, 8).transpose(1, 0, 2))


def _from_blocked(blk):
    """[Wp / 8, F, 8] -> [F, Wp]."""
    return np.ascontiguousarray(blk.transpose(1, 0, 2)).reshape(blk.shape[1], -1)


def _dev_bitmap(bits, W, blocked, Wp=None):
    """The bitmap of bits (bool [F, ncols]) on the device with Wp > W words per row ->
    (tensor, the kernels' ld): row-major [F, Wp] or blocked [Wp / 8, F, 8]."""
    if Wp is None:
        Wp = (W // 8 + 2) * 8 if blocked else W + 3              # (two blocks or more: a block stride to speak of)
    wrd = _pack(bits, Wp)
    t = torch.from_numpy((_to_blocked(wrd) if blocked else wrd).view(np.int64)).to(DEV)
    ld = prim.bitmap_ld(t)
    assert ld == (-8 * bits.shape[0] if blocked else Wp) and Wp > W
    return t, ld


def _window_rows_of(rng, F, n_items):
    """n_items sorted rows of a bitmap of F > n_items rows, row 0 and the last row among them."""
    if n_items == 1:
        return np.array([F - 1], np.int32)
    mid = 1 + rng.choice(F - 2, n_items - 2, replace=False)
    return np.sort(np.concatenate([[0, F - 1], mid])).astype(np.int32)


def _held(rng, n_items, held):
    """bool [n_items, ncols]: column c holds exactly held[c] of the items, which ones at random."""
    order = rng.random((n_items, held.size)).argsort(0).argsort(0)           # a permutation per column
    return order < held[None, :]


# ---------------------------------------------------------------------------
# 1. k_win_alive: alive[q] = the mask of word q's columns that hold >= k of the window's items
#    (a bit-sliced counter of `planes` planes), cnt[q] its popcount
# ---------------------------------------------------------------------------
ALIVE_N = [1, 2, 3, 7, 8, 9, 15, 16, 17, 63, 64, 255, 256]       # 2^p - 1, 2^p: the planes loop; the ring of 8
ALIVE_W = [1, 63, 255, 256, 257]                                 # the 256-thread grid's edge
ALIVE_CASES = [(n, 9) for n in ALIVE_N] + [(9, W) for W in ALIVE_W]


def _alive_ks(n):
    """1, 2, n - 1, n, n + 1 and the powers of two up to n with their neighbours."""
    ks, p = {1, 2, n - 1, n, n + 1}, 1
    while p <= n:
        ks |= {p - 1, p, p + 1}
        p *= 2
    return sorted(k for k in ks if k >= 1)


@functools.lru_cache(maxsize=None)
def _alive_case(n_items, W):
    """-> (bits bool [F, ncols] of a bitmap of F = n_items + 5 rows, the window's rows int32
    [n_items], ncols).  Column c holds exactly c mod (n_items + 1) of the window's items; the
    other rows are noise."""
    rng = np.random.default_rng(1000 * n_items + W)
    ncols, F = 64 * W - 17, n_items + 5
    rows = _window_rows_of(rng, F, n_items)
    target = np.arange(ncols) % (n_items + 1)
    bits = rng.random((F, ncols)) < 0.5
    bits[rows] = _held(rng, n_items, target)
    count = bits[rows].sum(0)
    assert ncols % 64 and ncols > n_items and np.array_equal(count, target)
    assert set(count.tolist()) == set(range(n_items + 1))          # every count 0 .. n_items is present
    assert rows.size == n_items and np.unique(rows).size == n_items and rows[-1] == F - 1 and (n_items == 1 or rows[0] == 0)
    return bits, rows, ncols


def _alive_ref(bits, rows, W, k):
    """(alive uint64 [W], cnt int64 [W]) by the definition."""
    a = _pack((bits[rows].sum(0) >= k)[None, :], W)[0]
    return a, _popc(a)


def test_alive_references():
    assert _alive_ks(8) == [1, 2, 3, 4, 5, 7, 8, 9] and _alive_ks(1) == [1, 2]
    for n, W in ALIVE_CASES:
        bits, rows, ncols = _alive_case(n, W)
        planes = n.bit_length()                                   # the launcher's loop
        assert (1 << planes) > n >= (1 << (planes - 1))
        ks = _alive_ks(n)
        assert n + 1 in ks and any(k >> planes for k in ks) == (n + 1 == 1 << planes)    # the early-out
        for k in ks:
            a, cnt = _alive_ref(bits, rows, W, k)
            assert int(cnt.sum()) == int((np.arange(ncols) % (n + 1) >= k).sum())
            assert (k <= n) == bool(cnt.any())
            assert not (int(a[-1]) >> (ncols & 63))               # the padding bits are dead


def _run_alive(bm, ld, rows_d, n_items, W, k):
    """fa_hip_win_alive into buffers of W + 2 preset entries -> (alive uint64, cnt int32), W + 2 each."""
    alive = torch.full((W + 2,), 0x5A5A5A5A5A5A5A5A, dtype=torch.int64, device=DEV)
    cnt = torch.full((W + 2,), -7, dtype=torch.int32, device=DEV)
    prim._hip_call("fa_hip_win_alive", bm.data_ptr(), ld, rows_d.data_ptr(), n_items, W, int(k), alive.data_ptr(),
                   cnt.data_ptr(), prim._stream(bm))
    return alive.cpu().numpy().view(np.uint64), cnt.cpu().numpy()


@pytest.mark.gpu
@pytest.mark.parametrize("n_items,W", ALIVE_CASES)
def test_win_alive_planted_counts(n_items, W):
    bits, rows, _ = _alive_case(n_items, W)
    rows_d = torch.from_numpy(rows).to(DEV)
    for blocked in (False, True):
        bm, ld = _dev_bitmap(bits, W, blocked)
        for k in _alive_ks(n_items):
            alive, cnt = _run_alive(bm, ld, rows_d, n_items, W, k)
            want, wcnt = _alive_ref(bits, rows, W, k)
            bad = np.flatnonzero(alive[:W] != want)
            assert bad.size == 0, (blocked, k, bad[:4], [hex(int(x)) for x in alive[bad[:4]]])
            assert np.array_equal(cnt[:W], wcnt), (blocked, k)
            assert (alive[W:] == 0x5A5A5A5A5A5A5A5A).all() and (cnt[W:] == -7).all()     # nothing past W


# ---------------------------------------------------------------------------
# 2. k_win_compact: every window row's bits at the alive columns, packed from bit 0; one wave
#    per 64 input words, output words shared between neighbour waves
# ---------------------------------------------------------------------------
def _out_words(K):
    """window_bitmap's padded output width in words."""
    return -(-((K + 63) // 64) // 64) * 64


def _spread(rng, total, first=None):
    """Alive bits per word of one wave's 64 words summing to total (at most 64 each), word 0
    fixed to `first` when given."""
    cnt = np.zeros(64, np.int64)
    free = np.arange(64)
    if first is not None:
        cnt[0], free, total = first, free[1:], total - first
    assert 0 <= total <= 64 * free.size
    cnt += np.bincount(rng.permutation(np.repeat(free, 64))[:total], minlength=64)
    return cnt


def _alive_from_counts(rng, cnt, ncols):
    """bool [ncols]: cnt[q] alive columns in word q, at random bits."""
    a = np.zeros((cnt.size, 64), bool)
    for q, c in enumerate(cnt):
        a[q, rng.permutation(64)[:c]] = True
    a = a.reshape(-1)
    assert not a[ncols:].any()
    return a[:ncols]


COMPACT_CASES = ["identity", "one_word", "dead_waves", "offsets", "last_word", "K4096", "K4097"] + \
                [f"items{n}" for n in (1, 7, 8, 9, 17)] + [f"W{W}" for W in (1, 63, 64, 65, 255, 256, 257, 300)]


@functools.lru_cache(maxsize=None)
def _compact_case(name):
    """-> (W, ncols, alive bool [ncols], n_items), with the checks that the mask is what the
    case is named for."""
    rng = np.random.default_rng(sum(map(ord, name)))
    n_items = 3
    if name == "identity":                         # shift 0, no word shared, output = input
        W = 130
        ncols = 64 * W
        alive = np.ones(ncols, bool)
    elif name == "one_word":                       # one alive column per wave: six waves OR into output word 0
        W = 64 * 5 + 3
        ncols = 64 * W - 9
        alive = np.zeros(ncols, bool)
        for s in range(0, ncols, 4096):
            alive[s + rng.integers(0, min(4096, ncols - s))] = True
        assert alive.sum() == 6 and _out_words(6) == 64
    elif name == "dead_waves":                     # the first, a middle and the last wave without an alive column
        W = 64 * 7
        ncols = 64 * W - 30
        alive = rng.random(ncols) < 0.3
        for wv in (0, 3, 6):
            alive[4096 * wv:4096 * (wv + 1)] = False
        per_wave = np.add.reduceat(alive, np.arange(0, ncols, 4096))
        assert (per_wave == 0).tolist() == [True, False, False, True, False, False, True]
    elif name == "offsets":
        # wave i has 64 a_i + i alive columns, so its first output bit is at i (i - 1) / 2
        # mod 64: over the waves 1 .. 64 every value once (wave 0 starts on bit 0 as wave 1
        # does).  The wave that starts on bit 63 does so with a word of one alive column;
        # one that starts on another odd bit with a fully alive word
        NW, n_items = 65, 2
        W = 64 * NW
        ncols = 64 * W
        n = np.array([64 * (1 + i % 2) + i for i in range(NW)])
        base = np.concatenate([[0], np.cumsum(n)[:-1]])
        assert sorted((base[1:] & 63).tolist()) == list(range(64))   # every base & 63 is present
        i63 = int(np.flatnonzero((base & 63) == 63)[0])
        iodd = int(np.flatnonzero(((base & 63) % 2 == 1) & ((base & 63) != 63))[0])
        cnt = np.concatenate([_spread(rng, int(n[i]), {i63: 1, iodd: 64}.get(i)) for i in range(NW)])
        alive = _alive_from_counts(rng, cnt, ncols)
        off = np.concatenate([[0], np.cumsum(cnt)])
        assert (off[64 * i63] & 63, cnt[64 * i63]) == (63, 1) and (off[64 * iodd] & 1, cnt[64 * iodd]) == (1, 64)
        assert np.array_equal(off[::64][:NW], base)
    elif name == "last_word":                      # alive only in the partial last word
        W = 70
        ncols = 64 * 69 + 40
        alive = np.zeros(ncols, bool)
        alive[64 * 69:] = rng.random(40) < 0.5
        assert W % 64 and alive.any()
    elif name in ("K4096", "K4097"):               # the padded output: 64 words, then 128
        W = 80
        ncols = 64 * W - 13
        alive = np.zeros(ncols, bool)
        alive[rng.choice(ncols, int(name[1:]), replace=False)] = True
        assert _out_words(int(alive.sum())) == (64 if name == "K4096" else 128)
    elif name.startswith("items"):                 # rounds of kWinBatch = 8 items, a partial last one
        W, n_items = 70, int(name[5:])
        ncols = 64 * W - 21
        alive = rng.random(ncols) < 0.4
    else:                                          # one wave, part of one, the 4-wave workgroup's edge
        W = int(name[1:])
        ncols = 64 * W - 11
        alive = rng.random(ncols) < 0.4
    assert ncols <= 64 * W and ncols > 64 * (W - 1) and alive.any()
    return W, ncols, alive, n_items


@functools.lru_cache(maxsize=None)
def _compact_inputs(name, planted):
    """-> (bits bool [F, ncols] of a bitmap of F = n_items + 4 rows, the window's rows, k).
    planted: the columns alive for k = max(1, n_items - 1) are exactly the case's mask (an alive
    column holds k or more of the items, a dead one fewer; which ones at random: the payload);
    else the rows are noise and the mask is handed to the kernel as it is."""
    W, ncols, alive, n_items = _compact_case(name)
    rng = np.random.default_rng(7 + sum(map(ord, name)))
    F = n_items + 4
    rows = _window_rows_of(rng, F, n_items)
    bits = rng.random((F, ncols)) < 0.5
    k = max(1, n_items - 1)
    if planted:
        held = np.where(alive, rng.integers(k, n_items + 1, ncols), rng.integers(0, k, ncols))
        bits[rows] = _held(rng, n_items, held)
        assert np.array_equal(bits[rows].sum(0) >= k, alive)
    return bits, rows, k


def _compact_ref(bits, rows, alive):
    """uint64 [n_items, _out_words(K)]: bits[rows][:, alive], everything past K zero."""
    return _pack(bits[rows][:, alive], _out_words(int(alive.sum())))


def test_compact_references():
    for name in COMPACT_CASES:
        W, ncols, alive, n_items = _compact_case(name)
        for planted in (False, True):
            bits, rows, k = _compact_inputs(name, planted)
            want = _compact_ref(bits, rows, alive)
            K = int(alive.sum())
            assert np.array_equal(_unpack_rows(want, K), bits[rows][:, alive])
            assert not _unpack_rows(want, want.shape[1] * 64)[:, K:].any()
    W, ncols, alive, _ = _compact_case("identity")
    bits, rows, _ = _compact_inputs("identity", False)
    assert np.array_equal(_compact_ref(bits, rows, alive)[:, :W], _pack(bits[rows], W))
    for kind in SAMPLED:
        _sampled_case(kind)


def _out_buffer(n_items, wp, blocked):
    if blocked:
        out = torch.zeros((wp // 8, n_items, 8), dtype=torch.int64, device=DEV)
        return out, -out.stride(0)
    out = torch.zeros((n_items, wp), dtype=torch.int64, device=DEV)
    return out, out.stride(0)


def _host_out(out, n_items):
    o = out.cpu().numpy().view(np.uint64)
    return _from_blocked(o) if o.ndim == 3 else o


@pytest.mark.gpu
@pytest.mark.parametrize("case", COMPACT_CASES)
def test_win_compact_direct(case):
    # hand-made alive masks and their exclusive prefix over rows of noise
    W, ncols, alive, n_items = _compact_case(case)
    bits, rows, _ = _compact_inputs(case, False)
    want = _compact_ref(bits, rows, alive)
    aw = _pack(alive[None, :], W)[0]
    off = np.concatenate([[0], np.cumsum(_popc(aw))]).astype(np.int64)
    alive_d = torch.from_numpy(aw.view(np.int64)).to(DEV)
    off_d, rows_d = torch.from_numpy(off).to(DEV), torch.from_numpy(rows).to(DEV)
    for blocked, out_blocked in LAYOUTS:
        bm, ld = _dev_bitmap(bits, W, blocked)
        out, ldo = _out_buffer(n_items, want.shape[1], out_blocked)
        prim._hip_call("fa_hip_win_compact", bm.data_ptr(), ld, rows_d.data_ptr(), n_items, W, alive_d.data_ptr(),
                       off_d.data_ptr(), out.data_ptr(), ldo, prim._stream(bm))
        got = _host_out(out, n_items)
        bad = np.argwhere(got != want)
        assert bad.size == 0, (blocked, out_blocked, bad[:4].tolist())


@pytest.mark.gpu
@pytest.mark.parametrize("case", COMPACT_CASES)
def test_window_bitmap_planted(case):
    # the same masks through k_win_alive: planted with k = n_items - 1, so the compacted rows
    # are ones with at most one hole per column
    W, ncols, alive, n_items = _compact_case(case)
    bits, rows, k = _compact_inputs(case, True)
    want, K = _compact_ref(bits, rows, alive), int(alive.sum())
    rows_d = torch.from_numpy(rows).to(DEV)
    for blocked, out_blocked in LAYOUTS:
        bm, _ = _dev_bitmap(bits, W, blocked)
        got = prim.window_bitmap(bm, rows_d, W, k, blocked=out_blocked)
        assert got[0] == K
        assert tuple(got[1].shape) == ((want.shape[1] // 8, n_items, 8) if out_blocked else want.shape)
        bad = np.argwhere(_host_out(got[1], n_items) != want)
        assert bad.size == 0, (blocked, out_blocked, bad[:4].tolist())
    # max_keep: K rows are kept, K - 1 are not
    got = prim.window_bitmap(bm, rows_d, W, k, max_keep=K)
    assert got is not None and got[0] == K and np.array_equal(_host_out(got[1], n_items), want)
    assert prim.window_bitmap(bm, rows_d, W, k, max_keep=K - 1) is None


# window_bitmap's sampling branch at W = 64 * WINDOW_SAMPLE words: the first W / WINDOW_SAMPLE
# words decide first
SAMPLED = {"dense_sample": (["fa_hip_win_alive"], False),
           "sparse_sample_total_over": (["fa_hip_win_alive"] * 2, False),
           "both_under": (["fa_hip_win_alive"] * 2 + ["fa_hip_win_compact"], True)}


@functools.lru_cache(maxsize=None)
def _sampled_case(kind):
    """-> (bits, rows, k, alive, max_keep).  dense_sample: every column of the sample alive, the rest
    dead: the extrapolation is over max_keep though the total is not; sparse_sample_total_over: 10
    alive columns in the sample, 3000 after it; both_under: the same with room for them."""
    rng = np.random.default_rng(len(kind))
    W = 64 * prim.WINDOW_SAMPLE
    ws = W // prim.WINDOW_SAMPLE
    ncols, n_items, k = 64 * W - 5, 3, 3
    alive = np.zeros(ncols, bool)
    if kind == "dense_sample":
        alive[:64 * ws] = True
        max_keep = 5000
        assert alive.sum() <= max_keep < alive[:64 * ws].sum() * (W / ws)
    else:
        alive[rng.choice(64 * ws, 10, replace=False)] = True
        alive[64 * ws + rng.choice(ncols - 64 * ws, 3000, replace=False)] = True
        max_keep = 3009 if kind == "sparse_sample_total_over" else 3010
        assert alive[:64 * ws].sum() * (W / ws) <= max_keep and alive.sum() == 3010
    rows = _window_rows_of(rng, n_items + 4, n_items)
    bits = rng.random((n_items + 4, ncols)) < 0.5
    bits[rows] = _held(rng, n_items, np.where(alive, 3, rng.integers(0, 3, ncols)))
    assert np.array_equal(bits[rows].sum(0) >= k, alive)
    return bits, rows, k, alive, max_keep


@pytest.mark.gpu
@pytest.mark.parametrize("kind", list(SAMPLED))
def test_window_bitmap_sampling(monkeypatch, kind):
    launches, kept = SAMPLED[kind]
    bits, rows, k, alive, max_keep = _sampled_case(kind)
    W = 64 * prim.WINDOW_SAMPLE
    bm, _ = _dev_bitmap(bits, W, True)
    seen, call = [], prim._hip_call
    monkeypatch.setattr(prim, "_hip_call", lambda name, *a: (seen.append(name), call(name, *a))[1])
    got = prim.window_bitmap(bm, torch.from_numpy(rows).to(DEV), W, k, max_keep=max_keep)
    assert seen == launches
    if not kept:
        assert got is None
    else:
        assert got[0] == alive.sum() and np.array_equal(_host_out(got[1], 3), _compact_ref(bits, rows, alive))


# ---------------------------------------------------------------------------
# 3. k_dl_chunk_bits: the used-item bitset of every chunk of a one-level bundle's candidates
# ---------------------------------------------------------------------------
CHUNK_CASES = ["lat20_F70", "lat12_F70_m3", "lat12_F64", "lat12_F65", "lat12_F128", "lat12_F32768"]


def _bitset(items, nwd):
    b = np.zeros(nwd * 64, np.uint8)
    b[np.asarray(items, np.int64)] = 1
    return np.packbits(b, bitorder="little").view(np.uint64)


def _chunk_sizes(C):
    return [1, 7, 256, C - 1, C, C + 1, 1024]


def _chunk_ref(cand, F1, chunk):
    """uint64 [chunks, words]: chunk j's row is the bitset of the items of candidates [j chunk, (j + 1) chunk)."""
    nwd = (F1 + 63) // 64
    return np.stack([_bitset(np.unique(cand[s:s + chunk]), nwd) for s in range(0, len(cand), chunk)])


def _level(case):
    """-> (F1, chain of one level, candidates int32 [C, m + 1])."""
    F1, ch = bundle_case(case, 1)
    return F1, ch, ch[0][2]


def test_chunk_references(native):
    assert prim.dl().kDlBitsW == 512 and CHUNK_CASES[-1].endswith(f"_F{64 * prim.dl().kDlBitsW}")
    for case in CHUNK_CASES:
        F1, ch, cand = _level(case)
        m0 = ch[0][0].shape[1]
        assert cand.shape == ({"lat20": 1140, "lat12": 495 if m0 == 3 else 220}[case[:5]], m0 + 1)
        used = set(np.unique(cand).tolist())
        assert {0, 63, F1 - 1} <= used and (F1 == 64 or 64 in used)
        C = len(cand)
        for chunk in _chunk_sizes(C):
            ref = _chunk_ref(cand, F1, chunk)
            assert ref.shape[0] == -(-C // chunk) and _popc(ref.reshape(-1)).reshape(ref.shape).sum(1).min() >= m0 + 1
            assert np.array_equal(np.bitwise_or.reduce(ref, 0), _bitset(sorted(used), ref.shape[1]))
        assert _chunk_ref(cand, F1, C - 1).shape[0] == 2 and _chunk_ref(cand, F1, 1).shape[0] == C
    assert len(_level("lat20_F70")[2]) % 1024 == 116               # a partial last chunk of the default size


def _chunk_bits(S, F1, chunk, nch, nwd):
    """fa_hip_dl_chunk_bits into a preset buffer of nch + 1 chunks -> (return code, uint64 [nch + 1, nwd])."""
    out = torch.full(((nch + 1) * nwd,), -1, dtype=torch.int64, device=DEV)
    rc = _native.hip().fa_hip_dl_chunk_bits(S.desc.ctypes.data, F1, chunk, out.data_ptr(),
                                            torch.cuda.current_stream(DEV).cuda_stream)
    return rc, out.cpu().numpy().view(np.uint64).reshape(nch + 1, nwd)


@pytest.mark.gpu
@pytest.mark.parametrize("case", CHUNK_CASES)
def test_dl_chunk_bits(dl_state, case):
    F1, ch, cand = _level(case)
    c, P0 = run_bundle(dl_state, F1, ch, 1, 1.0)
    assert c[prim.dl().kDlLevels] == 1 and c[prim.dl().kDlCl] == len(cand)
    nwd = (F1 + 63) // 64
    for chunk in _chunk_sizes(len(cand)):
        ref = _chunk_ref(cand, F1, chunk)
        rc, got = _chunk_bits(dl_state, F1, chunk, ref.shape[0], nwd)
        assert rc == 0
        bad = np.argwhere(got[:-1] != ref)
        assert bad.size == 0, (chunk, bad[:4].tolist())
        assert (got[-1] == np.uint64(0xFFFFFFFFFFFFFFFF)).all()    # nothing past the last chunk
    del P0


@pytest.mark.gpu
def test_dl_chunk_bits_refusals(dl_state):
    F1, ch, cand = _level("lat20_F70")
    c, P0 = run_bundle(dl_state, F1, ch, 1, 1.0)
    over = 64 * prim.dl().kDlBitsW + 1
    for f1, chunk in ((F1, 0), (over, 1024), (0, 1024)):
        rc, got = _chunk_bits(dl_state, f1, chunk, 2, (over + 63) // 64)
        assert rc == 1 and (got == np.uint64(0xFFFFFFFFFFFFFFFF)).all()      # refused, nothing launched
    del P0


# ---------------------------------------------------------------------------
# 4. dl_window_plan: greedily, the longest run of chunks whose item union leaves accumulators
#    for all of its candidates at the rule's slab width
# ---------------------------------------------------------------------------
def _ref_windows(cand, F1, chunk, lds, accb):
    """The docstring's rule from the candidates: [(w0, w1, sw, sorted items)], or None when one
    chunk alone does not fit."""
    C, wins, w0 = len(cand), [], 0
    while w0 < C:
        w1, best = w0, None
        while w1 < C:
            nxt = min(w1 + chunk, C)
            items = np.unique(cand[w0:nxt])
            sw, cap = prim.slab_width(items.size, nxt - w0, lds, accb)
            if sw == 0 or cap < nxt - w0:
                break
            w1, best = nxt, (sw, items)
        if best is None:
            return None
        wins.append((w0, w1, best[0], best[1]))
        w0 = w1
    return wins


def _check_windows(wins, cand, F1, chunk, lds, accb):
    """A plan against the rule, property by property."""
    C, nwd = len(cand), (F1 + 63) // 64
    assert wins[0][0] == 0 and wins[-1][1] == C
    for i, (w0, w1, sw, bits) in enumerate(wins):
        assert w0 < w1 and w0 % chunk == 0 and (w1 % chunk == 0 or w1 == C)      # on chunk boundaries
        assert i == 0 or w0 == wins[i - 1][1]                                    # in order, no gap
        items = np.unique(cand[w0:w1])
        assert np.asarray(bits).dtype == np.uint64 and np.array_equal(bits, _bitset(items, nwd)), i
        want_sw, cap = prim.slab_width(items.size, w1 - w0, lds, accb)
        assert sw == want_sw > 0 and cap >= w1 - w0, i
        if w1 < C:                                                               # maximal: one more chunk does not fit
            nxt = min(w1 + chunk, C)
            sw2, cap2 = prim.slab_width(np.unique(cand[w0:nxt]).size, nxt - w0, lds, accb)
            assert sw2 == 0 or cap2 < nxt - w0, i


# (case, chunk, LDS bytes, bytes per accumulator): 20 / 12 items at 48 B per 4-word slab row, then
# room for ~300 / ~130 / ~70 accumulators
PLAN_CASES = [("lat20_F70", 64, 20 * 48 + 4 * 300, 4), ("lat20_F70", 100, 20 * 48 + 2 * 300, 2),
              ("lat20_F70", 1024, 20 * 48 + 2 * 1030, 2), ("lat12_F70_m3", 64, 12 * 48 + 4 * 130, 4),
              ("lat12_F32768", 64, 12 * 48 + 4 * 70, 4), ("lat40_F70", 1024, 40 * 48 + 2 * 2500, 2),
              ("lat40_F70", 1024, 40 * 48 + 4 * 2500, 4)]


def test_window_plan_references(native):
    widths = set()
    for case, chunk, lds, accb in PLAN_CASES:
        F1, _, cand = _level(case)
        wins = _ref_windows(cand, F1, chunk, lds, accb)
        assert wins is not None and len(wins) >= (2 if (case, chunk) == ("lat20_F70", 1024) else 3), (case, len(wins))
        assert len({tuple(w[3].tolist()) for w in wins}) >= min(3, len(wins))    # windows with differing item sets
        widths |= {w[2] for w in wins}
        nwd = (F1 + 63) // 64
        _check_windows([(a, b, sw, _bitset(it, nwd)) for a, b, sw, it in wins], cand, F1, chunk, lds, accb)
    assert widths == {4, 8, 16}                                    # a window's width follows its own items
    F1, _, cand = _level("lat20_F70")
    assert _ref_windows(cand, F1, 64, 20 * 48 + 4 * 10, 4) is None


@pytest.mark.gpu
@pytest.mark.parametrize("case,chunk,lds,accb", PLAN_CASES)
def test_dl_window_plan(dl_state, case, chunk, lds, accb):
    F1, ch, cand = _level(case)
    c, P0 = run_bundle(dl_state, F1, ch, 1, 1.0)
    st = torch.cuda.current_stream(DEV).cuda_stream
    wins = prim.dl_window_plan(dl_state, F1, len(cand), lds, accb, st, DEV, chunk=chunk)
    ref = _ref_windows(cand, F1, chunk, lds, accb)
    assert wins is not None and [w[:3] for w in wins] == [w[:3] for w in ref]
    _check_windows(wins, cand, F1, chunk, lds, accb)
    del P0


@pytest.mark.gpu
def test_dl_window_plan_none(dl_state):
    F1, ch, cand = _level("lat20_F70")
    c, P0 = run_bundle(dl_state, F1, ch, 1, 1.0)
    st = torch.cuda.current_stream(DEV).cuda_stream
    # one chunk of 64 candidates over 20 items does not fit accumulators for 10
    assert prim.dl_window_plan(dl_state, F1, len(cand), 20 * 48 + 4 * 10, 4, st, DEV, chunk=64) is None
    # a bitset of more than kDlBitsW words
    assert prim.dl_window_plan(dl_state, 64 * prim.dl().kDlBitsW + 1, len(cand), 1 << 16, 4, st, DEV) is None
    del P0


# ---------------------------------------------------------------------------
# 5. dl_count_multipass: a one-level bundle counted window by window over dense rows B[T, F1],
#    its inputs built as FastApriori._dl_multipass builds them; the reference is the number
#    (or the weight) of the rows that hold all of a candidate's items
# ---------------------------------------------------------------------------
T_ROWS = 2100                 # no multiple of 64, more than one 1024-row slab
T_DRAIN = 70_000              # counts above 65 535; 274 four-word slabs, a u16 drain every 255
# name: (lattice, rows, per-window items, u16 accumulators, LDS bytes, bitmap, word weights,
#        window rows, sup_frac)
MP_CASES = {
    "equal_u16": ("lat40_F70", T_ROWS, False, True, 40 * 48 + 2 * 3500, "rank", False, False, 0.0),
    "equal_u32": ("lat40_F70", T_ROWS, False, False, 40 * 48 + 4 * 3500, "compact_blocked", False, False, 0.25),
    "items_rank": ("lat40_F70", T_ROWS, True, True, 40 * 48 + 2 * 2500, "rank_blocked", False, False, 0.25),
    "items_bmap": ("lat40_F70", T_ROWS, True, True, 40 * 48 + 2 * 2500, "compact_blocked", False, False, 0.0),
    "items_u32": ("lat40_F70", T_ROWS, True, False, 40 * 48 + 4 * 2500, "compact", False, False, 0.25),
    "items_wword": ("lat40_F70", T_ROWS, True, True, 40 * 48 + 4 * 2500, "rank", True, False, 0.25),
    "items_lat20": ("lat20_F70", T_ROWS, True, True, 20 * 48 + 2 * 1030, "compact_blocked", False, False, 0.25),
    "rows_rank": ("lat40_F70", T_ROWS, True, True, 40 * 48 + 2 * 2500, "rank_blocked", False, True, 0.25),
    "rows_bmap": ("lat40_F70", T_ROWS, True, True, 40 * 48 + 2 * 2500, "compact_blocked", False, True, 0.0),
    "drain_u16": ("lat20_F70", T_DRAIN, True, True, 20 * 48 + 2 * 1030, "compact_blocked", False, False, 0.25),
}
NONE_WINDOW = 1               # the window whose window_rows callback answers None


def _mp_accb(name):
    _, _, _, acc16, _, _, weighted, _, _ = MP_CASES[name]
    return 2 if acc16 and not weighted else 4


def _mp_windows(name):
    """The windows the case must be counted in: [(w0, w1, sorted items or None)]."""
    case, _, per_items, _, lds, _, _, _, _ = MP_CASES[name]
    F1, _, cand = _level(case)
    C, accb = len(cand), _mp_accb(name)
    if per_items:
        wins = _ref_windows(cand, F1, 1024, lds, accb)
        assert wins is not None
        return [(w0, w1, it) for w0, w1, _, it in wins]
    sw, cap = prim.slab_width(np.unique(cand).size, C, lds, accb)
    assert sw > 0 and cap < C
    cap = -(-C // -(-C // cap))
    assert C % cap                                                 # the last window is shorter
    return [(w0, min(C, w0 + cap), None) for w0 in range(0, C, cap)]


def _support(B, cand, w=None):
    """Rows (or their weights' sum) that hold all items of each candidate, int64 [C]."""
    has, out = B.astype(bool), np.empty(len(cand), np.int64)
    for s in range(0, len(cand), 128):
        m = has[:, cand[s:s + 128]].all(2)
        out[s:s + 128] = m.sum(0) if w is None else (m * w[:, None]).sum(0)
    return out


@functools.lru_cache(maxsize=None)
def _mp_case(name):
    """-> (B int64 [T, F1], word weights int32 [W] or None, reference counts int64 [C], windows)."""
    case, T, _, _, _, _, weighted, rows, _ = MP_CASES[name]
    F1, _, cand = _level(case)
    rng = np.random.default_rng(sum(map(ord, name)))
    ranks = np.unique(cand)
    wins = _mp_windows(name)
    if T == T_DRAIN:
        # four of the items in every row, the others in 97 % of them
        B = (rng.random((T, F1)) < 0.97).astype(np.int64)
        B[:, ranks[:4]] = 1
    else:
        B = (rng.random((T, F1)) < rng.permutation(np.linspace(0.15, 0.9, F1))).astype(np.int64)
        thin = np.arange(T) % 3 == 2
        B[thin] &= rng.random((int(thin.sum()), F1)) < 0.2                    # sparse rows: few of a window's items
        B[np.ix_(np.arange(T) % 8 < 2, ranks)] = 1                            # planted full rows
    if rows:
        # no row holds 3 of the last window's items (the top ranks): that window has no rows
        last = wins[-1][2]
        sub = B[:, last]
        sub[np.cumsum(sub, 1) > 2] = 0
        B[:, last] = sub
    B[B.sum(1) < 2, :2] = 1
    w = rng.integers(1, 9, (T + 63) // 64).astype(np.int32) if weighted else None
    ref = _support(B, cand, None if w is None else np.repeat(w, 64)[:T].astype(np.int64))
    assert ref.max() > 255 and np.unique(ref).size > 50
    if T == T_DRAIN:
        assert ref.max() == T > 65535 and (ref > 65535).sum() > 100 and -(-T // 256) > 65535 // 256
    if rows:
        w0, w1, last = wins[-1]
        assert not ref[w0:w1].any() and ref[:w0].any()            # the skipped window's true counts are all 0
        assert (B[:, last].sum(1) < 3).all()
        assert len(wins) >= 4 and NONE_WINDOW < len(wins) - 1
    return B, w, ref, wins


def test_multipass_references(native):
    for name, (case, T, per_items, _, _, _, _, _, _) in MP_CASES.items():
        B, w, ref, wins = _mp_case(name)
        assert T % 64 and T > 1024 and B.shape[0] == T
        assert len(wins) >= (2 if case == "lat20_F70" else 3), (name, len(wins))
        if per_items and case == "lat40_F70":                      # at least 3 windows with differing item sets
            assert len({tuple(it.tolist()) for _, _, it in wins}) >= 3
            assert wins[-1][2].size < wins[0][2].size == 40
    assert [len(_level(c)[2]) for c in ("lat20_F70", "lat40_F70")] == [1140, 9880]


def _level_bitmap(B, used, kind):
    """The level's bitmap as FastApriori._bitmaps builds it: rank-indexed [F1][Wp] (bmap None) or
    the used items' rows only with the rank -> row map; row-major or 8-word blocked.
    -> (bm, bmap, bm_rows: slab row u of the level -> bitmap row)."""
    T, F1 = B.shape
    Wp = max(64, -(-((T + 63) // 64) // 64) * 64)
    bits = B.T.astype(bool)
    bmap = None
    if kind.startswith("compact"):
        bits = bits[used]
        imap = np.full(F1, -1, np.int32)
        imap[used] = np.arange(used.size, dtype=np.int32)
        bmap = torch.from_numpy(imap).to(DEV)
    bm, _ = _dev_bitmap(bits, (T + 63) // 64, kind.endswith("blocked"), Wp=Wp)
    used_t = torch.from_numpy(used.astype(np.int64)).to(DEV)
    bm_rows = (bmap[used_t] if bmap is not None else used_t).to(torch.int32).contiguous()
    return bm, bmap, bm_rows


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(MP_CASES))
def test_dl_count_multipass(dl_state, tune, name):
    case, T, per_items, acc16, lds, bm_kind, weighted, rows, sup_frac = MP_CASES[name]
    S, K = dl_state, prim.dl()
    B, w, ref, wins = _mp_case(name)
    F1, ch, cand = _level(case)
    C, k = len(cand), cand.shape[1]
    c, P0 = run_bundle(S, F1, ch, 1, 1.0)
    used = np.flatnonzero(np.unpackbits(c[K.kDlBits:K.kDlBits + (F1 + 63) // 64].view(np.uint8), bitorder="little")[:F1])
    assert np.array_equal(used, np.unique(cand)) and c[K.kDlNUsed] == used.size
    tune(mp_window_items=per_items, dl_acc16=acc16, lane_deal_min_rows=-1)
    roff, ranks = (t.to(DEV) for t in _csr(B))
    bm, bmap, bm_rows = _level_bitmap(B, used, bm_kind)
    wword = None if w is None else torch.from_numpy(w).to(DEV)
    seen = []

    def window_rows(used_w, n_cand):
        # FastApriori._window_rows without its estimate: the window's items over the rows that
        # hold >= k of them; one window counts the level's rows instead
        used_t = torch.from_numpy(used_w.astype(np.int64)).to(DEV)
        rows_w = (bmap[used_t] if bmap is not None else used_t).to(torch.int32).contiguous()
        got = prim.window_bitmap(bm, rows_w, (T + 63) // 64, k)
        seen.append((used_w.copy(), n_cand, got[0]))
        return None if len(seen) - 1 == NONE_WINDOW else got

    hip = _native.hip()
    try:
        if T == T_DRAIN:
            hip.fa_hip_debug_slab_max_wg(1)        # one workgroup walks every slab: its u16 counters must drain
        out = prim.dl_count_multipass(S, F1, used.size, C, lds, roff, ranks, None, T, wword, bm, bm_rows, sup_frac, DEV,
                                      bmap=bmap, window_rows=window_rows if rows else None)
        torch.cuda.synchronize()
    finally:
        hip.fa_hip_debug_slab_max_wg(0)
    plan = dict(prim.LAST_LEVEL_PLAN)
    assert out.dtype == torch.int32 and tuple(out.shape) == (C,)
    got = out.cpu().numpy().astype(np.int64)
    bad = np.flatnonzero(got != ref)
    assert bad.size == 0, (bad.size, bad[:6], got[bad[:6]], ref[bad[:6]], [(a, b) for a, b, _ in wins])
    skipped = 0
    if rows:
        has = B.astype(bool)
        assert [(u.tolist(), n) for u, n, _ in seen] == [(it.tolist(), w1 - w0) for w0, w1, it in wins]
        assert [kk for _, _, kk in seen] == [int((has[:, it].sum(1) >= k).sum()) for _, _, it in wins]
        assert seen[-1][2] == 0 and all(kk > 0 for _, _, kk in seen[:-1])        # the last window was skipped
        assert all(kk < T for _, _, kk in seen)                                  # and every other one lost rows
        skipped = 1
    assert plan["kernel"] == "slab_dev_multi" and plan["C"] == C
    assert plan["passes"] == len(wins) - skipped
    assert plan["windows_trimmed"] == (len(wins) - 1 if rows else 0)
    del P0
