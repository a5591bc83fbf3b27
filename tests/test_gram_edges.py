"""Edge shapes of the dense k = 2 path: the bit-matrix Gram kernels of count.hip
(k_pair_gram_fp4, the i8 form k_pair_gram_mfma4<false>, k_pair_gram_popc) through
ops.primitives.pair_counts_gram.

As in test_kernel_edges.py every input is built on purpose -- from a dense 0/1 matrix
B[T, F1] (seeded where random) or from explicit words -- to reach one thing each: the
number of K stages a workgroup runs and the valid words of its last one, the K split
over workgroups, the tile and wave sub-tile edges, views that start and end inside an
8-word block, the f32 range of the FP4 sums, and the weight-class launch list.  The
expected counts come from B in numpy (float64 Gram, exact below 2^53) or from a closed
form plus a numpy popcount, never from another path of this project, and every
comparison is exact equality over the whole output.

What every case has in common:
  * each item has its own density, the last item is in every transaction and two items
    are identical: a transposed or misplaced tile changes the result;
  * every word of the bitmap buffer outside the view [w0, w0 + W) is all ones, before
    the view and from its end to the padded end of the buffer: a kernel that reads one
    word too many counts 64 transactions that are not there;
  * the diagonal and the lower triangle of the raw output stay 0;
  * on the device each case runs through all three kernels, in the row-major layout
    and in 8-word blocks; the row-major form runs on "cpu" (fa_cpu_pair_gram) too,
    which proves the builders and the references where there is no GPU.
target_wgs = 1 makes one workgroup per item tile walk all W words.
"""
import functools

import numpy as np
import pytest
import torch

from fastapriori_amd import ops
from fastapriori_amd.models.apriori import FastApriori
from fastapriori_amd.ops import primitives as prim

DEV = torch.device("cuda", 0)
KERNELS = {"fp4": dict(fp4=True), "i8": dict(fp4=False), "popc": dict(force_popc=True)}
# (device, kernel, layout)
GPU = [pytest.param("cuda", k, lay, marks=pytest.mark.gpu, id=f"cuda-{k}-{lay}")
       for k in KERNELS for lay in ("rows", "blocks")]
GPU_ROWS = [pytest.param("cuda", k, "rows", marks=pytest.mark.gpu, id=f"cuda-{k}-rows") for k in KERNELS]
CPU = [pytest.param("cpu", None, "rows", id="cpu")]
BOTH, BOTH_ROWS = CPU + GPU, CPU + GPU_ROWS

ONES = np.uint64(0xFFFFFFFFFFFFFFFF)


# ---------------------------------------------------------------------------
# builders and references
# ---------------------------------------------------------------------------
def _gram(B, w=None):
    """Upper triangle of B.T @ diag(w) @ B, int64.  The product runs in float64 (BLAS):
    every entry is an integer below 2^53, so it is exact."""
    A = B.astype(np.float64)
    L = A.T if w is None else A.T * np.asarray(w, np.float64)
    G = np.rint(L @ A).astype(np.int64)
    assert G.max(initial=0) < 1 << 53
    return np.triu(G, 1)


@functools.lru_cache(maxsize=None)
def _matrix(F1, W, seed):
    """B[64 W, F1]: item i with its own density; the last item all ones; items 0 and
    F1 - 2 identical (F1 >= 3)."""
    rng = np.random.default_rng(seed)
    dens = rng.uniform(0.05, 0.95, F1)
    B = (rng.random((64 * W, F1)) < dens).astype(np.int64)
    B[:, F1 - 1] = 1
    if F1 >= 3:
        B[:, F1 - 2] = B[:, 0]
    B.setflags(write=False)
    return B


def _words(B):
    """B[64 W, F1] -> uint64 [F1, W]: transaction t is bit t & 63 of word t >> 6."""
    assert B.shape[0] % 64 == 0
    rows = np.ascontiguousarray(B.T.astype(np.uint8))
    return np.ascontiguousarray(np.packbits(rows, axis=1, bitorder="little")).view(np.uint64).reshape(B.shape[1], -1)


def _buffer(words, w0=0):
    """The view's words at [w0, w0 + W) of a row-major buffer [F1, Wp] whose other words
    are all ones.  Wp is a multiple of 8 with at least one whole block past the view."""
    F1, W = words.shape
    Wp = (w0 + W + 7) // 8 * 8 + 8
    buf = np.full((F1, Wp), ONES, np.uint64)
    buf[:, w0:w0 + W] = words
    assert (buf[:, :w0] == ONES).all() and (buf[:, w0 + W:] == ONES).all() and Wp - (w0 + W) >= 8
    return buf


def _bitmap(buf, dev, layout):
    bm = torch.from_numpy(buf.view(np.int64))
    if dev == "cpu":
        assert layout == "rows"
        return bm
    bm = bm.to(DEV)
    return prim.to_blocked(bm) if layout == "blocks" else bm


def _counts(bm, W, dev, kernel, wword=None, wcls=None, **kw):
    """pair_counts_gram -> int64 numpy [F1, F1]; the device's raw int32 matrix is checked
    for its untouched diagonal and lower triangle before it is widened."""
    F1 = bm.shape[1] if bm.dim() == 3 else bm.shape[0]
    on_gpu = dev != "cpu"
    got = prim.pair_counts_gram(bm, W, wword, wcls, raw=on_gpu, **KERNELS.get(kernel, {}), **kw)
    assert got.shape == (F1, F1) and got.dtype == (torch.int32 if on_gpu else torch.int64)
    got = got.cpu().numpy().astype(np.int64)
    assert not np.tril(got).any(), "diagonal or lower triangle written"
    return got


def _check_unit(F1, W, seed, dev, kernel, layout, w0=0, **kw):
    B = _matrix(F1, W, seed)
    ref = _gram(B)
    assert ref[0, F1 - 1] == B[:, 0].sum() and (F1 < 3 or ref[0, F1 - 2] == B[:, 0].sum())
    bm = _bitmap(_buffer(_words(B), w0), dev, layout)
    got = _counts(bm, W, dev, kernel, w0=w0, **kw)
    assert np.array_equal(got, ref)


# ---------------------------------------------------------------------------
# 1. stage counts and tails: one tile, one workgroup over all W words.  The FP4 kernel
#    runs ceil(W / 8) = 1 .. 9 stages (its LDS double buffer is reused from the third on)
#    with 1 .. 8 valid words in the last; the i8 kernel ceil(W / 16) = 1 .. 5 steps; the
#    popcount kernel ceil(W / 32) = 1 .. 3.
# ---------------------------------------------------------------------------
STAGE_WS = [1, 7, 8, 9, 15, 16, 17, 23, 24, 25, 33, 40, 41, 63, 64, 65]


@pytest.mark.parametrize("dev,kernel,layout", BOTH)
@pytest.mark.parametrize("W", STAGE_WS)
def test_gram_stages_and_tails(native, W, dev, kernel, layout):
    _check_unit(40, W, 1000 + W, dev, kernel, layout, target_wgs=1)


# ---------------------------------------------------------------------------
# 2. K split: nk > 1 chunks with a short last one.  Matrix-core launchers (chunks of a
#    multiple of 16 words): (33, 2) -> 32 + 1, (48, 3) -> 16 + 16 + 16, (17, 4) -> 16 + 1,
#    (65, 2) -> 48 + 17; the popcount launcher (multiples of 32): 32 + 1, 32 + 16, 17,
#    64 + 1.  F1 = 257: 3 tiles of 256 (15 of 64), so with target_wgs = 7 (40) the
#    matrix-core (popcount) grid is tiles x chunks and both tp = logical % ntp and
#    kc = logical / ntp vary; 1 and 3 leave one chunk per tile.
# ---------------------------------------------------------------------------
SPLITS = [(40, 33, 2), (40, 48, 3), (40, 17, 4), (40, 65, 2), (257, 41, 1), (257, 41, 3), (257, 41, 7), (257, 41, 40)]


@pytest.mark.parametrize("dev,kernel,layout", BOTH)
@pytest.mark.parametrize("F1,W,target_wgs", SPLITS)
def test_gram_k_split(native, F1, W, target_wgs, dev, kernel, layout):
    _check_unit(F1, W, 2000 + F1 + W, dev, kernel, layout, target_wgs=target_wgs)


# ---------------------------------------------------------------------------
# 3. tile geometry (256-item workgroup tiles of 2 x 2 wave sub-tiles of 128; 64-item
#    popcount tiles): the minimum F1, the sub-tile edge at 128 / 129 (the wave below the
#    diagonal of a diagonal tile is skipped), a second tile of one item (tile (1, 1) holds
#    no pair), three tiles.  W = 24: three FP4 stages in one workgroup (target_wgs = 1),
#    or two chunks of 16 and 8 words at the default.
# ---------------------------------------------------------------------------
TILE_F1 = [2, 3, 32, 33, 128, 129, 255, 256, 257, 512, 513]


@pytest.mark.parametrize("dev,kernel,layout", BOTH)
@pytest.mark.parametrize("target_wgs", [1, 4096])
@pytest.mark.parametrize("F1", TILE_F1)
def test_gram_tile_geometry(native, F1, target_wgs, dev, kernel, layout):
    _check_unit(F1, 24, 3000 + F1, dev, kernel, layout, target_wgs=target_wgs)


# ---------------------------------------------------------------------------
# 4. views: words [w0, w0 + W) of a wider buffer, row-major (row stride > W) and in 8-word
#    blocks (BmView::woff = w0 & 7), starting and ending inside a block
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("dev,kernel,layout", BOTH)
@pytest.mark.parametrize("W", [19, 32])
@pytest.mark.parametrize("w0", [0, 1, 7, 8, 9, 13])
def test_gram_views(native, w0, W, dev, kernel, layout):
    _check_unit(70, W, 4000 + 100 * w0 + W, dev, kernel, layout, w0=w0, target_wgs=1)
    _check_unit(70, W, 4000 + 100 * w0 + W, dev, kernel, layout, w0=w0)


@pytest.mark.gpu
@pytest.mark.parametrize("woff", [8, -1])
def test_gram_rejects_offset_outside_block(woff):
    """The launchers take an in-block offset of 0 .. 7 only: anything else is -EINVAL and
    no kernel runs (the output stays as it was)."""
    F1, W = 70, 19
    buf = _buffer(_words(_matrix(F1, W, 4900)), 8)
    bm = torch.from_numpy(buf.view(np.int64)).to(DEV)
    out = torch.full((F1, F1), 7, dtype=torch.int32, device=DEV)
    st = torch.cuda.current_stream(DEV).cuda_stream
    lib = ops._native.hip()
    for fp4 in (1, 0):
        assert lib.fa_hip_pair_gram_mfma(bm.data_ptr(), F1, bm.stride(0), 8, woff, W, out.data_ptr(), 1, 1, fp4, st) == -22
    assert lib.fa_hip_pair_gram_popc(bm.data_ptr(), F1, bm.stride(0), 8, woff, W, None, out.data_ptr(), 1, st) == -22
    torch.cuda.synchronize(DEV)
    assert bool((out == 7).all())


# ---------------------------------------------------------------------------
# 5. the f32 range of the FP4 sums.  The launcher caps an FP4 chunk at 2^18 words = 2^24
#    transactions, so every partial sum is an integer <= 2^24 and exact in f32; in
#    [2^23, 2^24) f32 spacing is 1, so the conversion to uint32 must not add 0.5 first (a
#    tie, rounded to even: every odd count would come out one too large).  Words are
#    built directly (F1 = 3, about 6 MB a buffer); expected counts are a closed form,
#    checked against a numpy popcount of a & b.
# ---------------------------------------------------------------------------
def _popcount_pairs(words):
    F1 = words.shape[0]
    ref = np.zeros((F1, F1), np.int64)
    for i in range(F1):
        for j in range(i + 1, F1):
            ref[i, j] = int(np.unpackbits((words[i] & words[j]).view(np.uint8)).sum(dtype=np.int64))
    return ref


@functools.lru_cache(maxsize=None)
def _f32_odd_counts():
    W = 1 << 18                                       # one FP4 chunk, exactly at the cap
    words = np.zeros((3, W), np.uint64)
    words[0] = ONES
    words[1] = ONES
    words[1, W - 1] = ONES ^ np.uint64(1 << 40)       # one transaction short
    words[2, :W // 2] = ONES
    words[2, W // 2] = np.uint64(1)                   # one transaction more
    ref = np.zeros((3, 3), np.int64)
    ref[0, 1] = (1 << 24) - 1
    ref[0, 2] = ref[1, 2] = (1 << 23) + 1
    assert np.array_equal(ref, _popcount_pairs(words))
    return _buffer(words), W, ref


@functools.lru_cache(maxsize=None)
def _f32_cap():
    W = (1 << 18) + 24                                # chunks of 2^18 and 24 words
    words = np.zeros((3, W), np.uint64)
    words[0] = ONES
    words[1] = ONES
    words[1, W - 24:] = ONES ^ np.uint64(1)           # 63 transactions in each of the last 24 words
    words[2] = np.uint64(0x5555555555555555)
    ref = np.zeros((3, 3), np.int64)
    ref[0, 1] = (1 << 24) + 63 * 24
    ref[0, 2] = 32 * W
    ref[1, 2] = 32 * W - 24
    assert np.array_equal(ref, _popcount_pairs(words))
    return _buffer(words), W, ref


@pytest.mark.parametrize("dev,kernel,layout", BOTH_ROWS)
def test_gram_f32_odd_counts_from_2_23(native, dev, kernel, layout):
    """Pairs (0, 1) = 2^24 - 1 and (0, 2) = (1, 2) = 2^23 + 1 from one chunk of 2^18 words.
    With the `+ 0.5f` conversion this project had before, the FP4 kernel returned 2^24 and
    2^23 + 2 (IEEE ties-to-even); the i8 and popcount kernels count in integers."""
    buf, W, ref = _f32_odd_counts()
    got = _counts(_bitmap(buf, dev, layout), W, dev, kernel, target_wgs=1)
    print("f32 odd counts", dev, kernel, got[np.triu_indices(3, 1)].tolist(), "expected",
          ref[np.triu_indices(3, 1)].tolist())
    assert np.array_equal(got, ref)


@pytest.mark.parametrize("dev,kernel,layout", BOTH_ROWS)
def test_gram_f32_chunk_cap(native, dev, kernel, layout):
    """Pair (0, 1) = 2^24 + 63 * 24 from 2^18 + 24 words asked of one workgroup: the FP4
    launch must split at 2^18 words (2^24 + 0 and 63 * 24, both exact); one chunk would add
    63 at a time above 2^24, where f32 holds even integers only."""
    buf, W, ref = _f32_cap()
    got = _counts(_bitmap(buf, dev, layout), W, dev, kernel, target_wgs=1)
    print("f32 chunk cap", dev, kernel, got[np.triu_indices(3, 1)].tolist(), "expected",
          ref[np.triu_indices(3, 1)].tolist())
    assert np.array_equal(got, ref)


# ---------------------------------------------------------------------------
# 6. weight classes: the launch list (gram_segments), the scaled matrix-core launches and
#    the popcount launches with per-word weights, candidate-mode word slices
# ---------------------------------------------------------------------------
MIN_CLASS = 16        # TUNING.gram_mfma_min_class_words in these tests (default 512)


def _wcls(classes):
    return (np.array([wt for wt, _ in classes], np.int64), np.array([n for _, n in classes], np.int64))


def _wword(classes):
    return np.concatenate([np.full(n, wt, np.int32) for wt, n in classes] + [np.zeros(0, np.int32)])


SEGMENT_CASES = {
    # id: ((weight, words) per class, W or None = all of them)
    "len_15": ([(3, 15)], None),
    "len_16": ([(3, 16)], None),
    "len_17": ([(3, 17)], None),
    "short_before_between_after": ([(3, 15), (5, 16), (2, 1), (7, 17), (1, 8), (1000, 40), (4, 2), (6, 3)], None),
    "long_first_and_last": ([(5, 16), (2, 1), (9, 15), (7, 17)], None),
    "only_short": ([(1, 3), (2, 15), (3, 1)], None),
    "adjacent_long": ([(1, 16), (2, 40), (3, 17)], None),
    "zero_word_class": ([(1, 20), (2, 0), (3, 5), (4, 0), (5, 30), (6, 0)], None),
    "W_cuts_long_class_to_long": ([(1, 20), (2, 40)], 20 + 16),
    "W_cuts_long_class_to_short": ([(1, 20), (2, 40)], 20 + 15),
    "W_cuts_long_class_after_short_run": ([(1, 3), (2, 40)], 3 + 15),
    "W_cuts_short_class": ([(1, 20), (2, 9), (3, 30)], 25),
    "W_at_class_end": ([(1, 20), (2, 9), (3, 30)], 29),
    "W_0": ([(1, 20), (2, 9)], 0),
}


@pytest.mark.parametrize("case", list(SEGMENT_CASES))
def test_gram_segments_partition(tune, case):
    """The launch list is in order, partitions [0, W) exactly, gives every class piece of
    >= MIN_CLASS words its own matrix-core launch and nothing else one, and carries the
    weight of every word: a matrix-core segment's scale, wword under a popcount segment."""
    classes, W = SEGMENT_CASES[case]
    tune(gram_mfma_min_class_words=MIN_CLASS)
    wword = _wword(classes)
    W = wword.size if W is None else W
    assert W <= wword.size
    segs = prim.gram_segments(W, True, _wcls(classes))
    at = 0
    for a, b, wt in segs:
        assert a == at and b > a and wt >= 0, segs
        at = b
    assert at == W, segs
    rebuilt = np.full(W, -1, np.int64)
    for a, b, wt in segs:
        rebuilt[a:b] = wt if wt > 0 else wword[a:b]
    assert np.array_equal(rebuilt, wword[:W]), segs
    cum = np.cumsum([n for _, n in classes])
    beg, end = np.minimum(cum - [n for _, n in classes], W), np.minimum(cum, W)
    long_pieces = [(int(a), int(b), wt) for (wt, _), a, b in zip(classes, beg, end) if b - a >= MIN_CLASS]
    assert [s for s in segs if s[2] > 0] == long_pieces, segs
    # the same list with every class on the popcount Gram
    assert prim.gram_segments(W, True, _wcls(classes), force_popc=True) == ([(0, W, 0)] if W else [])


def test_gram_segments_unweighted_and_unclassed():
    assert prim.gram_segments(41, False) == [(0, 41, 1)]
    assert prim.gram_segments(41, False, force_popc=True) == [(0, 41, 0)]
    assert prim.gram_segments(41, True, None) == [(0, 41, 0)]


WEIGHTED_CLASSES = [(3, 15), (5, 16), (2, 1), (7, 17), (1, 8), (1000, 40)]
W_POISON = 1 << 20          # the weight of the words around the view's


def _weights(wword, dev):
    """wword inside a buffer whose other entries are W_POISON (the view starts 12 B in)."""
    buf = np.full(wword.size + 8, W_POISON, np.int32)
    buf[3:3 + wword.size] = wword
    t = torch.from_numpy(buf)
    return (t.to(DEV) if dev != "cpu" else t)[3:3 + wword.size]


@pytest.mark.parametrize("dev,kernel,layout", BOTH)
@pytest.mark.parametrize("w0", [0, 5])
def test_gram_weight_classes(native, tune, w0, dev, kernel, layout):
    """Popcount launches at words 0, 31 and 49 (wword + 4 a), scaled matrix-core launches
    at 15, 32 and 57 (off the 8-word blocks) of 16, 17 and 40 words."""
    tune(gram_mfma_min_class_words=MIN_CLASS)
    F1, wword, wcls = 70, _wword(WEIGHTED_CLASSES), _wcls(WEIGHTED_CLASSES)
    W = wword.size
    assert prim.gram_segments(W, True, wcls) == [(0, 15, 0), (15, 31, 5), (31, 32, 0), (32, 49, 7), (49, 57, 0),
                                                 (57, 97, 1000)]
    B = _matrix(F1, W, 6000)
    ref = _gram(B, np.repeat(wword.astype(np.int64), 64))
    assert ref.max() < 1 << 31
    bm = _bitmap(_buffer(_words(B), w0), dev, layout)
    got = _counts(bm, W, dev, kernel, wword=_weights(wword, dev), wcls=wcls, w0=w0)
    assert np.array_equal(got, ref)


SLICE_CLASSES = {100: [(1, 33), (4, 20), (2, 7), (9, 40)], 40: [(1, 9), (4, 17), (2, 3), (9, 11)]}


@pytest.mark.parametrize("dev,kernel,layout", BOTH)
@pytest.mark.parametrize("weighted", [False, True], ids=["unit", "weighted"])
@pytest.mark.parametrize("W", [100, 40])
@pytest.mark.parametrize("nr", [2, 3, 8])
def test_gram_candidate_slices(native, tune, nr, W, weighted, dev, kernel, layout):
    """Candidate parallelism (FastApriori._pairs): rank r of nr counts a 32-word-aligned
    slice of the words, whose neighbours in the buffer are the other ranks' words; the
    slices' counts add up to the whole Gram, and an empty slice gives zeros."""
    tune(gram_mfma_min_class_words=MIN_CLASS)
    F1, classes = 70, SLICE_CLASSES[W]
    wword, wcls = (_wword(classes), _wcls(classes)) if weighted else (None, None)
    assert wword is None or wword.size == W
    B = _matrix(F1, W, 7000 + W)
    ref = _gram(B, None if wword is None else np.repeat(wword.astype(np.int64), 64))
    bm = _bitmap(_buffer(_words(B)), dev, layout)
    ww = None if wword is None else _weights(wword, dev)
    total, at, empty = np.zeros((F1, F1), np.int64), 0, 0
    for r in range(nr):
        w0, w1 = (W * r // nr) // 32 * 32, (W if r == nr - 1 else (W * (r + 1) // nr) // 32 * 32)
        assert w0 == at and w1 >= w0
        at = w1
        got = _counts(bm, max(w1 - w0, 0), dev, kernel, wword=None if ww is None else ww[w0:w1],
                      wcls=FastApriori._slice_classes(wcls, w0, w1), w0=w0)
        if w1 == w0:
            empty += 1
            assert not got.any()
        else:
            lo = _gram(B[64 * w0:64 * w1], None if wword is None else np.repeat(wword[w0:w1].astype(np.int64), 64))
            assert np.array_equal(got, lo), (r, w0, w1)
        total += got
    # W = 40: ranks 0 .. nr - 2 round down to [0, 0) except rank 6 of 8, which takes [0, 32)
    assert at == W and (W != 40 or empty == (6 if nr == 8 else nr - 1))
    assert np.array_equal(total, ref)
