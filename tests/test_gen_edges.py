"""Edge shapes of the candidate generator (csrc/hip/gen.hip, csrc/host/apriori_gen.cpp).

The other generator tests feed Quest data with 60-150 frequent items and compare the device
with the project's own C++ apriori_gen, so only one word per lane of ag_row_bits runs and no
itemset is placed on a bitset word's edge.  Here every input is built on purpose -- lattices
(all m-subsets of N placed ranks), planted cliques, a bipartite graph with a few triangles --
and the expected candidates come from a brute-force apriori-gen over a set of tuples, straight
from the definition, never from another path of this project.  All values are integers and
every comparison is exact equality over the whole output.

1. one level (ops.apriori_gen_device; on "cpu" ops.host.apriori_gen, which proves the builders
   where there is no GPU and checks the C++ generator, its bitset path included, at the same edges)
2. the host loop's chains (ops.primitives.apriori_gen_chain: fa_hip_ag_chain, ag_chain_dev)
3. the device bundle's speculative levels (ops.primitives.dl_bundle_gen with max_levels > 1)

tests/test_dl_plan_edges.py counts section 3's bundles through the device piece plan.
"""
import functools
import itertools
import math

import numpy as np
import pytest
import torch

from fastapriori_amd import ops
from fastapriori_amd.ops import primitives as prim

DEV = torch.device("cuda", 0)
BOTH = ["cpu", pytest.param("cuda", marks=pytest.mark.gpu)]


# ---------------------------------------------------------------------------
# the reference
# ---------------------------------------------------------------------------
def _brute(rows):
    """apriori-gen by the definition.  rows: ascending tuples of m items in lexicographic
    order.  The extensions of x are the last items y > x[m-1] of x's class (the rows with
    x's first m-1 items) such that x - {x[p]} + {y} is a row for every p < m-1.
    Returns (extensions per row int64 [n], candidate rows (x, y) in lexicographic order)."""
    have, m, cls = set(rows), len(rows[0]), {}
    for x in rows:
        cls.setdefault(x[:-1], []).append(x[-1])
    cnt, cand = np.zeros(len(rows), np.int64), []
    for i, x in enumerate(rows):
        for y in cls[x[:-1]]:
            if y > x[-1] and all(x[:p] + x[p + 1:] + (y,) in have for p in range(m - 1)):
                cand.append(x + (y,))
                cnt[i] += 1
    assert cand == sorted(cand)
    return cnt, cand


def _brute_pairs(rows, F1):
    """The same for m = 2 from a dense adjacency matrix (A[i, j], i < j), chunked: row
    (i, j) is extended by the y adjacent to both; A is upper triangular, so y > j."""
    A = np.zeros((F1, F1), bool)
    A[rows[:, 0], rows[:, 1]] = True
    cnt, parts = np.zeros(len(rows), np.int64), []
    for s in range(0, len(rows), 8192):
        r = rows[s:s + 8192]
        M = A[r[:, 0]] & A[r[:, 1]]
        cnt[s:s + 8192] = M.sum(1)
        ii, y = np.nonzero(M)
        parts.append(np.column_stack([r[ii], y]))
    return cnt, np.concatenate(parts).astype(np.int32)


def _arr(rows, w):
    return np.ascontiguousarray(np.array(rows, np.int32).reshape(-1, w))


def _chain(rows, depth=64):
    """The brute force iterated: [(rows int32 [n, m], cnt int64 [n], candidates int32 [C, m + 1])]
    level after level, each level's candidates the next one's rows, up to and including
    the first level without candidates."""
    out = []
    while rows and len(out) < depth:
        m = len(rows[0])
        cnt, cand = _brute(rows)
        out.append((_arr(rows, m), cnt, _arr(cand, m + 1)))
        rows = cand
    return out


# ---------------------------------------------------------------------------
# input families
# ---------------------------------------------------------------------------
def _nwl(F1):
    """Bitset words per lane of ag_row_bits<NWL> for F1 ranks."""
    nw = (F1 + 63) // 64
    return 1 if nw <= 64 else 2 if nw <= 128 else 4 if nw <= 256 else 8


def _placed(F1, N):
    """N ranks of [0, F1) placed on the bitset's edges, the most telling first: bits 63 / 0
    of words 0 / 1, the top rank, bit 62, rank 0, the last word one lane owns and the
    word after it (words NWL - 1 and NWL), words 1 / 2, the middle of word 0; then spread."""
    g = _nwl(F1)
    first = [63, 64, F1 - 1, 62, F1 - 2, 0, 64 * g - 1, 64 * g, 128, 127, 32, 31]
    spread = np.linspace(1, F1 - 3, 97).astype(int).tolist() + list(range(F1))
    out = []
    for r in first + spread:
        if 0 <= r < F1 and r not in out:
            out.append(r)
        if len(out) == N:
            break
    assert len(out) == N
    return tuple(sorted(out))


def _lattice(ranks, m, drop=()):
    """All m-subsets of the ranks without the rows at the indices `drop` -> (rows, the
    expected candidates by a count that needs no generator: the (m+1)-subsets none of
    whose m-subsets was dropped)."""
    full = list(itertools.combinations(ranks, m))
    gone = {full[d] for d in drop}
    rows = [x for x in full if x not in gone]
    want = [c for c in itertools.combinations(ranks, m + 1)
            if not any(s in gone for s in itertools.combinations(c, m))]
    N = len(ranks)
    if not drop:
        assert len(want) == math.comb(N, m + 1)
    elif len(drop) == 1:
        assert len(want) == math.comb(N, m + 1) - (N - m)      # the dropped row's supersets
    return rows, want


def _edge_flags(rows, cnt, cand, F1):
    """Which bitset edges a case reaches, read off the reference: a row whose last item is on
    bit 63 with an extension (in a later word); a row ending on bit 62 extended by bit 63;
    the top rank as an extension."""
    m = rows.shape[1]
    last, y = cand[:, m - 1], cand[:, m]
    return dict(bit63=bool(((last & 63) == 63).any()),
                bit62_63=bool((((last & 63) == 62) & (y == last + 1)).any()),
                top=bool((y == F1 - 1).any()))


def _cliques(seed):
    """Planted cliques: every pair inside each of 8 overlapping rank sets of 5-9 items out of a
    pool of 36, 60 noise pairs, a seeded ~10 % of all pairs removed.  F1 = 130 (3 words)."""
    rng, F1 = np.random.default_rng(900 + seed), 130
    pool = np.union1d([62, 63, 64, 127, 128, 129], rng.choice(F1, 30, replace=False))
    pairs = set()
    for _ in range(8):
        s = np.sort(rng.choice(pool, int(rng.integers(5, 10)), replace=False)).tolist()
        pairs.update(itertools.combinations(s, 2))
    for _ in range(60):
        a, b = np.sort(rng.choice(pool, 2, replace=False)).tolist()
        pairs.add((a, b))
    rows = sorted(pairs)
    keep = rng.random(len(rows)) >= 0.1
    return [r for r, k in zip(rows, keep) if k], F1


def _bipartite():
    """The pairs (i, j), i < 520 <= j < 1040: 270 400 rows and no triangle; then one triangle
    each from the ranks 1040 .. 1043, tied to one pair apiece, and the pair (2, 9), which
    closes a triangle with every j.  More rows than k_ag_rows' grid has waves (262 144)."""
    F1 = 1044
    i, j = np.divmod(np.arange(520 * 520), 520)
    extra = [(2, 9)]
    for z, (a, b) in zip(range(1040, 1044), [(0, 520), (504, 581), (504, 582), (519, 1039)]):
        extra += [(a, z), (b, z)]
    rows = np.concatenate([np.stack([i, j + 520], 1), np.array(extra)])
    rows = np.ascontiguousarray(rows[np.lexsort((rows[:, 1], rows[:, 0]))], np.int32)
    return rows, F1


F1_SIZES = [64, 65, 4096, 4097, 8192, 8193, 16384, 16385, 32768]
PROBE_M = [2, 3, 4, 5, 6, 9, 10, 13]          # m - 1 = 1 .. 5, 8, 9, 12: every remainder of the 4-wide loop
LONG_M = [40, 41, 63, 64, 65, 66]             # 64: the last wave-parallel probe; 65, 66: the serial path

GEN_CASES = [f"pairs12_F{F1}{d}" for F1 in F1_SIZES for d in ("", "_del2")] + \
            [f"probe_m{m}_F{F1}" for m in PROBE_M for F1 in (70, 8193)] + \
            [f"long_m{m}{d}" for m in LONG_M for d in ("", "_del1")] + \
            ["one_row", "classes_of_one", "cliques_s1", "cliques_s2", "cliques_s3", "bipartite"]


@functools.lru_cache(maxsize=None)
def _gen_case(name):
    """-> (rows int32 [n, m], F1, extensions per row int64 [n], candidates int32 [C, m + 1])."""
    kind, _, rest = name.partition("_")
    if name == "bipartite":
        rows, F1 = _bipartite()
        cnt, cand = _brute_pairs(rows, F1)
        assert len(rows) == 270400 + 9 and len(rows) > 65536 * 4
        assert len(cand) == 520 + 4 and cnt.max() == 520
        at = np.flatnonzero(cnt)                    # triangles on both sides of the grid's first sweep
        assert at.tolist() == [0, 1041, 262143, 262144, 270403]
        return rows, F1, cnt, cand
    want = None
    if kind == "pairs12":
        F1 = int(rest.split("_")[0][1:])
        ranks, m = _placed(F1, 12), 2
        # dropped: the last row (the two top ranks: the class of F1 - 2 disappears) and a middle one
        rows, want = _lattice(ranks, m, (65, 21) if name.endswith("_del2") else ())
        if name.endswith("_del2"):
            assert len(want) == math.comb(12, 3) - 2 * 10
    elif kind == "probe":
        m, F1 = int(rest.split("_")[0][1:]), int(rest.split("_")[1][1:])
        rows, want = _lattice(_placed(F1, m + 3), m)
    elif kind == "long":
        # the m + 1 ranks up to 127, bit 63 of word 1 (from m = 64 on they start in word 0),
        # and the top rank, in word 2
        m, F1 = int(rest.split("_")[0][1:]), 130
        n = math.comb(m + 2, m)
        # dropped: the last row, the m top ranks.  The rows that end on the second rank from
        # the top then look up a class that no longer exists (the serial path's sp < 0)
        rows, want = _lattice(tuple(range(127 - m, 128)) + (F1 - 1,), m, (n - 1,) if name.endswith("_del1") else ())
    elif name == "one_row":
        rows, F1 = [(5, 63)], 70
    elif name == "classes_of_one":
        rows, F1 = [(2 * q, 2 * q + 1 + (q % 3)) for q in range(40)], 130
    else:
        rows, F1 = _cliques(int(name[-1]))
    cnt, cand = _brute(rows)
    m = len(rows[0])
    rows, cand = _arr(rows, m), _arr(cand, m + 1)
    if want is not None:
        assert np.array_equal(cand, _arr(want, m + 1))
        fl = _edge_flags(rows, cnt, cand, F1)
        assert fl["top"], fl
        if kind != "probe" and F1 > 64 and "_del" not in name:
            assert fl["bit63"] and fl["bit62_63"], fl
        if kind == "pairs12" and F1 > 64 and "_del" not in name:
            g = _nwl(F1)                             # an itemset across the lane's last word and the next
            assert ((cand[:, 1] >> 6 == g - 1) & (cand[:, 2] >> 6 == g)).any()
    elif kind == "cliques":
        assert {0, 1} <= set(cnt.tolist()) and cnt.max() >= 4
        assert np.array_equal(cand, _brute_pairs(rows, F1)[1])       # the dense form agrees
    else:
        assert len(cand) == 0
    return rows, F1, cnt, cand


def _check_level(got, cnt, cand):
    """got: (prefix_idx, ext_off, ext[, candidate rows]) as ops.host.apriori_gen returns them."""
    pidx = np.flatnonzero(cnt)
    assert got[0].dtype == np.int32 and np.array_equal(got[0], pidx)
    assert got[1].dtype == np.int64 and np.array_equal(got[1], np.concatenate([[0], np.cumsum(cnt[pidx])]))
    assert got[2].dtype == np.int32 and np.array_equal(got[2], cand[:, -1])
    if len(got) > 3:
        assert got[3].dtype == np.int32 and got[3].shape == cand.shape and np.array_equal(got[3], cand)


# ---------------------------------------------------------------------------
# 1. one level: fa_hip_ag_gen (k_ag_insert, k_ag_ext, k_ag_rows<., NWL>) / fa_apriori_gen
# ---------------------------------------------------------------------------
def test_nwl_sizes():
    # the F1 sizes run every lane width at its last size and the next one at its first;
    # at 4097 word 64 is lane 32's first and word 65 does not exist
    assert [_nwl(F1) for F1 in F1_SIZES] == [1, 1, 1, 2, 2, 4, 4, 8, 8]
    assert prim.dl().kAgMaxF1 == F1_SIZES[-1]
    for F1 in F1_SIZES[2:]:
        assert {0, 31, 32, 62, 63, 64, 127, 128, F1 - 2, F1 - 1, 64 * _nwl(F1) - 1, 64 * _nwl(F1)} <= set(_placed(F1, 12))
    assert [(4097 + 63) // 64 % 2, (8193 + 63) // 64 % 4, (16385 + 63) // 64 % 8] == [1, 1, 1]


@pytest.mark.parametrize("dev", BOTH)
@pytest.mark.parametrize("case", GEN_CASES)
def test_gen_one_level(native, case, dev):
    rows, F1, cnt, cand = _gen_case(case)
    if dev == "cpu":
        got = ops.host.apriori_gen(rows)
    else:
        got = ops.apriori_gen_device(rows, F1, DEV, want_rows=True)
    _check_level(got, cnt, cand)


# ---------------------------------------------------------------------------
# 2. the host loop's chains: fa_hip_ag_chain, and ag_chain_dev's batches of kAgdBatch = 4
#    device-sized levels for first_free chains
# ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _chain_case(name):
    """-> (F1, _chain of the case's pairs).  lat{N}_F{F1}: the pairs of N placed ranks, whose
    chain is known in advance: C(N, 3), C(N, 4), .., 1 candidates, then none."""
    if name.startswith("lat"):
        N, F1 = int(name[3:].split("_")[0]), int(name.split("_F")[1])
        ranks = _placed(F1, N)
        ch = _chain(_lattice(ranks, 2)[0])
        assert [len(c) for _, _, c in ch] == [math.comb(N, k) for k in range(3, N + 1)] + [0]
        for k, (_, _, c) in enumerate(ch[:-1]):
            assert np.array_equal(c, _arr(list(itertools.combinations(ranks, k + 3)), k + 3))
        fl = _edge_flags(*ch[0], F1)
        assert fl["top"] and fl["bit63"] and fl["bit62_63"], fl
        return F1, ch
    rows, F1 = _cliques(int(name[-1]))
    ch = _chain(rows)
    assert len(ch) >= 4 and len(ch[-1][2]) == 0
    return F1, ch


def _check_chain(got, ch, L):
    assert len(got) == L
    for lv, (_, cnt, cand) in zip(got, ch):
        _check_level(lv, cnt, cand)


def test_chain_references():
    for name in ("lat13_F70", "lat13_F4097", "lat7_F32768", "cliques_s3"):
        _chain_case(name)
    assert math.comb(13, 5) / math.comb(13, 4) == 1.8


CHAIN_FREE = [("lat13_F70", ml) for ml in (1, 2, 5, 6, 9, 10, 12)] + \
             [("lat13_F4097", 6), ("lat13_F4097", 12), ("lat7_F32768", 12), ("cliques_s3", 12)]


@pytest.mark.gpu
@pytest.mark.parametrize("case,max_levels", CHAIN_FREE)
def test_chain_first_free(case, max_levels):
    # levels 1 .. max_levels - 1 run on the device in batches of 4: 5 and 9 end on a batch's
    # last level, 6 and 10 on the next one's first; 12 lets the lattice's chain end by
    # itself inside a batch (no candidates from the one 13-itemset)
    F1, ch = _chain_case(case)
    natural = len(ch) - 1
    assert natural == {"lat13": 11, "lat7_": 5}.get(case[:5], natural) and natural < 12
    growth = 3.0 if case.startswith("lat") else 1e9
    for (_, _, a), (_, _, b) in zip(ch, ch[1:-1]):
        assert len(b) <= growth * len(a)
    got = prim.apriori_gen_chain(ch[0][0], F1, DEV, max_levels, growth, 0, 0, first_free=True)
    _check_chain(got, ch, min(max_levels, natural))


@pytest.mark.gpu
@pytest.mark.parametrize("less,levels", [(0, 3), (1, 2)])
def test_chain_tmax(less, levels):
    # the caller's bundle limit: the first three levels' total is accepted, one less is not
    F1, ch = _chain_case("lat13_F70")
    tmax = sum(len(c) for _, _, c in ch[:3]) - less
    assert tmax + less == 286 + 715 + 1287
    got = prim.apriori_gen_chain(ch[0][0], F1, DEV, 6, 4.0, 0, tmax)
    _check_chain(got, ch, levels)


@pytest.mark.gpu
@pytest.mark.parametrize("half,levels", [(0.5, 2), (-0.5, 0)])
def test_chain_growth(half, levels):
    # from the lattice's 4-subsets: C(13, 5) = 1.8 C(13, 4) candidates against a growth just
    # above and just below 1.8; the level after it grows less
    F1, ch = _chain_case("lat13_F70")
    rows, _, cand = ch[2]
    assert rows.shape == (715, 4) and len(cand) == 1287 and len(ch[3][2]) == 1716
    got = prim.apriori_gen_chain(rows, F1, DEV, 2, (1287 + half) / 715, 0, 1 << 40)
    _check_chain(got, ch[2:], levels)


# ---------------------------------------------------------------------------
# 3. the device bundle's speculative levels: fa_hip_dl_level0 + fa_hip_dl_more.  Level 1 is
#    built by k_agd_insert / k_agd_ext, every later level from the hash table and Ext bitsets
#    that the level before it wrote in its emit pass (k_dl_rows), in batches of 4 with
#    k_dl_decide's acceptance on the device.
# ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def bundle_case(name, depth=64):
    """-> (F1, chain).  The parent rows of a device bundle and the brute force iterated, `depth`
    levels at the most (the large lattices' chains are cut where their bundles end)."""
    rng = np.random.default_rng(sum(map(ord, name)))
    if name.startswith("lat"):                       # lat{N}_F{F1}[_m{m0}][_del{d}]
        parts = name.split("_")
        N, F1 = int(parts[0][3:]), int(parts[1][1:])
        m0 = next((int(p[1:]) for p in parts if p[0] == "m"), 2)
        d = next((int(p[3:]) for p in parts if p.startswith("del")), 0)
        drop = tuple(rng.choice(math.comb(N, m0), d, replace=False).tolist())
        rows, want = _lattice(_placed(F1, N), m0, drop)
        ch = _chain(rows, depth)
        assert np.array_equal(ch[0][2], _arr(want, m0 + 1)) and len(ch[0][0]) == math.comb(N, m0) - d
        if not d:
            assert [len(c) for _, _, c in ch] == ([math.comb(N, k) for k in range(m0 + 1, N + 1)] + [0])[:depth]
    elif name == "k13_triangles":
        # 13 ranks' pairs and 200 triangles apart from them: 286 + 200, 715, 1287 candidates, so
        # the second speculative level grows more (1.8) than the first (1.47)
        F1 = 13 + 600
        rows = list(itertools.combinations(range(13), 2))
        for t in range(200):
            a = 13 + 3 * t
            rows += [(a, a + 1), (a, a + 2), (a + 1, a + 2)]
        ch = _chain(rows)
        assert [len(c) for _, _, c in ch[:3]] == [486, 715, 1287]
    elif name == "two_rows":
        F1, ch = 70, _chain([(3, 63), (3, 64)])
        assert [len(c) for _, _, c in ch] == [0]
    elif name == "classes_of_one":
        F1, ch = 130, _chain([(2 * q, 2 * q + 1 + (q % 3)) for q in range(40)])
        assert [len(c) for _, _, c in ch] == [0]
    else:
        rows, F1 = _cliques(int(name[-1]))
        ch = _chain(rows)
    return F1, ch


def accepted(ch, max_levels, growth):
    """(levels a bundle accepts, the chain ended on a level without candidates): level 0
    always, level l while it has candidates and at most growth x the level before."""
    L = 1
    while L < max_levels:
        C = len(ch[L][2]) if L < len(ch) else 0
        if C == 0:
            return L, True
        if C > growth * len(ch[L - 1][2]):
            return L, False
        L += 1
    return L, False


@pytest.fixture(scope="module")
def dl_state():
    return prim.DeviceLevelState(DEV)


def ws_array(S, ptr, count, dtype):
    """count values of dtype at the device address ptr inside S.ws."""
    o, nb = int(ptr) - S.ws.data_ptr(), count * np.dtype(dtype).itemsize
    assert 0 <= o and o + nb <= S.ws.numel()
    return S.ws[o:o + nb].cpu().numpy().view(dtype)


def run_bundle(S, F1, ch, max_levels, growth, c_bound=None):
    """dl_bundle_gen on the chain's first rows -> (control block, the parent rows' tensor: the
    level table points at it).  c_bound defaults to C_0, the smallest that takes level 0;
    the later levels' bounds follow from it by the growth."""
    rows, _, cand = ch[0]
    n, m0 = rows.shape
    P0 = torch.from_numpy(rows).to(DEV)
    cb = max(len(cand), 1) if c_bound is None else c_bound
    c = prim.dl_bundle_gen(S, P0.data_ptr(), None, n, n, m0, F1, cb, prim.dl_lds_budget(F1), growth, max_levels,
                           torch.cuda.current_stream(DEV).cuda_stream, post=False)
    assert not c[prim.dl().kDlOverBound]
    return c, P0


def check_bundle(S, c, F1, ch, L, empty=False):
    """The control block and every accepted level's buffers against the brute force."""
    K = prim.dl()
    assert c[K.kDlLevels] == L and bool(c[K.kDlEmpty]) == empty
    assert not c[K.kDlMulti] and not c[K.kDlEnd]
    base = 0
    for l in range(L):
        rows, cnt, cand = ch[l]
        n, m = rows.shape
        C, d = len(cand), S.desc[l]
        assert (c[K.kDlNl + l], c[K.kDlCl + l], c[K.kDlGl + l]) == (n, C, int((cnt > 0).sum())), l
        assert (d["m"], d["n"], d["C"], d["base"]) == (m, n, C, base), l
        if l:
            assert d["P"] == S.desc[l - 1]["rows"]
        assert np.array_equal(ws_array(S, d["cnt"], n, np.int32), cnt), l
        assert np.array_equal(ws_array(S, d["off"], n + 1, np.int64), np.concatenate([[0], np.cumsum(cnt)])), l
        assert np.array_equal(ws_array(S, d["cnt"] + 4 * n, C, np.int32), cand[:, -1]), l
        assert np.array_equal(ws_array(S, d["rows"], C * (m + 1), np.int32).reshape(C, m + 1), cand), l
        base += C
    used = np.unique(ch[0][2])
    bits = np.unpackbits(c[K.kDlBits:K.kDlBits + K.kDlBitsW].view(np.uint8), bitorder="little")
    assert c[K.kDlNUsed] == used.size and np.array_equal(np.flatnonzero(bits), used)


def bundle_expect(case, max_levels, growth):
    """-> (accepted levels, ended empty) of a BUNDLES case, with the checks that the case is
    what it is listed for (they need the reference only)."""
    F1, ch = bundle_case(case)
    L, empty = accepted(ch, max_levels, growth)
    m0 = ch[0][0].shape[1]
    if case == "lat13_F70":
        assert (L, empty) == (min(max_levels, 11), max_levels == 31)
    elif case.startswith("lat7"):
        assert (L, empty) == (5, False)
    elif "_m" in case:
        assert L == max_levels and [r.shape[1] for r, _, _ in ch[:L]] == list(range(m0, m0 + L))
        assert case != "lat42_F70_m39" or max_levels == prim.dl().kDlMaxM - 39 + 1
    else:
        # the chain ends by itself, at a depth past the first batch, never by the growth
        natural = len(ch) - 1
        assert L == min(max_levels, natural) and empty == (max_levels > natural) and 6 <= natural < 31
    return L, empty


def test_bundle_references(native):
    for name in BUNDLE_NAMES:
        bundle_case(name)
    for case, max_levels, growth in BUNDLES:
        bundle_expect(case, max_levels, growth)
    for case, growth, L in GROWTH_STOPS:
        assert accepted(bundle_case(case)[1], 4, growth) == (L, False)
    assert prim.dl().kDlMaxM == 40 and prim.dl().kDlMaxLevels == 31 and prim.dl().kDlInline == 12


BUNDLES = [(name, ml, 3.0) for name in ("lat13_F70", "lat13_F70_del3") for ml in (2, 3, 5, 6, 9, 10, 31)] + \
          [("cliques_s3", ml, 8.0) for ml in (2, 3, 5, 6, 9, 10, 31)] + \
          [(f"lat7_F{F1}", 5, 3.0) for F1 in (4096, 4097, 8193, 16385, 32768)] + \
          [("lat15_F70_m11", 4, 3.0), ("lat42_F70_m39", 2, 3.0)]
GROWTH_STOPS = [("lat13_F70", 2.4, 1), ("k13_triangles", 1.6, 2), ("k13_triangles", 1.9, 4)]
BUNDLE_NAMES = sorted({b[0] for b in BUNDLES} | {"k13_triangles", "two_rows", "classes_of_one"})


@pytest.mark.gpu
@pytest.mark.parametrize("case,max_levels,growth", BUNDLES)
def test_bundle_levels(dl_state, case, max_levels, growth):
    # lat7 at the wide F1: k_dl_rows' next_ext store under every lane width, nw a multiple
    # of it (4096) and not; lat15 m11 / lat42 m39: parents of 11 .. 14 and of 39, 40 items,
    # the bundles tests/test_dl_plan_edges.py counts
    F1, ch = bundle_case(case)
    L, empty = bundle_expect(case, max_levels, growth)
    c, P0 = run_bundle(dl_state, F1, ch, max_levels, growth)
    check_bundle(dl_state, c, F1, ch, L, empty)
    assert bool(c[prim.dl().kDlStop]) == (L < max_levels)
    del P0


@pytest.mark.gpu
@pytest.mark.parametrize("case,growth,L", GROWTH_STOPS)
def test_bundle_growth_stop(dl_state, case, growth, L):
    # 715 > 2.4 * 286 rejects the first speculative level; with the triangles the first one
    # passes (715 <= 1.6 * 486) and the second is rejected (1287 > 1.6 * 715)
    F1, ch = bundle_case(case)
    c, P0 = run_bundle(dl_state, F1, ch, 4, growth)
    check_bundle(dl_state, c, F1, ch, L)
    assert bool(c[prim.dl().kDlStop]) == (L < 4)
    del P0


@pytest.mark.gpu
def test_bundle_c_bound(dl_state):
    # level 0's output buffer holds c_bound candidates: C_0 itself is taken, C_0 - 1 makes
    # the level "multi" (no rows, the host counts it window by window)
    K, (F1, ch) = prim.dl(), bundle_case("lat13_F70")
    C0 = len(ch[0][2])
    c, P0 = run_bundle(dl_state, F1, ch, 3, 3.0, c_bound=C0)
    check_bundle(dl_state, c, F1, ch, 3)
    c, P0 = run_bundle(dl_state, F1, ch, 3, 3.0, c_bound=C0 - 1)
    assert c[K.kDlMulti] and c[K.kDlStop] and not c[K.kDlEnd] and not c[K.kDlEmpty]
    assert (c[K.kDlLevels], c[K.kDlNl], c[K.kDlCl]) == (0, len(ch[0][0]), C0)
    del P0


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["two_rows", "classes_of_one"])
def test_bundle_end(dl_state, case):
    # fewer parent rows than m0 + 1 (the reference's loop test), and a level 0 without candidates
    K, (F1, ch) = prim.dl(), bundle_case(case)
    n, m0 = ch[0][0].shape
    assert (n < m0 + 1) == (case == "two_rows")
    c, P0 = run_bundle(dl_state, F1, ch, 4, 3.0)
    assert c[K.kDlEnd] and c[K.kDlStop] and not c[K.kDlMulti] and not c[K.kDlEmpty]
    assert (c[K.kDlLevels], c[K.kDlNl], c[K.kDlCl]) == (0, n, 0)
    del P0
