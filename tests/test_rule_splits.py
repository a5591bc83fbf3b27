"""The rule export with multi-item consequents (--rules-max-consequent, AssociationRules.all_rules
with max_consequent) on the CPU path: the shared enumeration header through its exports, the
hand example, max_consequent = 1 against today's export, the oracle's brute force from Python
ints (bit for bit), counts near 2^31, occurrence against line counts, the limits and errors,
the command line and two gloo ranks.  tests/test_gpu_rule_splits.py runs the same cases on the
device."""
import ctypes as C
import functools
import itertools
import math
import os

import numpy as np
import pytest

from fastapriori_amd.models import oracle
from fastapriori_amd.models.data import MiningResult
from fastapriori_amd.models.rules import AssociationRules
from fastapriori_amd.ops import _native, host
from fastapriori_amd.parallel.launch import spawn_local
from fastapriori_amd.utils import io
from fastapriori_amd.utils.metrics import Logger

from test_condense import D, U, _mine, quest300
from test_rule_measures import (BIG_N, HAND_BYTES, REPEATED, SORTS, THRESHOLDS, _cli, all_rules, as_oracle,
                                large_counts, little_to_do, missing_subset, small_lattice)

MFIELDS = ("ante_off", "ante", "cons_off", "cons", "cnt_s", "cnt_a", "cnt_c", "support", "conf", "lift", "leverage",
           "conviction")
MDTYPES = dict(ante_off=np.int64, ante=np.int32, cons_off=np.int64, cons=np.int32, cnt_s=np.int64, cnt_a=np.int64,
               cnt_c=np.int64, support=np.float64, conf=np.float64, lift=np.float64, leverage=np.float64,
               conviction=np.float64)


# ---------------------------------------------------------------------------
# helpers (shared with the device tests)
# ---------------------------------------------------------------------------
def tie_pos(res) -> np.ndarray:
    return AssociationRules(res, logger=Logger(enabled=False), device="cpu")._tie_pos()


def splits(res, **kw) -> host.MultiRuleMeasures:
    """ops.host.rule_splits: the new C++ path, max_consequent = 1 included."""
    return host.rule_splits(res.levels, res.counts, res.n_lines, tie_pos(res), **kw)


def mtable(rows) -> host.MultiRuleMeasures:
    """The oracle's (A, B, cS, cA, cB, five measures) tuples as a MultiRuleMeasures."""
    def csr(sets):
        off = np.zeros(len(sets) + 1, dtype=np.int64)
        if sets:
            off[1:] = np.cumsum([len(a) for a in sets])
        return off, np.array([x for a in sets for x in a], dtype=np.int32)
    cols = [np.array([r[j] for r in rows], dtype=t) for j, t in
            ((2, np.int64), (3, np.int64), (4, np.int64), (5, np.float64), (6, np.float64), (7, np.float64),
             (8, np.float64), (9, np.float64))]
    return host.MultiRuleMeasures(*csr([sorted(r[0]) for r in rows]), *csr([sorted(r[1]) for r in rows]), *cols)


def as_multi(rm: host.RuleMeasures) -> host.MultiRuleMeasures:
    """Today's export with every consequent as a one-element list."""
    return host.MultiRuleMeasures(rm.ante_off, rm.ante, np.arange(rm.n_rules + 1, dtype=np.int64), rm.cons, rm.cnt_s,
                                  rm.cnt_a, rm.cnt_c, rm.support, rm.conf, rm.lift, rm.leverage, rm.conviction)


def take(rm: host.MultiRuleMeasures, keep: np.ndarray) -> host.MultiRuleMeasures:
    """The rules at the (ascending) indices ``keep``, in order."""
    def csr(off, flat):
        ln = (off[1:] - off[:-1])[keep]
        new = np.zeros(keep.size + 1, dtype=np.int64)
        np.cumsum(ln, out=new[1:])
        return new, flat[np.repeat(off[:-1][keep] - new[:-1], ln) + np.arange(new[-1])]
    return host.MultiRuleMeasures(*csr(rm.ante_off, rm.ante), *csr(rm.cons_off, rm.cons),
                                  *[getattr(rm, f)[keep] for f in MFIELDS[4:]])


def msame(got: host.MultiRuleMeasures, want: host.MultiRuleMeasures) -> None:
    """Equal arrays, the doubles bit for bit (exact int64 products and one division per measure)."""
    assert isinstance(got, host.MultiRuleMeasures) and got.n_rules == want.n_rules
    for f in MFIELDS:
        g, w = getattr(got, f), getattr(want, f)
        assert g.dtype == MDTYPES[f] and g.shape == w.shape, f
        if g.dtype == np.float64:
            g, w = np.ascontiguousarray(g).view(np.int64), np.ascontiguousarray(w).view(np.int64)
        assert np.array_equal(g, w), f


def n_k(k: int, M: int) -> int:
    return sum(math.comb(k, b) for b in range(1, min(M, k - 1) + 1))


def elements(res, M: int) -> int:
    return sum(len(l) * n_k(k, M) for k, l in enumerate(res.levels, 1) if k >= 2)


def clique_elements(n: int) -> int:
    """(itemset, split) elements of a complete n-clique at all splits."""
    return 3 ** n - 2 ** (n + 1) + 1


def cliques(groups, w=None) -> MiningResult:
    """Disjoint complete lattices, small_lattice's counts: count(S) = 2^31 - 1 - sum of w_i."""
    n = 1 + max(max(g) for g in groups)
    w = w or {i: (0 if i in (2, 7) else 2 ** 29 if i == 5 else 3 * i + 1) for i in range(n)}
    levels, counts = [], []
    for k in range(1, max(map(len, groups)) + 1):
        rows = sorted(c for g in groups for c in itertools.combinations(g, k))
        levels.append(np.array(rows, dtype=np.int32).reshape(-1, k))
        counts.append(np.array([BIG_N - sum(w[i] for i in r) for r in rows], dtype=np.int64))
    return MiningResult([str(i) for i in range(n)], levels, counts, 1, BIG_N)


def edge_lattice(one_more_pair: bool = False) -> MiningResult:
    """One 8-clique, one 4-clique, three 3-cliques and four pairs: 6050 + 50 + 36 + 8 = 6144 =
    24 x 256 elements at all splits; one more pair: 6146, two live threads in a 25th workgroup."""
    groups = [tuple(range(8)), (8, 9, 10, 11), (12, 13, 14), (15, 16, 17), (18, 19, 20), (21, 22), (23, 24),
              (25, 26), (27, 28)] + ([(29, 30)] if one_more_pair else [])
    res = cliques(groups)
    assert (clique_elements(8), clique_elements(4), clique_elements(3), clique_elements(2)) == (6050, 50, 12, 2)
    assert elements(res, 7) == (6146 if one_more_pair else 6144) and 6144 == 24 * 256
    return res


CUBE_ITEMS = 12
CUBE_SPLIT_CONF = 0.5


@functools.lru_cache(maxsize=None)
def cube_splits():
    """test_rule_measures.cube's construction on 12 items at all splits: 3^12 - 2^13 + 1 = 523250
    elements in 2044 workgroups of 256, past one 1024-total scan chunk.  Returns (result, every
    element's confidence in enumeration order), the latter from numpy on counts by bitmask."""
    n = CUBE_ITEMS
    w = np.array([100 + 10 * i for i in range(n)], dtype=np.int64)
    n0 = int(w.sum()) + 30
    by_mask = n0 - ((np.arange(1 << n)[:, None] >> np.arange(n)) & 1) @ w
    levels, counts, conf = [], [], []
    for k in range(1, n + 1):
        rows = np.array(list(itertools.combinations(range(n), k)), dtype=np.int32).reshape(-1, k)
        bits = 1 << rows.astype(np.int64)
        mask = bits.sum(1)
        levels.append(rows)
        counts.append(by_mask[mask])
        if k >= 2:
            pick = np.array([[p in c for p in range(k)] for b in range(1, k)
                             for c in itertools.combinations(range(k), b)], dtype=np.int64)   # [n_k, k], enumeration order
            b_mask = bits @ pick.T                                         # [rows, n_k]
            conf.append((by_mask[mask][:, None].astype(np.float64) / by_mask[mask[:, None] ^ b_mask]).reshape(-1))
    conf = np.concatenate(conf)
    assert conf.size == clique_elements(n) == 523250 and -(-conf.size // 256) == 2044 > 1024
    return MiningResult([str(i) for i in range(n)], levels, counts, 1, n0), conf


def cube_per_workgroup() -> np.ndarray:
    sel = cube_splits()[1] >= CUBE_SPLIT_CONF
    return np.add.reduceat(sel.astype(np.int64), np.arange(0, sel.size, 256))


def check_cube_threshold() -> np.ndarray:
    """The threshold is chosen on the CPU: within a 12-itemset the splits are ordered by |B|
    and the confidence falls with the consequent's weight, so whole workgroups go either way."""
    per_wg = cube_per_workgroup()
    last = cube_splits()[1].size - 256 * (per_wg.size - 1)
    full = np.full(per_wg.size, 256)
    full[-1] = last
    assert per_wg.size == 2044 and (per_wg == 0).sum() >= 1 and (per_wg[:-1] == 256).sum() >= 1
    assert ((per_wg > 0) & (per_wg < full)).sum() >= per_wg.size // 4
    return per_wg


# ---------------------------------------------------------------------------
# 1. the shared header (csrc/host/fa_rule_splits.h) through libfa_host.so
# ---------------------------------------------------------------------------
def unrank(k: int, M: int, j: int):
    b, mask = C.c_int32(-1), C.c_uint32(0)
    rc = _native.host().fa_rule_split_unrank(k, M, j, C.addressof(b), C.addressof(mask))
    return rc, b.value, mask.value


def decode(local: int, nk: int):
    s, j = C.c_int64(-1), C.c_uint64(0)
    assert _native.host().fa_rule_split_decode(local, nk, C.addressof(s), C.addressof(j)) == 0
    return s.value, j.value


def test_unrank_is_a_bijection_in_the_stated_order():
    lib = _native.host()
    for k in range(2, 13):
        for M in list(range(1, k)) + [k, 40]:
            want = [(b, sum(1 << p for p in c)) for b in range(1, min(M, k - 1) + 1)
                    for c in itertools.combinations(range(k), b)]
            assert lib.fa_rule_split_count(k, M) == len(want) == n_k(k, M)
            got = [unrank(k, M, j) for j in range(len(want))]
            assert [g[0] for g in got] == [0] * len(want)
            assert [g[1:] for g in got] == want                            # b ascending, subsets lexicographic
            assert len({m for _, m in want}) == len(want) and all(0 < m < (1 << k) - 1 or k == 2 for _, m in want)
            assert unrank(k, M, len(want))[0] == 1                         # past the last split
    assert lib.fa_rule_split_count(1, 1) == 0 and lib.fa_rule_split_count(33, 1) == 0
    assert lib.fa_rule_split_count(5, 0) == 0


def test_unrank_at_the_level_limit():
    lib = _native.host()
    assert lib.fa_rule_split_count(32, 31) == 2 ** 32 - 2
    for M in (1, 2, 16, 31):
        nk = lib.fa_rule_split_count(32, M)
        assert nk == n_k(32, M)
        assert unrank(32, M, 0) == (0, 1, 1)
        assert unrank(32, M, nk - 1) == (0, M, ((1 << M) - 1) << (32 - M))       # the last M positions
    assert unrank(32, 16, n_k(32, 15)) == (0, 16, (1 << 16) - 1)                 # the first 16-subset


def test_decode_around_two_to_the_32():
    for nk in (2, 3, 6050, 2 ** 32 - 2):
        for local in (0, nk - 1, nk, 2 ** 32 - 2, 2 ** 32 - 1, 2 ** 32, 2 ** 32 + 1, 2 ** 40 + 12345, 2 ** 62 + 1):
            assert decode(local, nk) == divmod(local, nk), (local, nk)


# ---------------------------------------------------------------------------
# 2. the hand example
# ---------------------------------------------------------------------------
# D at M = 2: today's nine rules, then the triple split as one item -> two items.
# rule (cS, cA, cB, confidence, lift, leverage, conviction)
HAND_SPLITS = [(("3",), ("1", "2"), 2, 3, 3, 0.5, 2 / 3, 8 / 9, -0.0625, 0.75),
               (("2",), ("1", "3"), 2, 3, 2, 0.5, 2 / 3, 4 / 3, 0.125, 1.5),
               (("1",), ("2", "3"), 2, 3, 2, 0.5, 2 / 3, 4 / 3, 0.125, 1.5)]
HAND_MULTI_BYTES = HAND_BYTES + (b"3\t2 1\t2\t3\t3\t0.5\t0.6666666666666666\t0.8888888888888888\t-0.0625\t0.75\n"
                                 b"2\t3 1\t2\t3\t2\t0.5\t0.6666666666666666\t1.3333333333333333\t0.125\t1.5\n"
                                 b"1\t3 2\t2\t3\t2\t0.5\t0.6666666666666666\t1.3333333333333333\t0.125\t1.5\n")


def check_hand_splits(rm: host.MultiRuleMeasures, res) -> None:
    assert res.items == ["1", "2", "3"] and rm.n_rules == 12
    rows = [(tuple(res.items[r] for r in rm.antecedent(i)), tuple(res.items[r] for r in rm.consequent(i)),
             int(rm.cnt_s[i]), int(rm.cnt_a[i]), int(rm.cnt_c[i]), float(rm.support[i]), float(rm.conf[i]),
             float(rm.lift[i]), float(rm.leverage[i]), float(rm.conviction[i])) for i in range(rm.n_rules)]
    assert rows[9:] == HAND_SPLITS                                         # float ==: the exact doubles
    msame(take(rm, np.arange(9)), as_multi(all_rules(res)))
    msame(rm, mtable(oracle.all_rules_multi(as_oracle(res), 2)))


def test_hand_example(tmp_path):
    res = _mine(D, 0.5)
    rm = all_rules(res, max_consequent=2)
    check_hand_splits(rm, res)
    msame(all_rules(res, max_consequent=7), rm)                            # above K - 1: every split
    assert open(io.write_rules(rm, res.items, str(tmp_path / "rules")), "rb").read() == HAND_MULTI_BYTES
    one = splits(res, max_consequent=1)                                    # the new path and the new writer at M = 1
    assert open(io.write_rules(one, res.items, str(tmp_path / "one")), "rb").read() == HAND_BYTES
    assert isinstance(all_rules(res, max_consequent=1), host.RuleMeasures)
    assert len(host.RuleMeasures.__dataclass_fields__) == 11
    with pytest.raises(io.OutputExistsError):
        io.write_rules(rm, res.items, str(tmp_path / "rules"))


# ---------------------------------------------------------------------------
# 3. max_consequent = 1 against today's export
# ---------------------------------------------------------------------------
def test_one_item_consequents_equal_todays_export():
    res = quest300()[0]
    assert len(res.levels) == 10
    for sort in SORTS:
        for th in THRESHOLDS:
            msame(splits(res, max_consequent=1, sort=sort, **th), as_multi(all_rules(res, sort=sort, **th)))


# ---------------------------------------------------------------------------
# 4. C++ against the oracle's brute force on the mined case
# ---------------------------------------------------------------------------
SPLIT_THRESHOLDS = [dict(min_confidence=0.0), dict(min_confidence=0.5), dict(min_confidence=1.0),
                    dict(min_confidence=0.0, min_lift=1.0)]


@functools.lru_cache(maxsize=None)
def quest_rows(M: int):
    return oracle.rule_split_rows(as_oracle(quest300()[0]), M)


@functools.lru_cache(maxsize=None)
def quest_table(M: int, sort: str) -> host.MultiRuleMeasures:
    """The brute force runs once per M and is ordered once per sort measure; a thresholded
    table is that table filtered on the oracle's own doubles (a filter keeps the order), which
    test_thresholded_oracle_is_the_filtered_one checks."""
    return mtable(oracle.all_rules_multi(as_oracle(quest300()[0]), M, sort=sort, rows=quest_rows(M)))


def quest_want(M: int, sort: str, min_confidence: float = 0.0, min_lift=None) -> host.MultiRuleMeasures:
    full = quest_table(M, sort)
    keep = full.conf >= min_confidence
    if min_lift is not None:
        keep &= full.lift >= min_lift
    return full if keep.all() else take(full, np.flatnonzero(keep))


def test_thresholded_oracle_is_the_filtered_one():
    res = quest300()[0]
    msame(quest_want(2, "leverage", 0.5, 1.0),
          mtable(oracle.all_rules_multi(as_oracle(res), 2, 0.5, 1.0, "leverage", rows=quest_rows(2))))
    assert oracle.all_rules_multi(as_oracle(_mine(D, 0.5)), 1) == \
        [(a, frozenset([c]), *r) for a, c, *r in oracle.all_rules(as_oracle(_mine(D, 0.5)))]


@pytest.mark.parametrize("M", [2, 3, 9])
def test_cpp_equals_the_oracle_on_the_mined_case(M):
    res = quest300()[0]
    assert M <= len(res.levels) - 1 == 9
    sizes = set()
    for sort in SORTS:
        for th in SPLIT_THRESHOLDS:
            got = all_rules(res, max_consequent=M, sort=sort, **th)
            msame(got, quest_want(M, sort, **th))
            # the one-item-consequent rules, in order, are today's export
            one = np.flatnonzero(got.cons_off[1:] - got.cons_off[:-1] == 1)
            msame(take(got, one), as_multi(all_rules(res, sort=sort, **th)))
            sizes.add(got.n_rules)
    assert elements(res, M) in sizes and len(sizes) >= 4
    if M == 9:
        msame(all_rules(res, max_consequent=29), quest_want(9, "confidence"))      # above K - 1: every split


def test_limits_keep_a_prefix():
    res = quest300()[0]
    full = quest_want(2, "lift", 0.5)
    R = full.n_rules
    for limit in (0, 1, R - 1, R, R + 1):
        got = all_rules(res, max_consequent=2, min_confidence=0.5, sort="lift", limit=limit)
        msame(got, take(full, np.arange(min(limit, R))))
    assert all_rules(res, max_consequent=2, limit=0).cons_off.tolist() == [0]


# ---------------------------------------------------------------------------
# 5. / 6. large counts, occurrence counts against line counts
# ---------------------------------------------------------------------------
def check_big_counts(run) -> None:
    res = small_lattice()                                                  # N = 2^31 - 1, products near 2^61
    assert elements(res, 10) == clique_elements(11) + clique_elements(3) + clique_elements(2)
    rows = oracle.rule_split_rows(as_oracle(res), 10)
    for sort in ("leverage", "conviction"):
        msame(run(res, max_consequent=10, sort=sort),
              mtable(oracle.all_rules_multi(as_oracle(res), 10, sort=sort, rows=rows)))
    assert max(r[2] * BIG_N for r in rows) > 2 ** 61


def test_big_counts():
    check_big_counts(lambda res, **kw: all_rules(res, **kw))


REPEATED3 = REPEATED[0].replace("\n", " 3\n")      # "1 1 1 2 3 / 1 2 3": item 1 occurs 4 times on 2 lines


def check_repeated_token(run) -> None:
    for text in REPEATED:                                                  # two items: nothing but today's rules
        res = _mine(text, 0.5)
        msame(run(res, max_consequent=2), as_multi(all_rules(res)))
    res = _mine(REPEATED3, 0.5)
    assert res.n_lines == 2 and res.items[0] == "1" and res.counts[0].tolist() == [4, 2, 2]
    rm = run(res, max_consequent=2, sort="leverage")
    msame(rm, mtable(oracle.all_rules_multi(as_oracle(res), 2, sort="leverage")))
    by = {(tuple(rm.antecedent(i).tolist()), tuple(rm.consequent(i).tolist())): int(rm.cnt_c[i])
          for i in range(rm.n_rules)}
    assert by[((1, 2), (0,))] == 4                                         # {2,3} -> 1: the occurrence count
    assert by[((2,), (0, 1))] == 2 and by[((1,), (0, 2))] == 2             # 3 -> {1,2}: a line count


def test_repeated_token_on_a_line():
    check_repeated_token(lambda res, **kw: all_rules(res, **kw))


# ---------------------------------------------------------------------------
# 7. errors and shapes with little to do
# ---------------------------------------------------------------------------
def no_pair_2_3() -> MiningResult:
    """Items 0..3, all four triples and the quadruple, every pair except {2, 3}."""
    levels = [np.array(list(itertools.combinations(range(4), k)), dtype=np.int32).reshape(-1, k) for k in (1, 2, 3, 4)]
    levels[1] = levels[1][:-1]
    assert levels[1].tolist()[-1] == [1, 3]
    counts = [np.full(len(l), 9 - 2 * k, np.int64) for k, l in enumerate(levels)]
    return MiningResult(list("abcd"), levels, counts, 1, 10)


def missing_level(M: int) -> int:
    """The largest level of missing_subset() with a split that needs the removed triple."""
    res, full = missing_subset(), quest300()[0]
    gone = set(map(tuple, full.levels[2].tolist())) - set(map(tuple, res.levels[2].tolist()))
    (t,) = gone
    ks = [k for k, l in enumerate(res.levels, 1) if k >= 4 and (k - 3 <= M or 3 <= M)
          and any(set(t) <= set(r) for r in l.tolist())]
    return max(ks)


def check_errors(run) -> None:
    with pytest.raises(RuntimeError, match="size 4 has a subset"):
        run(missing_subset(), max_consequent=1)
    k = missing_level(2)
    assert k in (4, 5)
    with pytest.raises(RuntimeError, match=f"size {k} has a subset"):
        run(missing_subset(), max_consequent=2)
    with pytest.raises(RuntimeError, match="size 4 has a subset"):
        run(no_pair_2_3(), max_consequent=2)                               # {0,1,2,3} split as {2,3} -> {0,1}
    with pytest.raises(RuntimeError, match="size 3 has a subset"):
        run(no_pair_2_3(), max_consequent=1)                               # {0,2,3} as {2,3} -> 0


def test_errors():
    check_errors(splits)
    with pytest.raises(RuntimeError, match="size 4 has a subset"):
        all_rules(no_pair_2_3(), max_consequent=2)
    res = _mine(D, 0.5)
    for M in (0, -3):
        with pytest.raises(ValueError, match="max_consequent"):
            all_rules(res, max_consequent=M)
        with pytest.raises(ValueError, match="max_consequent"):
            splits(res, max_consequent=M)
    deep = MiningResult([str(i) for i in range(33)], [np.arange(k, dtype=np.int32).reshape(1, k) for k in range(1, 34)],
                        [np.ones(1, np.int64)] * 33, 1, 1)
    with pytest.raises(ValueError, match="limit of 32"):
        all_rules(deep, max_consequent=2)
    with pytest.raises(ValueError, match="limit of 32"):
        splits(deep, max_consequent=1)
    with pytest.raises(ValueError, match="line total is unknown"):
        all_rules(MiningResult(res.items, res.levels, res.counts, res.min_count, 0), max_consequent=2)


def test_element_total_over_the_grid_limit(monkeypatch):
    monkeypatch.setattr(_native, "host", lambda: pytest.fail("a native call"))
    args = (None, None, 1, 0.0, None, "confidence", None)
    cap = (2 ** 31 - 2) * 256                                              # the most elements one grid holds
    for sizes in ([3, cap // 2], [3, 3, cap // 6 - 1]):                    # 2 and 6 + 6 splits per itemset
        assert int(host.rule_splits_plan(*args, 2, sizes=sizes)["eoff"][-1]) == cap
    with pytest.raises(ValueError,
                       match=rf"{cap + 2} \(itemset, split\) elements.*smaller --rules-max-consequent.*--max-level"):
        host.rule_splits_plan(*args, 1, sizes=[3, cap // 2 + 1])
    big = [10 ** 6] * 32
    with pytest.raises(ValueError, match="--max-level"):
        host.rule_splits_plan(*args, 31, sizes=big)
    assert host.rule_splits_plan(*args, 31, sizes=[10] * 20)["M"] == 19
    with pytest.raises(ValueError, match="limit of 32"):
        host.rule_splits_plan(*args, 2, sizes=[1] * 33)


def test_two_levels_and_shapes_with_little_to_do():
    res = large_counts()
    msame(all_rules(res, max_consequent=5), as_multi(all_rules(res)))
    for name, (res, n) in little_to_do().items():
        rm = all_rules(res, max_consequent=2)
        msame(rm, as_multi(all_rules(res)))
        assert rm.n_rules == n and rm.cons_off.size == n + 1, name
        if n == 0:
            assert rm.cons_off.tolist() == [0] and rm.ante_off.tolist() == [0] and rm.cons.size == 0


# ---------------------------------------------------------------------------
# 8. command line
# ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def cli_runs(tmp_path_factory):
    d = tmp_path_factory.mktemp("splits")
    (d / "D.dat").write_text(D)
    (d / "U.dat").write_text(U)
    runs = {"plain": _cli(d, "a_", "--rules"), "multi": _cli(d, "b_", "--rules", "--rules-max-consequent", "2")}
    os.rename(d / "b_rules", d / "b_rules_first")
    runs["rules_only"] = _cli(d, "b_", "--rules-only", "--overwrite", "--rules", "--rules-max-consequent", "2")
    runs["bad"] = _cli(d, "c_", "--rules-max-consequent", "2")
    runs["zero"] = _cli(d, "c_", "--rules", "--rules-max-consequent", "0")
    return d, runs


def test_cli_writes_the_hand_file(cli_runs):
    d, runs = cli_runs
    assert all(runs[k].returncode == 0 for k in ("plain", "multi", "rules_only")), [r.stderr for r in runs.values()]
    assert (d / "b_rules_first" / "part-00000").read_bytes() == HAND_MULTI_BYTES
    assert (d / "b_rules" / "part-00000").read_bytes() == HAND_MULTI_BYTES          # --rules-only from the checkpoint
    assert "==== Total time for get rules " in runs["multi"].stdout


def test_cli_without_the_flag_nothing_changes(cli_runs):
    d, runs = cli_runs
    assert (d / "a_rules" / "part-00000").read_bytes() == HAND_BYTES
    for name in ("freqItemset", "recommends"):
        assert (d / f"a_{name}" / "part-00000").read_bytes() == (d / f"b_{name}" / "part-00000").read_bytes()
    assert runs["bad"].returncode == 2 and "--rules-max-consequent requires --rules" in runs["bad"].stderr
    assert runs["zero"].returncode == 2 and "M must be at least 1" in runs["zero"].stderr
    assert not (d / "c_freqItemset").exists()


def test_flags_summary_and_metrics(tmp_path):
    import json

    from fastapriori_amd.config import JobConfig, parse_args
    from fastapriori_amd.parallel.comm import Comm
    from fastapriori_amd.pipeline import run_job
    assert parse_args(["in/", "out/", "--rules", "--rules-max-consequent", "3"]).rules_max_consequent == 3
    assert parse_args(["in/", "out/", "--rules"]).rules_max_consequent == 1
    (tmp_path / "D.dat").write_text(D)
    (tmp_path / "U.dat").write_text(U)
    log = tmp_path / "metrics.jsonl"
    job = dict(input=f"{tmp_path}/", min_support=0.5, device="cpu")
    s = run_job(JobConfig(**job, output=f"{tmp_path}/o_", rules=True, rules_max_consequent=2, metrics_path=str(log)),
                Comm())
    assert s["n_rules_exported"] == 12 and s["rules_max_consequent"] == 2
    assert (tmp_path / "o_rules" / "part-00000").read_bytes() == HAND_MULTI_BYTES
    recs = [r for r in map(json.loads, log.read_text().splitlines()) if r.get("phase") == "rules_export"]
    assert len(recs) == 1 and recs[0]["n_rules"] == 12 and recs[0]["max_consequent"] == 2


# ---------------------------------------------------------------------------
# 9. across ranks (gloo)
# ---------------------------------------------------------------------------
def _job(d: str, out: str):
    from fastapriori_amd.config import JobConfig
    from fastapriori_amd.parallel.comm import init_comm, shutdown_comm
    from fastapriori_amd.pipeline import run_job

    comm = init_comm("cpu")
    try:
        s = run_job(JobConfig(input=f"{d}/", output=f"{d}/{out}", min_support=0.02, device="cpu", rules=True,
                              min_confidence=0.3, rules_sort="leverage", rules_max_consequent=2, checkpoint=False), comm)
        return s["n_itemsets"], s["n_rules_exported"]
    finally:
        shutdown_comm(comm)


def test_world_size_two_writes_the_same_file(tmp_path):
    io.write_quest_file(str(tmp_path / "D.dat"), 1000, 8.0, 3.0, 60, 50, seed=2)
    io.write_quest_file(str(tmp_path / "U.dat"), 51, 8.0, 3.0, 60, 50, seed=2, users=True)
    ref = spawn_local(_job, 1, str(tmp_path), "w1_", timeout=300)[0]
    outs = spawn_local(_job, 2, str(tmp_path), "w2_", timeout=300)        # a hang at the meeting point times out
    assert outs[0] == ref and outs[1] == ref and ref[1] > 0
    one = (tmp_path / "w1_rules" / "part-00000").read_bytes()
    assert one == (tmp_path / "w2_rules" / "part-00000").read_bytes() and one.count(b"\n") == ref[1]
    assert any(" " in line.split(b"\t")[1].decode() for line in one.splitlines())    # some consequent has two items
