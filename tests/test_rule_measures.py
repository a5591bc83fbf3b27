"""The rule export (--rules, AssociationRules.all_rules) on the CPU path: every rule with
support, confidence, lift, leverage and conviction against a hand example, the oracle's brute
force from Python ints (bit for bit), counts near 2^31, occurrence counts above the line total,
thresholds on occurring values, shapes with little to do, the native writer against repr(),
the command line and two gloo ranks.  tests/test_gpu_rule_measures.py runs the same cases on
the device."""
import functools
import itertools
import math
import os
import subprocess
import sys

import numpy as np
import pytest

from fastapriori_amd.models import oracle
from fastapriori_amd.models.data import MiningResult
from fastapriori_amd.models.rules import AssociationRules
from fastapriori_amd.ops import host
from fastapriori_amd.parallel.launch import spawn_local
from fastapriori_amd.utils import io
from fastapriori_amd.utils.metrics import Logger

from test_condense import D, U, _mine, quest300

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ("ante_off", "ante", "cons", "cnt_s", "cnt_a", "cnt_c", "support", "conf", "lift", "leverage", "conviction")
DTYPES = dict(ante_off=np.int64, ante=np.int32, cons=np.int32, cnt_s=np.int64, cnt_a=np.int64, cnt_c=np.int64,
              support=np.float64, conf=np.float64, lift=np.float64, leverage=np.float64, conviction=np.float64)
INF = math.inf


# ---------------------------------------------------------------------------
# helpers (shared with the device tests)
# ---------------------------------------------------------------------------
def all_rules(res, device="cpu", **kw) -> host.RuleMeasures:
    return AssociationRules(res, logger=Logger(enabled=False), device=device).all_rules(**kw)


def as_oracle(res: MiningResult) -> oracle.OracleResult:
    """A mined (or synthetic) result as the oracle's input: frozensets and Python ints."""
    return oracle.OracleResult(items=res.items, counts1=[int(c) for c in res.counts[0]], itemsets=res.as_dict(),
                               min_count=res.min_count, n_lines=res.n_lines)


def table(rows) -> host.RuleMeasures:
    """The oracle's (A, c, cS, cA, cC, five measures) tuples as a RuleMeasures."""
    antes = [sorted(r[0]) for r in rows]
    off = np.zeros(len(rows) + 1, dtype=np.int64)
    if rows:
        off[1:] = np.cumsum([len(a) for a in antes])
    cols = [np.array([r[j] for r in rows], dtype=t) for j, t in
            ((1, np.int32), (2, np.int64), (3, np.int64), (4, np.int64), (5, np.float64), (6, np.float64),
             (7, np.float64), (8, np.float64), (9, np.float64))]
    return host.RuleMeasures(off, np.array([x for a in antes for x in a], dtype=np.int32), *cols)


def same(got: host.RuleMeasures, want: host.RuleMeasures) -> None:
    """Equal arrays, the doubles bit for bit: the tolerance IS equality (exact int64 products
    and one division per measure, see csrc/host/fa_rule_measures.h)."""
    assert got.n_rules == want.n_rules
    for f in FIELDS:
        g, w = getattr(got, f), getattr(want, f)
        assert g.dtype == DTYPES[f] and g.shape == w.shape, f
        if g.dtype == np.float64:
            g, w = g.view(np.int64), np.ascontiguousarray(w).view(np.int64)
        assert np.array_equal(g, w), f


def synthetic(n_lines: int, level1: list, level2: dict, items=None) -> MiningResult:
    """A two-level result: level1 counts by rank, level2 {(a, b): count}."""
    pairs = sorted(level2)
    return MiningResult(items or [f"t{i}" for i in range(len(level1))],
                        [np.arange(len(level1), dtype=np.int32).reshape(-1, 1),
                         np.array(pairs, dtype=np.int32).reshape(-1, 2)],
                        [np.array(level1, dtype=np.int64), np.array([level2[p] for p in pairs], dtype=np.int64)],
                        1, n_lines)


A30 = 2 ** 30
BIG_N = 2 ** 31 - 1


def large_counts() -> MiningResult:
    """N = 2^31 - 1, counts near 2^30 and 2^31 - 3.  For 0 -> 1 the two products of the
    leverage, (2^30 + 5)(2^31 - 1) and (2^31 - 3)(2^30 + 7), are near 2^61 and differ by
    16 - 2^31: 32-bit products and products taken in doubles both miss it."""
    return synthetic(BIG_N, [2 ** 31 - 3, A30 + 7, A30 - 5],
                     {(0, 1): A30 + 5, (0, 2): A30 - 9, (1, 2): 12345})


REPEATED = ("1 1 1 2\n1 2\n", "1 1 1 2\n1 2\n2\n")      # item 1 occurs 4 times on 2 (3) lines


def small_lattice(with_16_17: bool = False):
    """test_condense.lattice's shape with small counts: every k-combination of items 0..10,
    the 3-clique {11, 12, 13}, the pair {14, 15} and, on request, {16, 17};
    count(S) = N0 - sum of w_i over S with N0 = 2^31 - 1 lines.  11264 = 44 x 256 (itemset,
    position) elements above level 1, or 11266: two live threads in a 45th workgroup."""
    w = {i: 3 * i + 1 for i in range(18)}
    w.update({2: 0, 7: 0, 5: 2 ** 29})
    groups = [tuple(range(11)), (11, 12, 13), (14, 15)] + ([(16, 17)] if with_16_17 else [])
    levels, counts = [], []
    for k in range(1, 12):
        rows = sorted(c for g in groups for c in itertools.combinations(g, k))
        levels.append(np.array(rows, dtype=np.int32).reshape(-1, k))
        counts.append(np.array([BIG_N - sum(w[i] for i in r) for r in rows], dtype=np.int64))
    assert sum(len(l) * k for k, l in enumerate(levels, 1) if k >= 2) == (11266 if with_16_17 else 11264)
    return MiningResult([str(i) for i in range(18)], levels, counts, 1, BIG_N)


SCAN_CHUNK = 1024      # csrc/hip/rules.hip kRmScanTPB: per-workgroup totals per chunk of the one scan
CUBE_CONF = 0.9


@functools.lru_cache(maxsize=None)
def cube(n_items: int = 18):
    """All subsets of n_items items, count(S) = N0 - sum of the distinct weights 100 + 10 i:
    18 items give 2359278 (itemset, position) elements in 9216 workgroups of 256, nine chunks
    of the scan of their totals.  Returns (result, selected per workgroup at CUBE_CONF), the
    latter from numpy on a table of counts by bitmask."""
    w = np.array([100 + 10 * i for i in range(n_items)], dtype=np.int64)
    n0 = int(w.sum()) + 30
    by_mask = n0 - ((np.arange(1 << n_items)[:, None] >> np.arange(n_items)) & 1) @ w
    levels, counts, sel = [], [], []
    for k in range(1, n_items + 1):
        rows = np.array(list(itertools.combinations(range(n_items), k)), dtype=np.int32).reshape(-1, k)
        mask = (1 << rows.astype(np.int64)).sum(1)
        levels.append(rows)
        counts.append(by_mask[mask])
        if k >= 2:
            c_a = by_mask[mask[:, None] ^ (1 << rows.astype(np.int64))]
            sel.append((by_mask[mask][:, None].astype(np.float64) / c_a.astype(np.float64) >= CUBE_CONF).reshape(-1))
    sel = np.concatenate(sel)
    per_wg = np.add.reduceat(sel.astype(np.int64), np.arange(0, sel.size, 256))
    assert per_wg.size > SCAN_CHUNK, "the per-workgroup totals must cross one scan chunk: raise n_items"
    return MiningResult([str(i) for i in range(n_items)], levels, counts, 1, n0), per_wg


# ---------------------------------------------------------------------------
# 1. the hand example
# ---------------------------------------------------------------------------
# D: N = 4, items 1, 2, 3 (ranks 0, 1, 2) occur 3 times each; {1,2}: 3, {1,3}: 2, {2,3}: 2,
# {1,2,3}: 2.  Every (S, c) of the three pairs and the triple: 6 + 3 = 9 rules.
# (antecedent tokens, consequent, cS, cA, cC, support, confidence, lift, leverage, conviction)
HAND = [
    (("2",), "1", 3, 3, 3, 0.75, 1.0, 12 / 9, 3 / 16, INF),
    (("2", "3"), "1", 2, 2, 3, 0.5, 1.0, 8 / 6, 2 / 16, INF),
    (("1",), "2", 3, 3, 3, 0.75, 1.0, 12 / 9, 3 / 16, INF),
    (("1", "3"), "2", 2, 2, 3, 0.5, 1.0, 8 / 6, 2 / 16, INF),
    (("3",), "1", 2, 3, 3, 0.5, 2 / 3, 8 / 9, -1 / 16, 3 / 4),
    (("3",), "2", 2, 3, 3, 0.5, 2 / 3, 8 / 9, -1 / 16, 3 / 4),
    (("1",), "3", 2, 3, 3, 0.5, 2 / 3, 8 / 9, -1 / 16, 3 / 4),
    (("2",), "3", 2, 3, 3, 0.5, 2 / 3, 8 / 9, -1 / 16, 3 / 4),
    (("1", "2"), "3", 2, 3, 3, 0.5, 2 / 3, 8 / 9, -1 / 16, 3 / 4),
]
HAND_BYTES = (b"2\t1\t3\t3\t3\t0.75\t1.0\t1.3333333333333333\t0.1875\tinf\n"
              b"3 2\t1\t2\t2\t3\t0.5\t1.0\t1.3333333333333333\t0.125\tinf\n"
              b"1\t2\t3\t3\t3\t0.75\t1.0\t1.3333333333333333\t0.1875\tinf\n"
              b"3 1\t2\t2\t2\t3\t0.5\t1.0\t1.3333333333333333\t0.125\tinf\n"
              b"3\t1\t2\t3\t3\t0.5\t0.6666666666666666\t0.8888888888888888\t-0.0625\t0.75\n"
              b"3\t2\t2\t3\t3\t0.5\t0.6666666666666666\t0.8888888888888888\t-0.0625\t0.75\n"
              b"1\t3\t2\t3\t3\t0.5\t0.6666666666666666\t0.8888888888888888\t-0.0625\t0.75\n"
              b"2\t3\t2\t3\t3\t0.5\t0.6666666666666666\t0.8888888888888888\t-0.0625\t0.75\n"
              b"2 1\t3\t2\t3\t3\t0.5\t0.6666666666666666\t0.8888888888888888\t-0.0625\t0.75\n")
# --min-confidence 0.6 --rules-sort lift: all nine pass, lift 4/3 before 8/9 (the same order)
HAND_LIFT_BYTES = HAND_BYTES


def rows_of(rm: host.RuleMeasures, items) -> list:
    return [(tuple(items[r] for r in rm.antecedent(i)), items[rm.cons[i]], int(rm.cnt_s[i]), int(rm.cnt_a[i]),
             int(rm.cnt_c[i]), float(rm.support[i]), float(rm.conf[i]), float(rm.lift[i]), float(rm.leverage[i]),
             float(rm.conviction[i])) for i in range(rm.n_rules)]


def check_hand(rm: host.RuleMeasures, res) -> None:
    assert res.n_itemsets == 7 and res.n_lines == 4 and res.items == ["1", "2", "3"]
    assert rows_of(rm, res.items) == HAND                       # float ==: the exact doubles
    assert [rm.antecedent(i).tolist() for i in (1, 8)] == [[1, 2], [0, 1]]
    same(rm, table(oracle.all_rules(as_oracle(res))))


def test_hand_example(tmp_path):
    res = _mine(D, 0.5)
    rm = all_rules(res)
    check_hand(rm, res)
    assert rm.lift[8] == 8 / 9 and rm.conviction[2] == INF      # {1,2} -> 3 and 1 -> 2
    part = io.write_rules(rm, res.items, str(tmp_path / "rules"))
    assert open(part, "rb").read() == HAND_BYTES and (tmp_path / "rules" / "_SUCCESS").exists()
    with pytest.raises(io.OutputExistsError):
        io.write_rules(rm, res.items, str(tmp_path / "rules"))
    io.write_rules(rm, res.items, str(tmp_path / "rules"), overwrite=True)


# ---------------------------------------------------------------------------
# 2. C++ against the oracle's brute force on the mined case
# ---------------------------------------------------------------------------
SORTS = ("confidence", "lift", "leverage", "conviction", "support")
THRESHOLDS = [dict(min_confidence=0.0), dict(min_confidence=0.5), dict(min_confidence=1.0),
              dict(min_confidence=0.0, min_lift=1.0), dict(min_confidence=0.5, min_lift=1.0)]


@functools.lru_cache(maxsize=None)
def quest_oracle(sort: str, min_confidence: float, min_lift):
    """The oracle's rows for the mined case.  The brute force runs once per sort measure, with
    no threshold; a thresholded list is that list filtered on the oracle's own Python floats
    (a filter keeps the order), which test_thresholded_oracle_is_the_filtered_one checks."""
    if min_confidence == 0.0 and min_lift is None:
        return oracle.all_rules(as_oracle(quest300()[0]), sort=sort)
    return [r for r in quest_oracle(sort, 0.0, None) if r[6] >= min_confidence and (min_lift is None or r[7] >= min_lift)]


def test_thresholded_oracle_is_the_filtered_one():
    assert quest_oracle("leverage", 0.5, 1.0) == oracle.all_rules(as_oracle(quest300()[0]), 0.5, 1.0, "leverage")


def quest_cases():
    """(options, expected table): every sort with no threshold, every threshold set under two
    sorts (each sort under two sets), then limits around R."""
    for i, sort in enumerate(SORTS):
        for th in [THRESHOLDS[0]] + [THRESHOLDS[1 + (i + j) % 4] for j in (0, 1)]:
            yield dict(th, sort=sort), table(quest_oracle(sort, th["min_confidence"], th.get("min_lift")))
    rows = quest_oracle("lift", 0.5, None)
    R = len(rows)
    for limit in (0, 1, R - 1, R, R + 1):
        yield dict(min_confidence=0.5, sort="lift", limit=limit), table(rows[:limit])


def test_cpp_equals_the_oracle_on_the_mined_case():
    res = quest300()[0]
    n_all = sum(len(l) * k for k, l in enumerate(res.levels, 1) if k >= 2)
    seen = set()
    for kw, want in quest_cases():
        same(all_rules(res, **kw), want)
        seen.add(want.n_rules)
    assert n_all in seen and 0 in seen and len(seen) > 6          # everything, nothing, and cuts between
    full = table(quest_oracle("conviction", 0.0, None))
    assert np.isinf(full.conviction[0]) and not np.isinf(full.conviction[-1])      # +inf sorts first
    assert (full.leverage < 0).any() and (full.lift < 1).any()


# ---------------------------------------------------------------------------
# 3. / 4. large counts, occurrence counts above the line total
# ---------------------------------------------------------------------------
def check_large_counts(run) -> None:
    res = large_counts()
    for sort in SORTS:
        same(run(res, sort=sort), table(oracle.all_rules(as_oracle(res), sort=sort)))
    rm = run(res, sort="leverage")
    i = next(i for i in range(rm.n_rules) if (rm.antecedent(i).tolist(), int(rm.cons[i])) == ([0], 1))
    cs, ca, cc, n = A30 + 5, 2 ** 31 - 3, A30 + 7, BIG_N
    assert (int(rm.cnt_s[i]), int(rm.cnt_a[i]), int(rm.cnt_c[i])) == (cs, ca, cc)
    assert cs * n - ca * cc == 16 - 2 ** 31
    assert rm.leverage[i] == float(16 - 2 ** 31) / float(n * n)
    assert rm.leverage[i] != (float(cs) * float(n) - float(ca) * float(cc)) / (float(n) * float(n))
    assert rm.lift[i] == float(cs * n) / float(ca * cc) and rm.lift[i] != float((cs * n) % 2 ** 32) / float(ca * cc)
    assert rm.conviction[i] == float(ca * (n - cc)) / float(n * (ca - cs))


def test_large_counts():
    check_large_counts(all_rules)
    for bad in (synthetic(2 ** 31, [5, 4], {(0, 1): 3}), synthetic(100, [2 ** 31, 4], {(0, 1): 3}),
                synthetic(100, [5, 4], {(0, 1): 2 ** 31})):
        with pytest.raises(ValueError, match=r"2\^31 - 1"):
            all_rules(bad)
    assert all_rules(synthetic(BIG_N, [BIG_N, 4], {(0, 1): 3})).n_rules == 2       # the limit itself is fine


def check_repeated_token(run) -> None:
    r2, r3 = (_mine(text, 0.5) for text in REPEATED)
    assert r2.n_lines == 2 and r2.counts[0].tolist() == [4, 2] and r2.items == ["1", "2"]
    for res in (r2, r3):
        for sort in ("leverage", "conviction"):
            same(run(res, sort=sort), table(oracle.all_rules(as_oracle(res), sort=sort)))
    # 1 1 1 2 / 1 2: both rules have leverage (2 * 2 - 4 * 2) / 4 = -1
    assert run(r2).leverage.tolist() == [-1.0, -1.0]
    # ... and a third line "2": 2 -> 1 has cS = 2, cA = 3, cC = 4 > N = 3
    rm = run(r3)
    i = int(np.flatnonzero(rm.cons == r3.items.index("1"))[0])
    assert (int(rm.cnt_s[i]), int(rm.cnt_a[i]), int(rm.cnt_c[i])) == (2, 3, 4)
    assert rm.conviction[i] == float(3 * (3 - 4)) / float(3 * (3 - 2)) == -1.0
    assert rm.leverage[i] == float(2 * 3 - 3 * 4) / 9.0 < 0


def test_repeated_token_on_a_line():
    check_repeated_token(all_rules)


# ---------------------------------------------------------------------------
# 5. thresholds on occurring values
# ---------------------------------------------------------------------------
def check_thresholds(run) -> None:
    res = _mine(D, 0.5)
    assert run(res, min_confidence=2 / 3).n_rules == 9                      # the bound is inclusive
    assert run(res, min_confidence=math.nextafter(2 / 3, 1.0)).n_rules == 4
    assert run(res, min_confidence=1.0).n_rules == 4
    assert run(res, min_lift=8 / 9).n_rules == 9 and run(res, min_lift=math.nextafter(8 / 9, 1.0)).n_rules == 4
    none = run(res, min_confidence=math.nextafter(1.0, 2.0))
    assert none.n_rules == 0 and none.ante_off.tolist() == [0]
    same(none, table([]))


def test_thresholds(tmp_path):
    check_thresholds(all_rules)
    res = _mine(D, 0.5)
    part = io.write_rules(all_rules(res, min_confidence=1.5), res.items, str(tmp_path / "rules"))
    assert os.path.getsize(part) == 0 and (tmp_path / "rules" / "_SUCCESS").exists()


# ---------------------------------------------------------------------------
# 6. shapes with little to do
# ---------------------------------------------------------------------------
def little_to_do() -> dict:
    l1, c1 = np.array([[0], [1], [2]], dtype=np.int32), np.array([5, 4, 3], dtype=np.int64)
    e2, e3 = np.zeros((0, 2), np.int32), np.zeros((0, 3), np.int32)
    z = np.zeros(0, np.int64)
    l2, c2 = np.array([[0, 1], [0, 2]], dtype=np.int32), np.array([4, 2], dtype=np.int64)
    mk = lambda lv, ct: MiningResult(["a", "b", "c"], lv, ct, 1, 6)       # noqa: E731
    return {"level1_only": (mk([l1], [c1]), 0), "empty_level2": (mk([l1, e2], [c1, z]), 0),
            "no_levels": (mk([], []), 0), "trailing_empty": (mk([l1, l2, e3], [c1, c2, z]), 4)}


def missing_subset() -> MiningResult:
    """quest300 without one 3-subset of its first 4-itemset."""
    res = quest300()[0]
    levels, counts = [l.copy() for l in res.levels], [c.copy() for c in res.counts]
    hit = int(np.flatnonzero((levels[2] == levels[3][0][:3]).all(1))[0])
    levels[2], counts[2] = np.delete(levels[2], hit, 0), np.delete(counts[2], hit)
    return MiningResult(res.items, levels, counts, res.min_count, res.n_lines)


@pytest.mark.parametrize("name", sorted(little_to_do()))
def test_shapes_with_little_to_do(name):
    res, n = little_to_do()[name]
    rm = all_rules(res)
    assert rm.n_rules == n and rm.ante_off.size == n + 1
    same(rm, table(oracle.all_rules(as_oracle(res)) if res.levels else []))


def test_errors():
    res = _mine(D, 0.5)
    with pytest.raises(ValueError, match="line total is unknown"):
        all_rules(MiningResult(res.items, res.levels, res.counts, res.min_count, 0))
    with pytest.raises(RuntimeError, match="size 4 has a subset that is not in level 3"):
        all_rules(missing_subset())
    with pytest.raises(RuntimeError, match=r"size \d+ has a subset that is not in level \d+"):
        all_rules(quest300()[1])                                           # the closed form: not downward closed
    gap = little_to_do()["trailing_empty"][0]
    with pytest.raises(RuntimeError, match="size 3 has a subset that is not in level 2"):
        all_rules(MiningResult(gap.items, [gap.levels[0], gap.levels[2][:0].reshape(0, 2),
                                           np.array([[0, 1, 2]], dtype=np.int32)],
                               [gap.counts[0], gap.counts[2], np.array([1], dtype=np.int64)], 1, 6))
    no_cons = synthetic(10, [5, 4], {(0, 1): 3})
    no_cons.levels[0], no_cons.counts[0] = no_cons.levels[0][:1], no_cons.counts[0][:1]
    with pytest.raises(RuntimeError, match="size 2 has a subset that is not in level 1"):
        all_rules(no_cons)
    with pytest.raises(ValueError):
        all_rules(res, sort="jaccard")
    with pytest.raises(ValueError):
        all_rules(res, limit=-1)


# ---------------------------------------------------------------------------
# 7. the writer
# ---------------------------------------------------------------------------
def py_lines(rm: host.RuleMeasures, items) -> bytes:
    out = []
    for i in range(rm.n_rules):
        f = [" ".join(items[r] for r in rm.antecedent(i)[::-1]), items[rm.cons[i]], str(int(rm.cnt_s[i])),
             str(int(rm.cnt_a[i])), str(int(rm.cnt_c[i]))]
        f += [repr(float(v[i])) for v in (rm.support, rm.conf, rm.lift, rm.leverage, rm.conviction)]
        out.append("\t".join(f) + "\n")
    return "".join(out).encode("utf-8")


def test_writer_formats_floats_as_repr(tmp_path):
    vals = [1.0, 0.1, 1e-05, 1e16, 123456789012345.6, -0.25, INF, 5e-324, 2 / 3, -INF, 0.0, 1e15, 9999999999999998.0,
            0.0001, 0.00001234, 1.5e300, 1e22, 123.0, -1e-7, 2.5e-308, 1.7976931348623157e308]
    n = len(vals)
    items = ["apple", "béta", "c:d", "中文"]
    v = np.array(vals, dtype=np.float64)
    rm = host.RuleMeasures(np.arange(0, 2 * n + 1, 2, dtype=np.int64), np.tile(np.array([0, 2], np.int32), n),
                           np.array([1 + 2 * (i % 2) for i in range(n)], dtype=np.int32),
                           np.arange(n, dtype=np.int64), np.full(n, BIG_N, np.int64), np.full(n, 7, np.int64),
                           v, v[::-1].copy(), np.roll(v, 1), np.roll(v, 2), np.roll(v, 3))
    got = open(io.write_rules(rm, items, str(tmp_path / "rules")), "rb").read()
    assert got == py_lines(rm, items)
    first = got.split(b"\n")[0].decode("utf-8").split("\t")
    assert first[:5] == ["c:d apple", "béta", "0", str(BIG_N), "7"] and first[5] == "1.0"
    for tok in ("0.1", "1e-05", "1e+16", "123456789012345.6", "-0.25", "inf", "-inf", "5e-324", "0.6666666666666666"):
        assert ("\t" + tok).encode() in got
    # dictionary tokens round-trip
    back = [l.split("\t") for l in got.decode("utf-8").splitlines()]
    assert [(l[0].split(" ")[::-1], l[1]) for l in back] == [(["apple", "c:d"], items[c]) for c in rm.cons.tolist()]
    assert [float(l[5]) for l in back] == vals
    # ... and a mined dictionary vocabulary
    res = _mine("tea milk\ntea milk sugar\ntea\nmilk sugar\n", 0.5)
    assert not any(t.isdigit() for t in res.items)
    rm = all_rules(res, sort="lift")
    got = open(io.write_rules(rm, res.items, str(tmp_path / "rules2")), "rb").read()
    assert got == py_lines(rm, res.items) and rm.n_rules == 4


# ---------------------------------------------------------------------------
# 8. command line
# ---------------------------------------------------------------------------
def _cli(d, out, *flags):
    env = dict(os.environ, PYTHONPATH=ROOT)
    return subprocess.run([sys.executable, "-m", "fastapriori_amd", f"{d}/", f"{d}/{out}", f"{d}/tmp_{out}",
                           "--min-support", "0.5", "--device", "cpu", *flags],
                          capture_output=True, text=True, env=env, timeout=300)


@pytest.fixture(scope="module")
def cli_runs(tmp_path_factory):
    d = tmp_path_factory.mktemp("rules")
    (d / "D.dat").write_text(D)
    (d / "U.dat").write_text(U)
    opts = ("--rules", "--min-confidence", "0.6", "--rules-sort", "lift")
    runs = {"plain": _cli(d, "a_"), "rules": _cli(d, "b_", *opts)}
    os.rename(d / "b_rules", d / "b_rules_first")
    runs["rules_only"] = _cli(d, "b_", "--rules-only", "--overwrite", *opts)
    runs["bad"] = _cli(d, "c_", "--min-lift", "1.0")
    return d, runs


def test_cli_writes_the_rules(cli_runs):
    d, runs = cli_runs
    assert all(runs[k].returncode == 0 for k in ("plain", "rules", "rules_only")), [r.stderr for r in runs.values()]
    first = (d / "b_rules_first" / "part-00000").read_bytes()
    assert first == HAND_LIFT_BYTES and (d / "b_rules_first" / "_SUCCESS").exists()
    assert (d / "b_rules" / "part-00000").read_bytes() == first            # --rules-only from the checkpoint
    out = runs["rules"].stdout
    assert "==== Total time for get rules " in out
    assert out.index("Total time for get freqItemsets") < out.index("Total time for get rules") \
        < out.index("Total time for get recommends")
    assert "Total time for get rules" in runs["rules_only"].stdout


def test_cli_without_the_flag_nothing_changes(cli_runs):
    d, runs = cli_runs
    assert not (d / "a_rules").exists() and "get rules" not in runs["plain"].stdout
    for name in ("freqItemset", "recommends"):
        assert (d / f"a_{name}" / "part-00000").read_bytes() == (d / f"b_{name}" / "part-00000").read_bytes()
    assert runs["bad"].returncode == 2 and "--min-lift requires --rules" in runs["bad"].stderr
    assert not (d / "c_freqItemset").exists()


def test_flags_summary_and_metrics(tmp_path):
    import json

    from fastapriori_amd.config import JobConfig, parse_args
    from fastapriori_amd.parallel.comm import Comm
    from fastapriori_amd.pipeline import run_job
    cfg = parse_args(["in/", "out/", "--rules", "--min-confidence", "0.25", "--min-lift", "1.5", "--rules-sort",
                      "conviction", "--rules-limit", "7"])
    assert (cfg.rules, cfg.min_confidence, cfg.min_lift, cfg.rules_sort, cfg.rules_limit) == \
        (True, 0.25, 1.5, "conviction", 7)
    cfg = parse_args(["in/", "out/", "--rules"])
    assert (cfg.rules, cfg.min_confidence, cfg.min_lift, cfg.rules_sort, cfg.rules_limit) == \
        (True, 0.0, None, "confidence", None)
    assert not parse_args(["in/", "out/"]).rules
    for flags in (["--min-confidence", "0.5"], ["--rules-sort", "lift"], ["--rules-limit", "3"],
                  ["--rules", "--rules-limit", "-1"], ["--rules", "--rules-sort", "jaccard"]):
        with pytest.raises(SystemExit):
            parse_args(["in/", "out/", *flags])
    (tmp_path / "D.dat").write_text(D)
    (tmp_path / "U.dat").write_text(U)
    log = tmp_path / "metrics.jsonl"
    job = dict(input=f"{tmp_path}/", min_support=0.5, device="cpu")
    s = run_job(JobConfig(**job, output=f"{tmp_path}/o_", rules=True, min_lift=1.0, rules_limit=3,
                          metrics_path=str(log)), Comm())
    assert s["n_rules_exported"] == 3
    assert (tmp_path / "o_rules" / "part-00000").read_bytes() == b"".join(HAND_BYTES.splitlines(True)[:3])
    recs = [r for r in map(json.loads, log.read_text().splitlines()) if r.get("phase") == "rules_export"]
    assert len(recs) == 1 and recs[0]["n_rules"] == 3 and "ms" in recs[0]
    assert "n_rules_exported" not in run_job(JobConfig(**job, output=f"{tmp_path}/p_"), Comm())
    os.makedirs(tmp_path / "q_rules")                                      # --overwrite applies as elsewhere
    with pytest.raises(RuntimeError, match="--rules failed on rank 0: OutputExistsError"):
        run_job(JobConfig(**job, output=f"{tmp_path}/q_", rules=True), Comm())
    assert run_job(JobConfig(**job, output=f"{tmp_path}/q_", rules=True, overwrite=True), Comm())["n_rules_exported"] == 9


def test_rules_only_from_saved_files_has_no_line_total(tmp_path):
    from fastapriori_amd.config import JobConfig
    from fastapriori_amd.parallel.comm import Comm
    from fastapriori_amd.pipeline import run_job
    (tmp_path / "D.dat").write_text(D)
    (tmp_path / "U.dat").write_text(U)
    job = dict(input=f"{tmp_path}/", output=f"{tmp_path}/o_", min_support=0.5, device="cpu")
    run_job(JobConfig(**job, with_counts=True), Comm())
    with pytest.raises(RuntimeError, match="--rules failed on rank 0: ValueError: .*line total is unknown"):
        run_job(JobConfig(**job, rules_only=True, rules=True, overwrite=True), Comm())


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
                              min_confidence=0.3, rules_sort="leverage", checkpoint=False), comm)
        return s["n_itemsets"], s["n_rules_exported"]
    finally:
        shutdown_comm(comm)


def test_world_size_two_writes_the_same_file(tmp_path):
    io.write_quest_file(str(tmp_path / "D.dat"), 2000, 8.0, 3.0, 60, 50, seed=2)
    io.write_quest_file(str(tmp_path / "U.dat"), 101, 8.0, 3.0, 60, 50, seed=2, users=True)
    ref = spawn_local(_job, 1, str(tmp_path), "w1_", timeout=300)[0]
    outs = spawn_local(_job, 2, str(tmp_path), "w2_", timeout=300)        # a hang at the meeting point times out
    assert outs[0] == ref and outs[1] == ref and ref[1] > 0
    one = (tmp_path / "w1_rules" / "part-00000").read_bytes()
    assert one == (tmp_path / "w2_rules" / "part-00000").read_bytes() and one.count(b"\n") == ref[1]
