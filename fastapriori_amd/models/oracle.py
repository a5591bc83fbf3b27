"""Brute-force CPU oracle: the reference's observable behaviour, implemented literally.

This module is the ground truth every fast path (HIP kernels, the distributed
miner, the native host code) is tested against.  It deliberately shares no
code with the fast paths except the JVM-semantics helpers in
``fastapriori_amd.utils.jvm``.

Semantics reproduced:

* F1 counts token *occurrences* (``FastApriori.scala:55``: ``flatMap(_.map((_,1)))``);
  k >= 2 counts distinct sets over transactions that keep >= 2 frequent items
  (``FastApriori.scala:66-70``).
* ``minCount = ceil(minSupport * N)`` with N = all lines (``FastApriori.scala:38-39``).
* Rank = position after sort by count desc (``FastApriori.scala:60``); ties in the
  reference follow Spark's hash-partition collect order, which is not
  reproducible, so we break ties by Java string order (documented).
* Rules ``A -> s`` for every frequent S, |S| >= 2, A = S - {s},
  conf = count(S) / count(A) in IEEE double (``AssociationRules.scala:129-144``).
* Cut (``AssociationRules.scala:147-182``), sort (``:116-120``), first-match
  recommendation (``:80-106``).
"""
from __future__ import annotations

import itertools
from collections import Counter
from dataclasses import dataclass, field

from ..utils.jvm import item_tiebreak_key, java_split_ws, java_string_key, min_count, rule_tiebreak_key


@dataclass
class OracleResult:
    items: list[str]                       # rank -> token
    counts1: list[int]                     # rank -> occurrence count
    itemsets: dict[frozenset, int]         # frozenset of ranks -> count (all sizes)
    min_count: int
    n_lines: int
    rules: list[tuple[frozenset, int, float]] = field(default_factory=list)


def rank_items(counts: dict[str, int], mc: int, tiebreak: str = "string") -> list[str]:
    freq = [(t, c) for t, c in counts.items() if c >= mc]
    freq.sort(key=lambda tc: (-tc[1], item_tiebreak_key(tc[0], tiebreak)))
    return [t for t, _ in freq]


def mine(lines: list[list[str]], min_support: float, max_enum_len: int = 16, tiebreak: str = "string") -> OracleResult:
    n = len(lines)
    mc = min_count(min_support, n)
    occ = Counter()
    for toks in lines:
        occ.update(toks)
    items = rank_items(occ, mc, tiebreak)
    rank = {t: i for i, t in enumerate(items)}
    itemsets: dict[frozenset, int] = {frozenset([i]): occ[t] for i, t in enumerate(items)}

    txns: Counter = Counter()
    for toks in lines:
        s = frozenset(rank[t] for t in toks if t in rank)
        if len(s) > 1:
            txns[s] += 1

    if all(len(s) <= max_enum_len for s in txns):
        # independent brute force: every subset of every compressed transaction
        sub = Counter()
        for s, w in txns.items():
            srt = sorted(s)
            for k in range(2, len(srt) + 1):
                for c in itertools.combinations(srt, k):
                    sub[frozenset(c)] += w
        for s, c in sub.items():
            if c >= mc:
                itemsets[s] = c
    else:
        # level-wise fallback for long transactions
        prev = [frozenset([i]) for i in range(len(items))]
        k = 2
        while len(prev) >= k or k == 2:
            prevset = set(prev)
            cands = set()
            if k == 2:
                cands = {frozenset(p) for p in itertools.combinations(range(len(items)), 2)}
            else:
                for a, b in itertools.combinations(prev, 2):
                    u = a | b
                    if len(u) == k and all(u - {x} in prevset for x in u):
                        cands.add(u)
            cnt = Counter()
            for s, w in txns.items():
                for c in cands:
                    if c <= s:
                        cnt[c] += w
            prev = [c for c in cands if cnt[c] >= mc]
            for c in prev:
                itemsets[c] = cnt[c]
            k += 1
            if not prev:
                break
    return OracleResult(items=items, counts1=[occ[t] for t in items], itemsets=itemsets,
                        min_count=mc, n_lines=n)


def gen_rules(res: OracleResult) -> list[tuple[frozenset, int, float]]:
    """All rules, then the level-wise cut.  Returns the surviving rules unsorted."""
    by_level: dict[int, list[tuple[frozenset, int, float]]] = {}
    for s, c in res.itemsets.items():
        if len(s) < 2:
            continue
        for x in s:
            a = s - {x}
            by_level.setdefault(len(a), []).append((a, x, c / res.itemsets[a]))
    if not by_level:
        return []
    lo, hi = min(by_level), max(by_level)
    kept = list(by_level[lo])
    low = {(a, r): conf for a, r, conf in by_level[lo]}
    for i in range(lo + 1, hi + 1):
        nxt = {}
        for a, r, conf in by_level.get(i, []):
            ok = True
            for x in a:
                sub = a - {x}
                lc = low.get((sub, r))
                if lc is None or lc >= conf:
                    ok = False
                    break
            if ok:
                nxt[(a, r)] = conf
                kept.append((a, r, conf))
        low = nxt
    return kept


def sort_rules(rules, items: list[str]):
    """conf desc, then consequent as Int (AssociationRules.scala:116-120).  Remaining ties
    (same conf and consequent) are Spark collect order in the reference; they cannot change a
    recommendation, and we fix them as (antecedent size, antecedent ranks) for determinism."""
    return sorted(rules, key=lambda t: (-t[2], rule_tiebreak_key(items[t[1]]), len(t[0]),
                                        tuple(sorted(t[0]))))


def all_rules(res: OracleResult, min_confidence: float = 0.0, min_lift: float | None = None,
              sort: str = "confidence", limit: int | None = None) -> list[tuple]:
    """The rule export by brute force (an extension: the reference never shows its rules):
    every rule A -> c with A + {c} frequent and at least two items, NO cut, as
    (A, c, cS, cA, cC, support, confidence, lift, leverage, conviction).  Python ints for the
    products and differences, one float division per measure; the counts are the stored ones
    (level 1: occurrences).  Kept: confidence >= min_confidence and lift >= min_lift; order:
    the sort measure descending, confidence descending, the consequent's tiebreak key,
    antecedent size, antecedent ranks."""
    n = res.n_lines
    if n <= 0:
        raise ValueError("all_rules: the line total is unknown")
    out = []
    for s, cs in res.itemsets.items():
        if len(s) < 2:
            continue
        for c in s:
            a = s - {c}
            ca, cc = res.itemsets[a], res.itemsets[frozenset([c])]
            m = {"support": float(cs) / float(n), "confidence": float(cs) / float(ca),
                 "lift": float(cs * n) / float(ca * cc), "leverage": float(cs * n - ca * cc) / float(n * n),
                 "conviction": float("inf") if ca == cs else float(ca * (n - cc)) / float(n * (ca - cs))}
            if m["confidence"] >= min_confidence and (min_lift is None or m["lift"] >= min_lift):
                out.append((a, c, cs, ca, cc, m["support"], m["confidence"], m["lift"], m["leverage"], m["conviction"],
                            m[sort]))
    tie = [rule_tiebreak_key(t) for t in res.items]
    out.sort(key=lambda t: (-t[10], -t[6], tie[t[1]], len(t[0]), tuple(sorted(t[0]))))
    return [t[:10] for t in (out if limit is None else out[:limit])]


def rule_split_rows(res: OracleResult, max_consequent: int) -> list[tuple]:
    """Every rule A -> B with S = A + B frequent, A and B non-empty and disjoint and
    |B| <= max_consequent, unfiltered and unordered, as (A, B, cS, cA, cB, support, confidence,
    lift, leverage, conviction, order tail) with frozensets and all_rules' arithmetic on
    cB = count(B) (a one-item B: its occurrence count).  The order tail is (|B|, the
    consequent key -- a one-item B's tiebreak position, else its ranks --, |A|, A's ranks)."""
    n = res.n_lines
    if n <= 0:
        raise ValueError("all_rules: the line total is unknown")
    if max_consequent < 1:
        raise ValueError("all_rules: max_consequent must be at least 1")
    tie = sorted(range(len(res.items)), key=lambda r: rule_tiebreak_key(res.items[r]))
    tie_pos = {r: i for i, r in enumerate(tie)}
    out = []
    for s, cs in res.itemsets.items():
        for b in range(1, min(max_consequent, len(s) - 1) + 1):
            for cons in itertools.combinations(sorted(s), b):
                bset = frozenset(cons)
                a = s - bset
                ca, cc = res.itemsets[a], res.itemsets[bset]
                out.append((a, bset, cs, ca, cc, float(cs) / float(n), float(cs) / float(ca),
                            float(cs * n) / float(ca * cc), float(cs * n - ca * cc) / float(n * n),
                            float("inf") if ca == cs else float(ca * (n - cc)) / float(n * (ca - cs)),
                            (b, (tie_pos[cons[0]],) if b == 1 else cons, len(a), tuple(sorted(a)))))
    return out


def all_rules_multi(res: OracleResult, max_consequent: int, min_confidence: float = 0.0,
                    min_lift: float | None = None, sort: str = "confidence", limit: int | None = None,
                    rows: list | None = None) -> list[tuple]:
    """The rule export with multi-item consequents by brute force, NO cut, as (A, B, cS, cA,
    cB, support, confidence, lift, leverage, conviction).  Kept: confidence >= min_confidence
    and lift >= min_lift; order: the sort measure descending, confidence descending, then
    rule_split_rows' order tail.  ``rows``: rule_split_rows(res, max_consequent), when the
    caller has it already."""
    col = {"support": 5, "confidence": 6, "lift": 7, "leverage": 8, "conviction": 9}[sort]
    rows = rule_split_rows(res, max_consequent) if rows is None else rows
    out = [t for t in rows if t[6] >= min_confidence and (min_lift is None or t[7] >= min_lift)]
    out.sort(key=lambda t: (-t[col], -t[6], t[10]))
    return [t[:10] for t in (out if limit is None else out[:limit])]


def recommend(res: OracleResult, user_lines: list[list[str]]) -> list[str]:
    rules = sort_rules(gen_rules(res), res.items)
    rank = {t: i for i, t in enumerate(res.items)}
    out = []
    for toks in user_lines:
        u = frozenset(rank[t] for t in toks if t in rank)
        if not u:
            out.append("0")
            continue
        rec = "0"
        for a, r, _ in rules:
            if r not in u and a <= u:
                rec = res.items[r]
                break
        out.append(rec)
    return out


def recommend_topn(res: OracleResult, user_lines: list[list[str]], n: int) -> list[list[tuple[str, float]]]:
    """Ranked top-n per line (an extension: the reference has no counterpart): the first n
    firing rules in sorted order whose consequents are pairwise distinct, as (token, conf)."""
    rules = sort_rules(gen_rules(res), res.items)
    rank = {t: i for i, t in enumerate(res.items)}
    out = []
    for toks in user_lines:
        u = frozenset(rank[t] for t in toks if t in rank)
        top, seen = [], set()
        for a, r, conf in rules:
            if len(top) == n:
                break
            if r not in u and r not in seen and a <= u:
                seen.add(r)
                top.append((res.items[r], conf))
        out.append(top)
    return out


def holdout_ranks(res: OracleResult, user_lines: list[list[str]], n: int) -> list[list[tuple[str, int]]]:
    """Leave-one-out ranks per line (an extension: the reference evaluates nothing): for every
    item h of the line's basket (its distinct frequent items), in rank order, (token, the
    1-based position of h in the top-n list of the basket without h, or 0).  A basket of
    fewer than two items has no trial: its item, if any, gets 0."""
    rules = sort_rules(gen_rules(res), res.items)
    rank = {t: i for i, t in enumerate(res.items)}
    out = []
    for toks in user_lines:
        u = frozenset(rank[t] for t in toks if t in rank)
        line = []
        for h in sorted(u):
            rest, seen, pos = u - {h}, set(), 0
            for a, r, _ in rules:
                if len(u) < 2 or len(seen) == n:
                    break
                if r not in rest and r not in seen and a <= rest:
                    seen.add(r)
                    if r == h:
                        pos = len(seen)
                        break
            line.append((res.items[h], pos))
        out.append(line)
    return out


def _combined_scores(rules, weights, u: frozenset) -> list[tuple[int, int, int]]:
    """(consequent, S, f) of basket u in list order: S the summed weights of every firing rule
    with that consequent (Python ints), f the smallest such rule id; S descending, f ascending."""
    S: dict[int, int] = {}
    f: dict[int, int] = {}
    if not u:
        return []
    for i, r in [(i, t[1]) for i, t in enumerate(rules) if t[1] not in u and t[0] <= u]:
        S[r] = S.get(r, 0) + weights[i]
        f.setdefault(r, i)
    return sorted(((c, S[c], f[c]) for c in S), key=lambda t: (-t[1], t[2]))


def _combine_weights(rules, mode: str) -> list[int]:
    if mode == "sum":
        return [int(conf * 4294967296.0) for _, _, conf in rules]      # the product is exact; int() floors it
    if mode == "votes":
        return [1] * len(rules)
    raise ValueError(f"mode {mode!r} is not 'sum' or 'votes'")


def recommend_combined(res: OracleResult, user_lines: list[list[str]], n: int, mode: str) -> list[list[tuple[str, int]]]:
    """Combined scoring per line (an extension: the reference lets one rule decide): every
    firing rule adds its weight -- floor(conf * 2^32) for ``sum``, 1 for ``votes`` -- to its
    consequent; the first n consequents by sum descending, then by their first firing rule in
    sorted order, as (token, sum)."""
    rules = sort_rules(gen_rules(res), res.items)
    weights = _combine_weights(rules, mode)
    rank = {t: i for i, t in enumerate(res.items)}
    out = []
    for toks in user_lines:
        u = frozenset(rank[t] for t in toks if t in rank)
        out.append([(res.items[c], s) for c, s, _ in _combined_scores(rules, weights, u)[:n]])
    return out


def holdout_ranks_combined(res: OracleResult, user_lines: list[list[str]], n: int,
                           mode: str) -> list[list[tuple[str, int]]]:
    """Leave-one-out places per line under combined scoring: for every item h of the line's
    basket, in rank order, (token, the 1-based place of h in the combined list of the basket
    without h, or 0 when it is not among its first n).  A basket of fewer than two items has
    no trial: its item, if any, gets 0."""
    rules = sort_rules(gen_rules(res), res.items)
    weights = _combine_weights(rules, mode)
    rank = {t: i for i, t in enumerate(res.items)}
    out = []
    for toks in user_lines:
        u = frozenset(rank[t] for t in toks if t in rank)
        line = []
        for h in sorted(u):
            order = [c for c, _, _ in _combined_scores(rules, weights, u - {h})[:n]]
            line.append((res.items[h], order.index(h) + 1 if h in order else 0))
        out.append(line)
    return out


def count_itemsets(lines: list[list[str]], queries: list[list[str]]) -> list[int]:
    """Support of given itemsets by brute force (an extension: the reference counts only
    what it mines): per query the number of lines that contain every one of its tokens.  A
    LINE count -- a token repeated inside a line counts once, unlike the level-1 counts
    of ``mine`` -- with Python sets and nothing else."""
    sets = [set(toks) for toks in lines]
    return [sum(1 for s in sets if q <= s) for q in (set(q) for q in queries)]


def freq_itemset_lines(res: OracleResult) -> list[str]:
    """``Utils.saveFreqItemset``: tokens rank-descending, lines in Java String order."""
    lines = [" ".join(res.items[r] for r in sorted(s, reverse=True)) for s in res.itemsets]
    lines.sort(key=java_string_key)
    return lines


def mining_log_lines(n_items: int, itemsets) -> list[str]:
    """The reference's mining lines (FastApriori.scala:226, :107-108, :111-119, :127) with
    the millisecond values masked as '#', replayed from the frequent itemsets alone:
    the loop runs while |F_{k-1}| >= k, and a level prints the number of
    (prefix, extensions) groups genCandidates keeps (:173-190), |F_k| and its time.
    ``itemsets``: an iterable of rank sets (every size; sizes 1 are ignored)."""
    by: dict[int, set] = {}
    for s in itemsets:
        s = frozenset(s)
        by.setdefault(len(s), set()).add(s)
    F1 = n_items
    out = [f"2 candidates items {F1 * (F1 - 1) // 2}", f"2 freq items {len(by.get(2, ()))}", "Use Time 2 items #"]
    k = 3
    while len(by.get(k - 1, ())) >= k:
        prev = by[k - 1]
        # y must at least pass the subset test for x's largest item, (x - max x) + y:
        # only the largest items of x's class mates are tried
        mates: dict[frozenset, list[int]] = {}
        for x in prev:
            mates.setdefault(x - {max(x)}, []).append(max(x))
        groups = 0
        for x in prev:
            top = max(x)
            for y in mates[x - {top}]:
                if y > top and all((x - {xi}) | {y} in prev for xi in x):
                    groups += 1
                    break
        out += [f"{k} candidate items {groups}", f"{k} freq items {len(by.get(k, ()))}", f"Use Time {k} items #"]
        k += 1
    out.append(f"Total freq items sets {sum(len(v) for kk, v in by.items() if kk >= 2)}")
    return out


def run_oracle(d_lines: list[str], u_lines: list[str], min_support: float, tiebreak: str = "string"):
    D = [java_split_ws(l) for l in d_lines]
    U = [java_split_ws(l) for l in u_lines]
    res = mine(D, min_support, tiebreak=tiebreak)
    return freq_itemset_lines(res), recommend(res, U), res
