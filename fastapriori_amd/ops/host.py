"""Host-side native ops (libfa_host.so): candidate generation and rule building."""
from __future__ import annotations

import ctypes as C
import math
from dataclasses import dataclass, field

import numpy as np

from ..config import RULE_SORTS          # in fa_rule_measures.h RuleSort's order
from ..utils.env import num_threads
from . import _native


def apriori_gen(prev: np.ndarray):
    """Join + full-prune candidate generation (csrc/host/apriori_gen.cpp).

    prev: int32 [n, m] frequent m-itemsets (rows ascending, lexicographic).
    Returns (prefix_idx int32 [G], ext_off int64 [G+1], ext int32 [C]).
    """
    prev = np.ascontiguousarray(prev, dtype=np.int32)
    n, m = prev.shape
    sizes = np.zeros(2, dtype=np.int64)
    lib = _native.host()
    h = lib.fa_apriori_gen(prev.ctypes.data, n, m, num_threads(), sizes.ctypes.data)
    G, Cn = int(sizes[0]), int(sizes[1])
    prefix = np.zeros(max(G, 1), dtype=np.int32)
    ext_off = np.zeros(G + 1, dtype=np.int64)
    ext = np.zeros(max(Cn, 1), dtype=np.int32)
    lib.fa_cands_export(h, prefix.ctypes.data, ext_off.ctypes.data, ext.ctypes.data)
    lib.fa_cands_free(h)
    return prefix[:G], ext_off, ext[:Cn]


class RgLevelC(C.Structure):
    """regroup.cpp RgLevel: one level of a bundle in the generator's form and its regrouped form."""
    _fields_ = [(n, C.c_void_p) for n in ("P", "cnt", "off", "ex")] + \
               [(n, C.c_int64) for n in ("n", "C", "m")] + \
               [(n, C.c_void_p) for n in ("cnt_out", "off_out", "ex_out", "perm")] + \
               [(n, C.c_int64) for n in ("pieces_prefix", "pieces_rule", "rounds", "kept_prefix")]


def dl_regroup(levels) -> tuple[bool, list[dict]]:
    """Host model of the device bundles' regrouping step (csrc/host/fa_regroup.h, regroup.cpp).

    levels: per level (P int32 [n, m] parent rows, cnt int32 [n] extensions per row, ex int32 [C]
    their ids in row order), as the generator leaves them.  Returns (the bundle regroups, per
    level dict(cnt int32 [n], off int64 [n + 1], ex int32 [C], perm int32 [C] with perm[new
    index] = old index inside the level, pieces_prefix, pieces_rule, rounds, kept_prefix)).
    """
    L = len(levels)
    arr = (RgLevelC * L)()
    keep, out = [], []
    for l, (P, cnt, ex) in enumerate(levels):
        P = np.ascontiguousarray(P, dtype=np.int32)
        cnt = np.ascontiguousarray(cnt, dtype=np.int32)
        ex = np.ascontiguousarray(ex, dtype=np.int32)
        n, m = P.shape
        Cn = int(ex.size)
        assert cnt.shape == (n,) and int(cnt.sum()) == Cn
        off = np.concatenate([[0], np.cumsum(cnt, dtype=np.int64)]).astype(np.int64)
        o = dict(cnt=np.zeros(n, np.int32), off=np.zeros(n + 1, np.int64), ex=np.zeros(max(Cn, 1), np.int32),
                 perm=np.zeros(max(Cn, 1), np.int32))
        keep.append((P, cnt, ex, off))
        a = arr[l]
        a.P, a.cnt, a.off, a.ex = P.ctypes.data, cnt.ctypes.data, off.ctypes.data, ex.ctypes.data
        a.n, a.C, a.m = n, Cn, m
        a.cnt_out, a.off_out, a.ex_out, a.perm = (o[k].ctypes.data for k in ("cnt", "off", "ex", "perm"))
        out.append(o)
    regrouped = bool(_native.host().fa_dl_regroup(C.addressof(arr), L))
    for l, o in enumerate(out):
        Cn = int(arr[l].C)
        o["ex"], o["perm"] = o["ex"][:Cn], o["perm"][:Cn]
        for k in ("pieces_prefix", "pieces_rule", "rounds", "kept_prefix"):
            o[k] = int(getattr(arr[l], k))
    return regrouped, out


@dataclass
class RuleTable:
    """Rules after the cut, in recommendation order (conf desc, tiebreak)."""
    ante_off: np.ndarray   # int64 [R+1]
    ante: np.ndarray       # int32 concatenated antecedent ranks (ascending)
    cons: np.ndarray       # int32 [R]
    conf: np.ndarray       # float64 [R]
    level_stats: list      # [(antecedent size, before cut, after cut)]
    level_ms: list = field(default_factory=list)   # [ms of each level's cut], same order

    @property
    def n_rules(self) -> int:
        return int(self.cons.size)

    def antecedent(self, i: int) -> np.ndarray:
        return self.ante[self.ante_off[i]:self.ante_off[i + 1]]


@dataclass
class RuleMeasures:
    """The exported rules (AssociationRules.all_rules): every rule A -> c of every frequent
    S = A + {c}, without the cut, in the chosen order, with its three stored counts and five
    measures (csrc/host/fa_rule_measures.h; level-1 counts are occurrence counts)."""
    ante_off: np.ndarray    # int64 [R+1]
    ante: np.ndarray        # int32 concatenated antecedent ranks (ascending)
    cons: np.ndarray        # int32 [R]
    cnt_s: np.ndarray       # int64 [R] count(A + {c})
    cnt_a: np.ndarray       # int64 [R] count(A)
    cnt_c: np.ndarray       # int64 [R] count({c})
    support: np.ndarray     # float64 [R] cS / N
    conf: np.ndarray        # float64 [R] cS / cA
    lift: np.ndarray        # float64 [R] cS N / (cA cC)
    leverage: np.ndarray    # float64 [R] (cS N - cA cC) / N^2
    conviction: np.ndarray  # float64 [R] cA (N - cC) / (N (cA - cS)), +inf when cA == cS

    @property
    def n_rules(self) -> int:
        return int(self.cons.size)

    def antecedent(self, i: int) -> np.ndarray:
        return self.ante[self.ante_off[i]:self.ante_off[i + 1]]


@dataclass
class MultiRuleMeasures:
    """The exported rules with consequents of one or more items (AssociationRules.all_rules
    with max_consequent >= 2): every rule A -> B of every frequent S = A + B, without the cut,
    in the chosen order, with its three stored counts and five measures
    (csrc/host/fa_rule_measures.h with count(B) for count({c}); a one-item B's count is its
    occurrence count, a larger one's its line count)."""
    ante_off: np.ndarray    # int64 [R+1]
    ante: np.ndarray        # int32 concatenated antecedent ranks (ascending)
    cons_off: np.ndarray    # int64 [R+1]
    cons: np.ndarray        # int32 concatenated consequent ranks (ascending)
    cnt_s: np.ndarray       # int64 [R] count(A + B)
    cnt_a: np.ndarray       # int64 [R] count(A)
    cnt_c: np.ndarray       # int64 [R] count(B)
    support: np.ndarray     # float64 [R]
    conf: np.ndarray        # float64 [R]
    lift: np.ndarray        # float64 [R]
    leverage: np.ndarray    # float64 [R]
    conviction: np.ndarray  # float64 [R]

    @property
    def n_rules(self) -> int:
        return int(self.cnt_s.size)

    def antecedent(self, i: int) -> np.ndarray:
        return self.ante[self.ante_off[i]:self.ante_off[i + 1]]

    def consequent(self, i: int) -> np.ndarray:
        return self.cons[self.cons_off[i]:self.cons_off[i + 1]]


RULE_COUNT_MAX = 2 ** 31 - 1                                               # ... kRuleCountMax
RULE_SPLIT_MAX_K = 32        # fa_rule_splits.h kSplitMaxK: a split's position mask is one uint32
RULE_TPB = 256               # rules.hip kRuleTPB: elements per workgroup of the export


def rule_measures_plan(levels, counts, n_lines, min_confidence, min_lift, sort, limit) -> dict:
    """What both export paths (rule_measures here, ops.primitives.rule_measures_device) start
    from: the checked arguments and the levels in condense_marks' layout.

    Raises ValueError for an unknown line total (``n_lines <= 0``: a result reloaded from
    ``freqItems`` files), for a line total or a count above 2^31 - 1 (the measures' int64
    products are exact up to there) or below 1, and for bad options; RuntimeError
    (rules_not_closed) for rows above an empty level.  The levels end at the first empty one."""
    if sort not in RULE_SORTS:
        raise ValueError(f"all_rules: sort must be one of {', '.join(RULE_SORTS)}, not {sort!r}")
    if limit is not None and limit < 0:
        raise ValueError(f"all_rules: limit = {limit} is negative")
    n_lines = int(n_lines)
    if n_lines <= 0:
        raise ValueError("all_rules: the line total is unknown (n_lines = 0: a result loaded from freqItems files "
                         "carries none; a complete checkpoint does), so support, lift, leverage and conviction "
                         "are undefined")
    if n_lines > RULE_COUNT_MAX:
        raise ValueError(f"all_rules: {n_lines} lines exceed the limit of 2^31 - 1 = {RULE_COUNT_MAX} "
                         "(the measures' int64 products are exact up to there)")
    sizes = [len(c) for c in counts]
    bad = rules_gap_level([len(l) for l in levels])
    if bad:
        raise rules_not_closed(bad)
    K = 0
    while K < len(levels) and sizes[K] > 0:
        K += 1
    lv = [np.ascontiguousarray(levels[k], dtype=np.int32).reshape(-1) for k in range(K)]
    ct = [np.ascontiguousarray(counts[k], dtype=np.int64).reshape(-1) for k in range(K)]
    if any(l.size != c.size * (k + 1) for k, (l, c) in enumerate(zip(lv, ct))):
        raise ValueError("all_rules: levels[k-1] must be [n_k, k] with n_k counts")
    for c in ct:
        if c.size and (int(c.max()) > RULE_COUNT_MAX or int(c.min()) < 1):
            raise ValueError(f"all_rules: a count of {int(c.max()) if int(c.max()) > RULE_COUNT_MAX else int(c.min())} "
                             f"is outside 1 .. 2^31 - 1 = {RULE_COUNT_MAX} (the measures' int64 products are "
                             "exact up to there)")
    sizes = np.array(sizes[:K] or [0], dtype=np.int64)
    base = np.zeros(K + 2, dtype=np.int64)            # base[m]: element offset of the size-m level
    np.cumsum([l.size for l in lv], out=base[2:K + 2])
    cbase = np.zeros(K + 1, dtype=np.int64)           # cbase[m-1]: first row of the size-m level
    np.cumsum(sizes[:K], out=cbase[1:])
    eoff = np.zeros(K + 2, dtype=np.int64)            # eoff[k]: first (itemset, position) index of level k >= 2
    for k in range(2, K + 1):
        eoff[k + 1] = eoff[k] + int(sizes[k - 1]) * k
    return dict(K=K, sizes=sizes, base=base, cbase=cbase, eoff=eoff, n=int(cbase[K]), N=n_lines,
                rows=np.concatenate(lv) if lv else np.zeros(0, dtype=np.int32),
                cnts=np.concatenate(ct) if ct else np.zeros(0, dtype=np.int64),
                min_conf=float(min_confidence), has_lift=int(min_lift is not None),
                min_lift=float(min_lift) if min_lift is not None else 0.0, sort=RULE_SORTS.index(sort),
                limit=-1 if limit is None else int(limit))


def rule_measures(levels: list[np.ndarray], counts: list[np.ndarray], n_lines: int, tie_pos: np.ndarray,
                  min_confidence: float = 0.0, min_lift: float | None = None, sort: str = "confidence",
                  limit: int | None = None) -> RuleMeasures:
    """The rule export on the CPU (csrc/host/rules.cpp fa_rule_measures_cpu): selection,
    order and errors as ops.primitives.rule_measures_device; see rule_measures_plan."""
    m = rule_measures_plan(levels, counts, n_lines, min_confidence, min_lift, sort, limit)
    tie = np.ascontiguousarray(tie_pos, dtype=np.int64)
    if tie.size == 0:
        tie = np.zeros(1, dtype=np.int64)
    nr = np.zeros(1, dtype=np.int64)
    lib = _native.host()
    h = lib.fa_rule_measures_cpu(m["rows"].ctypes.data, m["base"].ctypes.data, m["cnts"].ctypes.data,
                                 m["cbase"].ctypes.data, m["K"], m["N"], m["min_conf"], m["has_lift"], m["min_lift"],
                                 m["sort"], m["limit"], tie.ctypes.data, num_threads(), nr.ctypes.data)
    R = int(nr[0])
    if R < 0:
        lib.fa_rule_measures_free(h)
        raise rules_not_closed(-R)
    na = int(lib.fa_rule_measures_nante(h))
    ante_off, ante, cons = np.zeros(R + 1, dtype=np.int64), np.zeros(na, dtype=np.int32), np.zeros(R, dtype=np.int32)
    ints = [np.zeros(R, dtype=np.int64) for _ in range(3)]
    flts = [np.zeros(R, dtype=np.float64) for _ in range(5)]
    lib.fa_rule_measures_export(h, *[a.ctypes.data for a in (ante_off, ante, cons, *ints, *flts)])
    lib.fa_rule_measures_free(h)
    return RuleMeasures(ante_off, ante, cons, *ints, *flts)


def rule_split_count(k: int, max_consequent: int) -> int:
    """n_k of csrc/host/fa_rule_splits.h from Python ints: the splits of one k-itemset."""
    return sum(math.comb(k, b) for b in range(1, min(max_consequent, k - 1) + 1))


def rule_splits_plan(levels, counts, n_lines, min_confidence, min_lift, sort, limit, max_consequent=1,
                     sizes=None) -> dict:
    """What both paths of the export with multi-item consequents (rule_splits here,
    ops.primitives.rule_splits_device) start from: rule_measures_plan's checks and layout,
    plus M = max_consequent (ValueError below 1; anything above K - 1 means every split), the
    level limit K <= 32 (ValueError) and eoff[k] = the first (itemset, split) element of level
    k with the element total at eoff[K + 1], from Python ints.  A total that needs 2^31 - 1
    workgroups of 256 or more raises ValueError before any native call.  ``sizes`` replaces
    the levels' row counts in that last check (a plan for a result that is not in memory)."""
    if int(max_consequent) < 1:
        raise ValueError(f"all_rules: max_consequent = {max_consequent} must be at least 1")

    def element_total(K, sz):
        if K > RULE_SPLIT_MAX_K:
            raise ValueError(f"all_rules: {K} levels exceed the limit of {RULE_SPLIT_MAX_K} on the max_consequent path "
                             "(a split's position mask is one 32-bit word)")
        M = max(1, min(int(max_consequent), K - 1))
        eoff = [0] * (K + 2)
        for k in range(2, K + 1):
            eoff[k + 1] = eoff[k] + int(sz[k - 1]) * rule_split_count(k, M)
        total = eoff[K + 1]
        if (total + RULE_TPB - 1) // RULE_TPB >= 2 ** 31 - 1:
            raise ValueError(f"all_rules: {total} (itemset, split) elements at max_consequent = {M} exceed the device "
                             f"grid of 2^31 - 2 workgroups of {RULE_TPB}: use a smaller --rules-max-consequent or mine "
                             "with --max-level")
        return M, eoff

    if sizes is not None:
        K = 0
        while K < len(sizes) and sizes[K] > 0:
            K += 1
        M, eoff = element_total(K, sizes)
        return dict(K=K, M=M, eoff=np.array(eoff, dtype=np.int64))
    m = rule_measures_plan(levels, counts, n_lines, min_confidence, min_lift, sort, limit)
    m["M"], eoff = element_total(m["K"], m["sizes"])
    m["eoff"] = np.array(eoff, dtype=np.int64)
    return m


def rule_splits(levels: list[np.ndarray], counts: list[np.ndarray], n_lines: int, tie_pos: np.ndarray,
                min_confidence: float = 0.0, min_lift: float | None = None, sort: str = "confidence",
                limit: int | None = None, max_consequent: int = 1) -> MultiRuleMeasures:
    """The rule export with consequents of up to ``max_consequent`` items on the CPU
    (csrc/host/rules.cpp fa_rule_splits_cpu): selection, order and errors as
    ops.primitives.rule_splits_device; see rule_splits_plan.  max_consequent = 1 gives
    rule_measures' rules with every consequent as a one-item list."""
    m = rule_splits_plan(levels, counts, n_lines, min_confidence, min_lift, sort, limit, max_consequent)
    tie = np.ascontiguousarray(tie_pos, dtype=np.int64)
    if tie.size == 0:
        tie = np.zeros(1, dtype=np.int64)
    nr = np.zeros(1, dtype=np.int64)
    lib = _native.host()
    h = lib.fa_rule_splits_cpu(m["rows"].ctypes.data, m["base"].ctypes.data, m["cnts"].ctypes.data,
                               m["cbase"].ctypes.data, m["K"], m["M"], m["N"], m["min_conf"], m["has_lift"],
                               m["min_lift"], m["sort"], m["limit"], tie.ctypes.data, num_threads(), nr.ctypes.data)
    R = int(nr[0])
    if R < 0:
        lib.fa_rule_splits_free(h)
        if R == -2 ** 63:
            raise RuntimeError("fa_rule_splits_cpu: the plan's limits do not hold")
        raise splits_not_closed(-R)
    na, nc = int(lib.fa_rule_splits_nante(h)), int(lib.fa_rule_splits_ncons(h))
    ante_off, ante = np.zeros(R + 1, dtype=np.int64), np.zeros(na, dtype=np.int32)
    cons_off, cons = np.zeros(R + 1, dtype=np.int64), np.zeros(nc, dtype=np.int32)
    ints = [np.zeros(R, dtype=np.int64) for _ in range(3)]
    flts = [np.zeros(R, dtype=np.float64) for _ in range(5)]
    lib.fa_rule_splits_export(h, *[a.ctypes.data for a in (ante_off, ante, cons_off, cons, *ints, *flts)])
    lib.fa_rule_splits_free(h)
    return MultiRuleMeasures(ante_off, ante, cons_off, cons, *ints, *flts)


def splits_not_closed(bad: int) -> RuntimeError:
    """The error of both paths of the export with multi-item consequents for a result whose
    level ``bad`` has an itemset with an antecedent or a consequent missing from its level."""
    return RuntimeError(f"rules: an itemset of size {bad} has a subset that is not in the level of its size "
                        "(the levels are not downward closed, or a level is not sorted)")


def rules_not_closed(bad: int) -> RuntimeError:
    """The error of both rule builders (this one and ops.primitives.rules_build_device) for a
    result whose level ``bad`` has an itemset with a subset missing from the level below."""
    return RuntimeError(f"rules: an itemset of size {bad} has a subset that is not in level {bad - 1} "
                        "(the levels are not downward closed, or a level is not sorted)")


def rules_gap_level(sizes) -> int:
    """The largest level with rows above an empty level (its subsets are missing), else 0."""
    return max((k for k in range(2, len(sizes) + 1) if sizes[k - 1] > 0 and sizes[k - 2] == 0), default=0)


def rules_build(levels: list[np.ndarray], counts: list[np.ndarray], tie_pos: np.ndarray) -> RuleTable:
    """Association rules on the CPU (csrc/host/rules.cpp), levels / counts as
    ops.primitives.rules_build_device.  The levels end at the first empty one (level_stats
    has no entry for it); a result that is not downward closed or not sorted (a level with
    rows above an empty one included) raises RuntimeError naming the level."""
    K = len(levels)
    lv = [np.ascontiguousarray(l, dtype=np.int32) for l in levels]
    ct = [np.ascontiguousarray(c, dtype=np.int64) for c in counts]
    rows_p = (C.c_void_p * max(K, 1))(*[l.ctypes.data for l in lv])
    cnt_p = (C.c_void_p * max(K, 1))(*[c.ctypes.data for c in ct])
    sizes = np.array([l.shape[0] for l in lv] or [0], dtype=np.int64)
    tie = np.ascontiguousarray(tie_pos, dtype=np.int64)
    if tie.size == 0:
        tie = np.zeros(1, dtype=np.int64)
    nr = np.zeros(1, dtype=np.int64)
    lib = _native.host()
    h = lib.fa_rules_build(C.cast(rows_p, C.c_void_p), C.cast(cnt_p, C.c_void_p), sizes.ctypes.data, K,
                           tie.ctypes.data, num_threads(), nr.ctypes.data)
    R = int(nr[0])
    if R < 0:
        lib.fa_rules_free(h)
        raise rules_not_closed(-R)
    na = int(lib.fa_rules_nante(h))
    ns = int(lib.fa_rules_nstats(h))
    ante_off = np.zeros(R + 1, dtype=np.int64)
    ante = np.zeros(max(na, 1), dtype=np.int32)
    cons = np.zeros(max(R, 1), dtype=np.int32)
    conf = np.zeros(max(R, 1), dtype=np.float64)
    stats = np.zeros(max(ns, 1), dtype=np.int64)
    lib.fa_rules_export(h, ante_off.ctypes.data, ante.ctypes.data, cons.ctypes.data, conf.ctypes.data,
                        stats.ctypes.data)
    lib.fa_rules_free(h)
    st = stats[:ns].reshape(-1, 3)
    level_stats = [(i + 1, int(b), int(a)) for i, (b, a, _) in enumerate(st.tolist())]
    level_ms = [us / 1e3 for _, _, us in st.tolist()]
    return RuleTable(ante_off, ante[:na], cons[:R], conf[:R], level_stats, level_ms)
