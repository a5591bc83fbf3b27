"""AssociationRules: rule generation, redundancy cut, ordering, recommendation.

Reference: AssociationRules.scala (class AssociationRules, :17-190).

  reference (Spark)                                  here
  -------------------------------------------------  -----------------------------------------------
  removeRedundancy: zipWithIndex, map to rank sets,  native parse of this rank's U.dat byte range,
    reduceByKey dedup, collectAsMap (:33-64)         LUT to ranks on the device (empty -> "0")
  genRules: linear scan for S - {s} (:122-145)       HIP subset index: one thread per (S, position)
                                                     binary-searches level k-1 (csrc/hip/rules.hip)
  cut, level by level (:147-182)                     HIP dense lookup of the child rule through the
                                                     subset index (no hash table, no broadcast)
  sortWith(conf desc, token.toInt) (:74, :116-120)   device stable sorts on a packed key; HIP emit
                                                     (CPU runs: the same in C++, csrc/host/rules.cpp)
  per-basket first-match scan (:80-106)              HIP: one wave per basket, 64 rules per step,
                                                     __ballot + ffs for the earliest match; big rule
                                                     tables scan only the per-item rule lists of the
                                                     basket's items (k_recommend_indexed)
  collect to driver + saveRecommends                 gather of rank ids to rank 0
  (none: the scan stops at the first match)          ranked top-N lists with confidences (run_topn):
                                                     HIP k_recommend_topn / k_recommend_topn_indexed
  (none: nothing is evaluated)                       leave-one-out hit rate / MRR / NDCG (evaluate):
                                                     HIP k_holdout_rank / k_holdout_rank_indexed
  (none: one rule decides)                           combine="sum" | "votes": every firing rule adds
                                                     its weight to its consequent, lists by the sums:
                                                     HIP k_recommend_combined / k_holdout_rank_combined

Divergences (documented): when there are no rules at all the reference throws
on ``rules.keys.min`` (:147); we recommend "0" for every user.  Non-integer
consequent tokens in a confidence tie would throw NumberFormatException there;
we order them after the integers by Java string order.
"""
from __future__ import annotations

import json
import math
from dataclasses import dataclass

import numpy as np
import torch

from .. import ops
from ..ops.host import MultiRuleMeasures, RuleMeasures, RuleTable, rule_measures, rule_splits, rules_build
from ..parallel.comm import Comm
from ..utils.jvm import rule_tiebreak_key
from ..utils.metrics import Logger
from .data import MiningResult, TransactionShard, Vocabulary, hash_tokens


@dataclass
class Evaluation:
    """Leave-one-out evaluation of the top-n recommender over a U.dat (AssociationRules.evaluate;
    the definitions are in docs/PARITY.md).  A trial hides one item of a basket of at least
    two items and ranks it in the top-n list of the rest; ``hits[r - 1]`` counts the trials of
    rank r.  The integers are summed over all ranks first, so the floats do not depend on the
    world size: sums over r ascending in float64, one division by ``n_trials`` at the end.
    ``combine``: how the lists were built (first | sum | votes)."""
    n: int
    n_lines: int
    n_lines_skipped: int           # lines with fewer than two frequent items: no trial
    n_trials: int
    n_infrequent_tokens: int       # occurrences of tokens that are no frequent item
    hits: list[int]
    hit_rate: list[float]          # hit_rate[k - 1]: trials of rank 1..k over all trials
    mrr: float
    ndcg: float
    combine: str = "first"

    @classmethod
    def from_counts(cls, n: int, n_lines: int, n_lines_skipped: int, n_trials: int, n_infrequent_tokens: int,
                    hits: list[int], combine: str = "first") -> "Evaluation":
        hits = [int(h) for h in hits]
        assert len(hits) == n
        cum, rr, dcg, acc = [], 0.0, 0.0, 0
        for r, h in enumerate(hits, 1):
            acc += h
            cum.append(acc)
            rr += h / r
            dcg += h / math.log2(r + 1)
        T = int(n_trials)
        if T == 0:
            rate, rr, dcg = [0.0] * n, 0.0, 0.0
        else:
            rate, rr, dcg = [c / T for c in cum], rr / T, dcg / T
        return cls(int(n), int(n_lines), int(n_lines_skipped), T, int(n_infrequent_tokens), hits, rate, rr, dcg,
                   combine)

    def as_json(self) -> str:
        """One JSON object, keys in field order, floats as Python repr; ``combine`` follows
        ``n`` and is written only when it is not ``first``."""
        keys = ("n",) + (("combine",) if self.combine != "first" else ()) + (
            "n_lines", "n_lines_skipped", "n_trials", "n_infrequent_tokens", "hits", "hit_rate", "mrr", "ndcg")
        return json.dumps({k: getattr(self, k) for k in keys})


class AssociationRules:
    def __init__(self, result: MiningResult, comm: Comm | None = None, logger: Logger | None = None,
                 device: torch.device | str | None = None):
        self.result = result
        self.comm = comm or Comm()
        self.log = logger or Logger(self.comm.rank)
        # rules are built where the job runs: the GPU kernels on a GPU rank, C++ on a CPU one
        self.device = torch.device(device) if device is not None else self.comm.device
        self._rules: RuleTable | None = None
        self._rules_dev = None
        self.use_index = True      # per-item rule lists for big rule tables (k_recommend_indexed)

    # ------------------------------------------------------------------
    def _tie_pos(self) -> np.ndarray:
        """Position of every rank's token in the consequent tiebreak order."""
        items = self.result.items
        order = sorted(range(len(items)), key=lambda r: rule_tiebreak_key(items[r]))
        tie_pos = np.empty(len(items), dtype=np.int64)
        tie_pos[np.asarray(order, dtype=np.int64)] = np.arange(len(items), dtype=np.int64)
        return tie_pos

    def rules(self) -> RuleTable:
        if self._rules is None:
            tie_pos = self._tie_pos()
            if self.device.type == "cuda":
                d = ops.primitives.rules_build_device(self.result.levels, self.result.counts, tie_pos, self.device)
                self._rules = RuleTable(d["ante_off"].cpu().numpy(), d["ante"].cpu().numpy(),
                                        d["cons"].cpu().numpy(), d["conf"].cpu().numpy(), d["level_stats"],
                                        d["level_ms"])
                self._rules_dev = (self.device, d["ante_off"], d["ante"], d["cons"])
            else:
                self._rules = rules_build(self.result.levels, self.result.counts, tie_pos)
            # the cut's log lines per antecedent size (AssociationRules.scala:155,177,181),
            # then the rule total (:75)
            ms = list(self._rules.level_ms) + [0.0] * len(self._rules.level_stats)
            for (size, before, after), t in zip(self._rules.level_stats[1:], ms[1:]):
                self.log.line(f"Before cut level {size} Nums: {before}")
                self.log.line(f"After cut level {size} Nums: {after}")
                self.log.line(f"Use Time cut leaves {size} Time: {int(t)}")
                self.log.metric(phase="rule_cut", level=size, before=before, after=after, ms=round(t, 3))
            self.log.line(f"Size association rules {self._rules.n_rules}")
        return self._rules

    def all_rules(self, min_confidence: float = 0.0, min_lift: float | None = None, sort: str = "confidence",
                  limit: int | None = None, max_consequent: int = 1) -> RuleMeasures | MultiRuleMeasures:
        """The rule export (an extension; the reference never shows its rules): EVERY rule
        A -> c with A + {c} frequent and at least two items -- the cut serves the recommender
        only and stays in rules() -- with support, confidence, lift, leverage and conviction
        (csrc/host/fa_rule_measures.h: exact int64 products of the stored counts, one fp64
        division; level-1 counts are occurrence counts, so with repeated tokens on a line
        count(c) can exceed the line total and leverage / conviction go negative).

        Kept: confidence >= min_confidence and, when given, lift >= min_lift (fp64, bounds
        inclusive).  Order: ``sort`` (confidence, lift, leverage, conviction or support)
        descending with +inf first, then confidence descending, the consequent's tie
        position, antecedent size, antecedent row; ``limit`` keeps that many rules.
        Takes the full mined result: a condensed one is not downward closed and raises
        RuntimeError, as any result with a subset missing from the level below; ValueError
        when the line total is unknown or it or a count exceeds 2^31 - 1.  A GPU rank
        runs ops.primitives.rule_measures_device, a CPU rank ops.host.rule_measures.

        ``max_consequent`` = M >= 2 splits every frequent S every way into A -> B with B of
        at most M items (anything above the deepest level - 1: every split) and returns
        MultiRuleMeasures: count(B) stands for count({c}) in the measures, and the order
        gains the consequent's size in front of its key (a larger consequent's key is its row
        in its level), so the one-item rules keep their relative order.  At most 32 levels;
        ValueError for M < 1, for more levels and for an element total past one device grid
        (docs/PARITY.md).  ops.primitives.rule_splits_device / ops.host.rule_splits."""
        r = self.result
        args = (min_confidence, min_lift, sort, limit)
        if int(max_consequent) < 1:
            raise ValueError(f"all_rules: max_consequent = {max_consequent} must be at least 1")
        if int(max_consequent) >= 2:
            if self.device.type == "cuda":
                d = ops.primitives.rule_splits_device(r.levels, r.counts, r.n_lines, self._tie_pos(), self.device,
                                                      *args, max_consequent)
                return MultiRuleMeasures(*[d[k].cpu().numpy() for k in (
                    "ante_off", "ante", "cons_off", "cons", "cnt_s", "cnt_a", "cnt_c", "support", "conf", "lift",
                    "leverage", "conviction")])
            return rule_splits(r.levels, r.counts, r.n_lines, self._tie_pos(), *args, max_consequent)
        if self.device.type == "cuda":
            d = ops.primitives.rule_measures_device(r.levels, r.counts, r.n_lines, self._tie_pos(), self.device, *args)
            return RuleMeasures(*[d[k].cpu().numpy() for k in ("ante_off", "ante", "cons", "cnt_s", "cnt_a", "cnt_c",
                                                               "support", "conf", "lift", "leverage", "conviction")])
        return rule_measures(r.levels, r.counts, r.n_lines, self._tie_pos(), *args)

    def rule_list(self) -> list[tuple[tuple[int, ...], int, float]]:
        rt = self.rules()
        return [(tuple(rt.antecedent(i).tolist()), int(rt.cons[i]), float(rt.conf[i]))
                for i in range(rt.n_rules)]

    # ------------------------------------------------------------------
    def _rank_lut(self, vocab: Vocabulary) -> np.ndarray:
        """User-shard id -> rank (-1 when the token is not a frequent item)."""
        lut = np.full(max(vocab.size, 1), -1, dtype=np.int32)
        if vocab.numeric:
            for r, t in enumerate(self.result.items):
                i = Vocabulary.numeric_id(t)
                if 0 <= i < vocab.size:
                    lut[i] = r
        elif vocab.size and self.result.items:
            # through the parser's 64-bit token hashes: no loop over the users' vocabulary
            rh = self.result.item_hashes
            if rh is None or len(rh) != len(self.result.items):
                rh = hash_tokens(self.result.items)     # e.g. results reloaded from files
            rh = np.asarray(rh, dtype=np.uint64)
            ro = np.argsort(rh)
            vh = vocab.hashes.astype(np.uint64)
            pos = np.minimum(np.searchsorted(rh[ro], vh), rh.size - 1)
            hit = rh[ro][pos] == vh
            lut[:vocab.size][hit] = ro[pos[hit]].astype(np.int32)
        return lut

    def _prepare_baskets(self, users: TransactionShard):
        """What a recommendation kernel needs for a (non-empty) user shard: (rule tensors
        on the users' device, per-item rule lists or None, F1, CSR of the baskets to
        scan, fan-out).  Identical baskets are scanned once (removeRedundancy's
        reduceByKey of the rank sets, AssociationRules.scala:51-58): baskets are
        canonicalised (ranks sorted), grouped by a 128-bit row hash, every group is
        verified equal to its representative element by element, and the CSR holds the
        representatives only; ``inv`` then maps every line to its representative's row
        (None: the CSR holds every line)."""
        rt = self.rules()
        dev = users.items.device
        lut = torch.from_numpy(self._rank_lut(users.vocab)).to(dev)
        n = users.n_lines
        F1 = len(self.result.items)
        r = lut[users.items.to(torch.int64)] if users.items.numel() else users.items
        keep = r >= 0
        lens = users.offsets[1:] - users.offsets[:-1]
        row = torch.repeat_interleave(torch.arange(n, device=dev), lens)
        rk, rr = row[keep], r[keep].to(torch.int64)
        # canonical basket = its ranks ascending (the basket is a set)
        key, _ = torch.sort(rk * max(F1, 1) + rr)
        bask = (key % max(F1, 1)).to(torch.int32).contiguous()
        bcnt = torch.bincount(rk, minlength=n)
        boff = torch.zeros(n + 1, dtype=torch.int64, device=dev)
        torch.cumsum(bcnt, 0, out=boff[1:])
        if self._rules_dev is None or self._rules_dev[0] != dev:
            self._rules_dev = (dev, torch.from_numpy(rt.ante_off).to(dev), torch.from_numpy(rt.ante).to(dev),
                               torch.from_numpy(rt.cons).to(dev))
        _, a_off, ante, cons = self._rules_dev[:4]
        index = None
        if dev.type == "cuda" and cons.numel() >= ops.primitives.RECOMMEND_INDEX_MIN_RULES and self.use_index:
            if len(self._rules_dev) == 4:
                self._rules_dev = self._rules_dev + (ops.primitives.recommend_index(a_off, ante, F1),)
            index = self._rules_dev[4]
        groups = self._basket_groups(boff, bask, bcnt) if (self.dedup_baskets and n > 1) else None
        if groups is None:
            self.stats["distinct_baskets"] = n
            return (a_off, ante, cons), index, F1, boff, bask, None
        rep, inv = groups
        self.stats["distinct_baskets"] = int(rep.numel())
        rcnt = bcnt[rep]
        roff = torch.zeros(rep.numel() + 1, dtype=torch.int64, device=dev)
        torch.cumsum(rcnt, 0, out=roff[1:])
        # gather the representatives' baskets into their own CSR
        pos = torch.repeat_interleave(boff[rep] - roff[:-1], rcnt) + torch.arange(int(roff[-1]), device=dev)
        rbask = bask[pos].contiguous()
        return (a_off, ante, cons), index, F1, roff, rbask, inv

    def recommend_shard(self, users: TransactionShard) -> torch.Tensor:
        """Recommended rank per local U.dat line (-1 = "0"), on the users' device.

        Identical baskets are recommended once (see _prepare_baskets) and the
        representatives' results fan out to all lines of their group.  Cost O(distinct
        baskets) instead of O(lines) in the first-match scan."""
        self.rules()
        if users.n_lines == 0:
            return torch.zeros(0, dtype=torch.int32, device=users.items.device)
        (a_off, ante, cons), index, F1, boff, bask, inv = self._prepare_baskets(users)
        rec = ops.recommend(a_off, ante, cons, F1, boff, bask, index=index)
        return rec if inv is None else rec[inv]

    def recommend_topn_shard(self, users: TransactionShard, n: int) -> torch.Tensor:
        """Ranked top-n per local U.dat line: int32 [n_lines, n] rule ids (-1 padded) on
        the users' device, see ops.recommend_topn.  The item of an entry is
        ``rules().cons[id]``, its confidence ``rules().conf[id]``.  Baskets are
        de-duplicated and the kernel chosen as in recommend_shard."""
        if not 1 <= n <= 64:
            raise ValueError(f"recommend_topn_shard: n = {n} is outside 1..64")
        self.rules()
        if users.n_lines == 0:
            return torch.zeros((0, n), dtype=torch.int32, device=users.items.device)
        (a_off, ante, cons), index, F1, boff, bask, inv = self._prepare_baskets(users)
        top = ops.recommend_topn(a_off, ante, cons, F1, boff, bask, n, index=index)
        return top if inv is None else top[inv]

    def _combine_args(self, combine: str, dev, index, a_off, ante, F1):
        """(weights on ``dev``, per-item rule lists) for ops.*_combined: the weights come from
        ops.combine_weights, once per mode, and a device always gets the lists (the combined
        kernels have no scan form)."""
        if not hasattr(self, "_weights"):
            self._weights = {}
        if (combine, dev) not in self._weights:
            self._weights[(combine, dev)] = ops.combine_weights(self.rules().conf, combine).to(dev)
        if index is None and dev.type == "cuda" and self.rules().n_rules:
            if len(self._rules_dev) == 4:
                self._rules_dev = self._rules_dev + (ops.primitives.recommend_index(a_off, ante, F1),)
            index = self._rules_dev[4]
        return self._weights[(combine, dev)], index

    def recommend_combined_shard(self, users: TransactionShard, n: int, combine: str):
        """Combined scoring per local U.dat line (``combine``: sum | votes; docs/PARITY.md):
        (rule int32 [n_lines, n], score int64 [n_lines, n]) on the users' device, see
        ops.recommend_combined.  An entry's item is ``rules().cons[rule]``, its score the sum of
        the weights of every firing rule with that consequent.  Baskets are de-duplicated as in
        recommend_shard."""
        if not 1 <= n <= 64:
            raise ValueError(f"recommend_combined_shard: n = {n} is outside 1..64")
        if combine not in ("sum", "votes"):
            raise ValueError(f"recommend_combined_shard: combine = {combine!r} is not 'sum' or 'votes'")
        self.rules()
        dev = users.items.device
        if users.n_lines == 0:
            return torch.zeros((0, n), dtype=torch.int32, device=dev), torch.zeros((0, n), dtype=torch.int64, device=dev)
        (a_off, ante, cons), index, F1, boff, bask, inv = self._prepare_baskets(users)
        weight, index = self._combine_args(combine, dev, index, a_off, ante, F1)
        rule, score = ops.recommend_combined(a_off, ante, cons, weight, F1, boff, bask, n, index=index)
        return (rule, score) if inv is None else (rule[inv], score[inv])

    def _holdout(self, users: TransactionShard, n: int, combine: str = "first"):
        """(boff, bask, ranks) of the local lines: the CSR of their baskets (ranks ascending)
        and the leave-one-out rank of every element (ops.holdout_rank, or with ``combine``
        sum | votes ops.holdout_rank_combined), on the users' device."""
        if not 1 <= n <= 64:
            raise ValueError(f"holdout_ranks_shard: n = {n} is outside 1..64")
        if combine not in ops.primitives.COMBINE_MODES:
            raise ValueError(f"holdout_ranks_shard: combine = {combine!r} is not one of first, sum, votes")
        self.rules()
        dev = users.items.device
        if users.n_lines == 0:
            return (torch.zeros(1, dtype=torch.int64, device=dev), torch.zeros(0, dtype=torch.int32, device=dev),
                    torch.zeros(0, dtype=torch.int32, device=dev))
        (a_off, ante, cons), index, F1, boff, bask, inv = self._prepare_baskets(users)
        if combine == "first":
            ranks = ops.holdout_rank(a_off, ante, cons, F1, boff, bask, n, index=index)
        else:
            weight, index = self._combine_args(combine, dev, index, a_off, ante, F1)
            ranks = ops.holdout_rank_combined(a_off, ante, cons, weight, F1, boff, bask, n, index=index)
        if inv is None:
            return boff, bask, ranks
        # every line takes the elements of its representative
        cnt = (boff[1:] - boff[:-1])[inv]
        loff = torch.zeros(inv.numel() + 1, dtype=torch.int64, device=dev)
        torch.cumsum(cnt, 0, out=loff[1:])
        pos = torch.repeat_interleave(boff[inv] - loff[:-1], cnt) + torch.arange(int(loff[-1]), device=dev)
        return loff, bask[pos].contiguous(), ranks[pos].contiguous()

    def holdout_ranks_shard(self, users: TransactionShard, n: int,
                            combine: str = "first") -> tuple[torch.Tensor, torch.Tensor]:
        """Leave-one-out ranks of the local U.dat lines: (boff int64 [lines + 1], ranks int32
        [nnz]) on the users' device.  Line i's basket (its distinct frequent items, ranks
        ascending) is elements boff[i] .. boff[i + 1]; an element's rank is the 1-based
        position of that item in the top-n list of the basket without it, 0 for a miss (and
        for a one-item basket).  ``combine`` sum | votes ranks it in the combined list
        (recommend_combined_shard) instead.  Baskets are de-duplicated and the kernel chosen as
        in recommend_shard."""
        boff, _, ranks = self._holdout(users, n, combine)
        return boff, ranks

    def run_evaluate(self, users: TransactionShard, n: int, rank_lines: bool = False, combine: str = "first"):
        """(Evaluation on every rank, the per-line rank file on rank 0 or None): with
        ``rank_lines`` one line per U.dat line, ``token:rank`` for every item of its basket
        in rank order joined by one space, "0" for an empty basket.  ``combine``: the lists the
        hidden items are ranked in (first | sum | votes)."""
        ops.primitives.reset_fallbacks()
        boff, bask, ranks = self._holdout(users, n, combine)
        if ops.primitives.FALLBACKS:
            self.stats["fallbacks"] = list(ops.primitives.FALLBACKS)
            for f in ops.primitives.FALLBACKS:
                self.log.metric(phase="fallback", what=f, stage="evaluate")
        dev = boff.device
        cnt = boff[1:] - boff[:-1]
        # a trial is an element of a basket of at least two items; the others rank 0
        hist = torch.bincount(ranks.to(torch.int64), minlength=n + 1)[1:n + 1]
        lut = torch.from_numpy(self._rank_lut(users.vocab)).to(dev)
        n_infreq = int((lut[users.items.to(torch.int64)] < 0).sum()) if users.items.numel() else 0
        extras = np.asarray(users.extras).astype(np.int64)
        if extras.size:
            n_infreq += int((lut.cpu().numpy()[extras] < 0).sum())
        tail = torch.stack([cnt.new_tensor(users.n_lines), (cnt < 2).sum(), cnt[cnt >= 2].sum(),
                            cnt.new_tensor(n_infreq)])
        vec = torch.cat([hist, tail]).to(torch.int64)
        vec = self.comm.all_reduce_(vec).tolist()
        ev = Evaluation.from_counts(n, vec[n], vec[n + 1], vec[n + 2], vec[n + 3], vec[:n], combine)
        if not rank_lines:
            return ev, None
        parts = [self.comm.gather_varlen(t) for t in (cnt, bask, ranks)]
        if parts[0] is None:
            return ev, None
        items, out = self.result.items, []
        for c, b, r in zip(*parts):
            b, r, o = b.tolist(), r.tolist(), 0
            for k in c.tolist():
                out.append(" ".join(f"{items[b[i]]}:{r[i]}" for i in range(o, o + k)) if k else "0")
                o += k
        return ev, out

    def evaluate(self, users: TransactionShard, n: int, combine: str = "first") -> Evaluation:
        """Leave-one-out evaluation of the top-n recommender on U.dat's own baskets (an
        extension; docs/PARITY.md): hit rate@1..n, MRR and NDCG over all trials of all ranks'
        lines, identical on every rank (one all-reduce of the n + 4 integers).  ``combine``
        sum | votes evaluates the combined lists."""
        return self.run_evaluate(users, n, combine=combine)[0]

    dedup_baskets = True

    @property
    def stats(self) -> dict:
        if not hasattr(self, "_stats"):
            self._stats = {}
        return self._stats

    @staticmethod
    def _basket_groups(boff: torch.Tensor, bask: torch.Tensor, bcnt: torch.Tensor):
        """(representative basket per group, group of every basket), or None when
        dedup does not pay (few repeats) or a hash group fails the exact check."""
        n = bcnt.numel()
        h1, h2 = ops.row_hash(boff, bask)
        # empty baskets hash alike: give them a key of their own (length is part of it)
        key = torch.stack([h1, h2 ^ bcnt.to(torch.int64)], dim=1)
        uk, inv = torch.unique(key, dim=0, return_inverse=True)
        G = uk.shape[0]
        if G > 0.9 * n:
            return None
        first = torch.full((G,), n, dtype=torch.int64, device=bask.device)
        first.scatter_reduce_(0, inv, torch.arange(n, device=bask.device), reduce="amin")
        # exact check: every basket equals its group's representative
        rep_of = first[inv]
        if not torch.equal(bcnt, bcnt[rep_of]):
            return None
        if bask.numel():
            row = torch.repeat_interleave(torch.arange(n, device=bask.device), bcnt)
            j = torch.arange(bask.numel(), device=bask.device) - boff[row]
            if not torch.equal(bask, bask[boff[rep_of][row] + j]):
                return None
        return first, inv

    def run(self, users: TransactionShard) -> list[str] | None:
        """Recommendations for every U.dat line, in file order, on rank 0 (None elsewhere)."""
        ops.primitives.reset_fallbacks()     # the rules phase reports its own fallbacks
        rec = self.recommend_shard(users)
        if ops.primitives.FALLBACKS:
            self.stats["fallbacks"] = list(ops.primitives.FALLBACKS)
            for f in ops.primitives.FALLBACKS:
                self.log.metric(phase="fallback", what=f, stage="rules")
        parts = self.comm.gather_varlen(rec)
        if parts is None:
            return None
        items = self.result.items
        out = []
        for p in parts:
            out.extend("0" if v < 0 else items[v] for v in p.tolist())
        return out

    def run_topn(self, users: TransactionShard, n: int, scores: bool = False,
                 combine: str = "first") -> list[str] | None:
        """Ranked top-n for every U.dat line, in file order, on rank 0 (None elsewhere): the
        items' tokens in list order joined by one space, "0" for an empty list.  With
        ``scores`` every entry is ``token:conf``, conf the repr() of the rule's float64
        confidence (the score is what follows the last ':').

        ``combine`` sum | votes: the combined lists (recommend_combined_shard) instead; with
        ``scores`` an entry is ``token:repr(S / 2**32)`` for sum (the summed confidences; the
        division of Python ints is correctly rounded) and ``token:S`` (an integer) for votes."""
        if combine not in ops.primitives.COMBINE_MODES:
            raise ValueError(f"run_topn: combine = {combine!r} is not one of first, sum, votes")
        if combine != "first":
            return self._run_topn_combined(users, n, scores, combine)
        ops.primitives.reset_fallbacks()
        top = self.recommend_topn_shard(users, n)
        if ops.primitives.FALLBACKS:
            self.stats["fallbacks"] = list(ops.primitives.FALLBACKS)
            for f in ops.primitives.FALLBACKS:
                self.log.metric(phase="fallback", what=f, stage="rules")
        parts = self.comm.gather_varlen(top.reshape(-1))
        if parts is None:
            return None
        rt, items = self.rules(), self.result.items
        cons, conf = rt.cons.tolist(), rt.conf.tolist()
        out = []
        for p in parts:
            for ids in p.reshape(-1, n).tolist():
                if scores:
                    ent = [f"{items[cons[i]]}:{conf[i]!r}" for i in ids if i >= 0]
                else:
                    ent = [items[cons[i]] for i in ids if i >= 0]
                out.append(" ".join(ent) if ent else "0")
        return out

    def _run_topn_combined(self, users: TransactionShard, n: int, scores: bool, combine: str) -> list[str] | None:
        ops.primitives.reset_fallbacks()
        rule, score = self.recommend_combined_shard(users, n, combine)
        if ops.primitives.FALLBACKS:
            self.stats["fallbacks"] = list(ops.primitives.FALLBACKS)
            for f in ops.primitives.FALLBACKS:
                self.log.metric(phase="fallback", what=f, stage="rules")
        # both gathers run on every rank; the scores travel as int64
        rparts = self.comm.gather_varlen(rule.reshape(-1))
        sparts = self.comm.gather_varlen(score.reshape(-1))
        if rparts is None:
            return None
        items, cons = self.result.items, self.rules().cons.tolist()
        out = []
        for rp, sp in zip(rparts, sparts):
            for ids, sc in zip(rp.reshape(-1, n).tolist(), sp.reshape(-1, n).tolist()):
                if not scores:
                    ent = [items[cons[i]] for i in ids if i >= 0]
                elif combine == "sum":
                    ent = [f"{items[cons[i]]}:{v / 2 ** 32!r}" for i, v in zip(ids, sc) if i >= 0]
                else:
                    ent = [f"{items[cons[i]]}:{v}" for i, v in zip(ids, sc) if i >= 0]
                out.append(" ".join(ent) if ent else "0")
        return out
