"""Job configuration: CLI > environment (FA_*) > defaults.

The environment can set the product settings a batch scheduler typically fixes per
job: FA_MIN_SUPPORT, FA_DEVICE, FA_STRATEGY, FA_PROFILE and FA_METRICS; everything
else is a command-line flag.  Internal tuning knobs are not here: see tuning.py
(one FA_TUNE variable for experiments) and docs/ARCHITECTURE.md ("Configuration").

Positional arguments keep the reference's semantics (Main.scala:24-25,
Utils.scala:21-23,39,48): ``input`` and ``output`` are string PREFIXES —
``input + "D.dat"``, ``output + "freqItemset"`` — so directories need a
trailing slash; ``temp`` is the checkpoint location (ignored by the reference).
"""
from __future__ import annotations

import argparse
import os
from dataclasses import dataclass, field


def _env(name: str, default):
    v = os.environ.get(name)
    if v is None:
        return default
    if isinstance(default, bool):
        return v.lower() in ("1", "true", "yes", "on")
    return type(default)(v)


# every FA_* variable the package reads (config / tuning / env / checkpoint / comm / build)
KNOWN_ENV = frozenset({"FA_MIN_SUPPORT", "FA_DEVICE", "FA_STRATEGY", "FA_PROFILE", "FA_METRICS", "FA_TUNE",
                       "FA_NUM_THREADS", "FA_DIST_BACKEND", "FA_FORCE_PG", "FA_FAULT_AT_LEVEL", "FA_FAULT_RANK",
                       "FA_HIP_LIB"})
# variables of earlier versions that are no longer read, with what replaced them (ADVICE r5:
# a job script still setting one would otherwise run with the default, silently)
RETIRED_ENV = {"FA_DEDUP": "--dedup", "FA_MAX_LEVEL": "--max-level", "FA_RESUME": "--resume",
               "FA_WITH_COUNTS": "--with-counts", "FA_WORLD_SIZE": "--world-size",
               "FA_DL_MULTI": "FA_TUNE=dl_multi=0|1", "FA_BUCKET_MB": "FA_TUNE=bucket_mb=<MiB>",
               "FA_FUSED_LAYOUT": "FA_TUNE=fused_layout=0|1"}
_WARNED = False


def unread_env(environ=None) -> list[str]:
    """Warnings for FA_* variables set in the environment that nothing reads."""
    environ = os.environ if environ is None else environ
    out = []
    for k in sorted(environ):
        if not k.startswith("FA_") or k in KNOWN_ENV:
            continue
        hint = RETIRED_ENV.get(k)
        out.append(f"{k} is no longer read" + (f": use {hint}" if hint else " (unknown FA_* variable)"))
    return out


def warn_unread_env() -> None:
    """Print unread_env()'s warnings once per process (stderr)."""
    global _WARNED
    if _WARNED:
        return
    _WARNED = True
    import sys
    for w in unread_env():
        print(f"fastapriori: warning: {w}", file=sys.stderr)


@dataclass
class JobConfig:
    input: str = ""
    output: str = ""
    temp: str = ""
    min_support: float = 0.092                  # Main.scala:23
    device: str = "auto"                        # auto | cuda | cpu
    dedup: str = "auto"
    pair_strategy: str = "auto"
    with_counts: bool = False                   # also write <out>freqItems ("a b[cnt]", Utils.scala:51-63)
    resume: bool = False
    rules_only: bool = False
    checkpoint: bool = True
    overwrite: bool = False
    profile: bool = False
    metrics_path: str | None = None
    max_level: int = 0
    strategy: str = "count"                     # count | candidate distribution
    world_size: int = 0                         # 0: whatever torchrun started; N: launch / require N ranks
    tiebreak: str = "string"                    # rank order of equal-count items (utils.jvm.item_tiebreak_key)
    top_n: int = 0                              # > 0: also write <out>recommendsTopN (ranked lists, 1..64 items)
    top_n_scores: bool = False                  # ... every entry as token:confidence
    closed: bool = False                        # also write <out>closedItemset ("a b[cnt]": no superset of equal count)
    maximal: bool = False                       # also write <out>maximalItemset ("a b[cnt]": no frequent superset)
    rules: bool = False                         # also write <out>rules (every rule with its measures, no cut)
    min_confidence: float = 0.0                 # ... keeping confidence >= this
    min_lift: float | None = None               # ... and lift >= this
    rules_sort: str = "confidence"              # ... ordered by this measure, descending
    rules_limit: int | None = None              # ... the first K only
    rules_max_consequent: int = 1               # ... with consequents of up to M items (1: A -> c only)
    count_itemsets: str | None = None           # query file: also write <out>itemsetCounts ("a b[cnt]" per query line)
    count_only: bool = False                    # ... and end there: no mining, no U.dat, no checkpoint
    verify_counts: bool = False                 # recount every mined itemset of >= 2 items over D.dat and compare
    evaluate: int = 0                           # > 0: also write <out>evaluation (leave-one-out metrics of the top-N lists)
    evaluate_ranks: bool = False                # ... and <out>evaluationRanks (token:rank per U.dat line)
    combine: str = "first"                      # first | sum | votes: how --top-n and --evaluate build a list
    extra: dict = field(default_factory=dict)


def build_parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(
        prog="python -m fastapriori_amd",
        description="MI355X-native FastApriori: frequent itemsets + association-rule recommendations")
    p.add_argument("input", help="input prefix: reads <input>D.dat and <input>U.dat")
    p.add_argument("output", help="output prefix: writes <output>freqItemset/ and <output>recommends/")
    p.add_argument("temp", nargs="?", default="", help="temporary path (per-level checkpoints)")
    p.add_argument("--min-support", type=float, default=_env("FA_MIN_SUPPORT", 0.092))
    p.add_argument("--device", choices=["auto", "cuda", "cpu"], default=_env("FA_DEVICE", "auto"))
    p.add_argument("--dedup", choices=["auto", "on", "off"], default="auto")
    p.add_argument("--pair-strategy", choices=["auto", "horizontal", "gram"],
                   default="auto")
    p.add_argument("--with-counts", action="store_true")
    p.add_argument("--resume", action="store_true")
    p.add_argument("--rules-only", action="store_true")
    p.add_argument("--no-checkpoint", dest="checkpoint", action="store_false", default=True)
    p.add_argument("--overwrite", action="store_true")
    p.add_argument("--profile", action="store_true", default=_env("FA_PROFILE", False))
    p.add_argument("--metrics", dest="metrics_path", default=os.environ.get("FA_METRICS"))
    p.add_argument("--max-level", type=int, default=0)
    p.add_argument("--strategy", choices=["count", "candidate"], default=_env("FA_STRATEGY", "count"),
                   help="count: shard transactions, all-reduce counts; candidate: replicate the DB on every "
                        "rank and split pairs by rows, level candidates by rank")
    p.add_argument("--world-size", type=int, default=0,
                   help="number of ranks (one per GPU). Without a torchrun environment the job "
                        "re-launches itself under torch.distributed.run; under torchrun the process "
                        "group must have exactly this many ranks")
    p.add_argument("--tiebreak", choices=["string", "numeric"], default="string",
                   help="order of frequent items with equal counts (it orders the tokens inside an itemset "
                        "line; the reference's Spark order is not reproducible): string = java.lang.String "
                        "order, numeric = integer tokens by value first")
    p.add_argument("--top-n", type=int, default=0, metavar="N",
                   help="also write <output>recommendsTopN/: per U.dat line the first N (1..64) firing rules' "
                        "consequents with distinct items, in rule order, or 0 when none fires")
    p.add_argument("--top-n-scores", action="store_true",
                   help="with --top-n: write every entry as token:confidence")
    p.add_argument("--closed", action="store_true",
                   help="also write <output>closedItemset/: the frequent itemsets with no proper superset of the "
                        "same count, as 'a b c[count]' lines (lossless: an itemset's count is the largest among "
                        "its closed supersets). With --max-level L: closed among the itemsets of at most L items")
    p.add_argument("--maximal", action="store_true",
                   help="also write <output>maximalItemset/: the frequent itemsets with no frequent proper superset, "
                        "as 'a b c[count]' lines. With --max-level L: maximal among the itemsets of at most L items "
                        "(every level-L itemset is written)")
    p.add_argument("--rules", action="store_true",
                   help="also write <output>rules/: every rule 'A -> c' with A + {c} frequent (no redundancy cut), one "
                        "per line, tab-separated: antecedent tokens, consequent, count(A+c), count(A), count(c), "
                        "support, confidence, lift, leverage, conviction. Needs the full result and the line total "
                        "(with --rules-only: a complete checkpoint)")
    p.add_argument("--min-confidence", type=float, default=None, metavar="F",
                   help="with --rules: keep rules with confidence >= F (default 0)")
    p.add_argument("--min-lift", type=float, default=None, metavar="F", help="with --rules: also require lift >= F")
    p.add_argument("--rules-sort", choices=list(RULE_SORTS), default=None,
                   help="with --rules: the measure the file is ordered by, descending (default confidence)")
    p.add_argument("--rules-limit", type=int, default=None, metavar="K", help="with --rules: the first K rules only")
    p.add_argument("--rules-max-consequent", type=int, default=None, metavar="M",
                   help="with --rules: also split every frequent itemset into 'A -> B' with B of up to M items "
                        "(default 1: one-item consequents only; anything above the deepest level - 1 means every "
                        "split). Field 2 then holds B's tokens one space apart, count(c) is count(B)")
    p.add_argument("--count-itemsets", metavar="PATH", default=None,
                   help="also write <output>itemsetCounts/: for every line of the query file PATH (tokenised as a "
                        "D.dat line; a blank line is the empty token) the number of D.dat lines that contain all of "
                        "its tokens, as 'a b c[count]' with the line's distinct tokens in first-occurrence order. A "
                        "line count: a token repeated inside a D.dat line counts once")
    p.add_argument("--count-only", action="store_true",
                   help="with --count-itemsets: read D.dat, count, write and end (no mining, no U.dat, no checkpoint)")
    p.add_argument("--verify-counts", action="store_true",
                   help="after mining, recount every mined itemset of two or more items over D.dat with the query "
                        "counter, which shares nothing with the miner, and fail on the first difference")
    p.add_argument("--evaluate", type=int, default=0, metavar="N",
                   help="also write <output>evaluation/: leave-one-out evaluation of the top-N (1..64) recommender on "
                        "U.dat itself, one JSON line: every item of every basket of two or more frequent items is "
                        "hidden in turn and ranked in the top-N list of the rest; hit rate@1..N, MRR and NDCG")
    p.add_argument("--evaluate-ranks", action="store_true",
                   help="with --evaluate: also write <output>evaluationRanks/: per U.dat line token:rank for every "
                        "frequent item of the line (0 = not in the list), or 0 when the line has none")
    p.add_argument("--combine", choices=["first", "sum", "votes"], default="first",
                   help="with --top-n / --evaluate: how a list is built. first: an item stands where its best firing "
                        "rule does. sum: every firing rule adds its confidence to its consequent, votes: it adds 1; the "
                        "items are listed by their sums, ties by their best rule. recommends/ is not affected")
    return p


# --rules-sort's choices; a measure's position is its code in csrc/host/fa_rule_measures.h (RuleSort)
RULE_SORTS = ("confidence", "lift", "leverage", "conviction", "support")


def parse_args(argv=None) -> JobConfig:
    p = build_parser()
    a = p.parse_args(argv)
    if a.top_n != 0 and not 1 <= a.top_n <= 64:
        p.error(f"--top-n {a.top_n}: N must be in 1..64")
    if a.top_n_scores and not a.top_n:
        p.error("--top-n-scores requires --top-n")
    for flag, v in (("--min-confidence", a.min_confidence), ("--min-lift", a.min_lift),
                    ("--rules-sort", a.rules_sort), ("--rules-limit", a.rules_limit),
                    ("--rules-max-consequent", a.rules_max_consequent)):
        if v is not None and not a.rules:
            p.error(f"{flag} requires --rules")
    if a.rules_limit is not None and a.rules_limit < 0:
        p.error(f"--rules-limit {a.rules_limit}: K must not be negative")
    if a.rules_max_consequent is not None and a.rules_max_consequent < 1:
        p.error(f"--rules-max-consequent {a.rules_max_consequent}: M must be at least 1")
    if a.count_only and not a.count_itemsets:
        p.error("--count-only requires --count-itemsets")
    for flag, on in (("--count-itemsets", a.count_itemsets), ("--count-only", a.count_only),
                     ("--verify-counts", a.verify_counts)):
        if on and a.rules_only:
            p.error(f"{flag} cannot be combined with --rules-only (there is no database to count over)")
    if a.evaluate != 0 and not 1 <= a.evaluate <= 64:
        p.error(f"--evaluate {a.evaluate}: N must be in 1..64")
    if a.evaluate_ranks and not a.evaluate:
        p.error("--evaluate-ranks requires --evaluate")
    for flag, on in (("--evaluate", a.evaluate), ("--evaluate-ranks", a.evaluate_ranks)):
        if on and a.count_only:
            p.error(f"{flag} cannot be combined with --count-only (nothing is mined)")
    if a.combine != "first" and not (a.top_n or a.evaluate):
        p.error(f"--combine {a.combine} requires --top-n or --evaluate")
    if a.verify_counts and a.count_only:
        p.error("--verify-counts cannot be combined with --count-only (nothing is mined)")
    warn_unread_env()
    return JobConfig(input=a.input, output=a.output, temp=a.temp, min_support=a.min_support, device=a.device,
                     dedup=a.dedup, pair_strategy=a.pair_strategy, with_counts=a.with_counts, resume=a.resume,
                     rules_only=a.rules_only, checkpoint=a.checkpoint, overwrite=a.overwrite,
                     profile=a.profile, metrics_path=a.metrics_path, max_level=a.max_level,
                     strategy=a.strategy, world_size=a.world_size, tiebreak=a.tiebreak, top_n=a.top_n,
                     top_n_scores=a.top_n_scores, closed=a.closed, maximal=a.maximal, rules=a.rules,
                     min_confidence=0.0 if a.min_confidence is None else a.min_confidence, min_lift=a.min_lift,
                     rules_sort=a.rules_sort or "confidence", rules_limit=a.rules_limit,
                     rules_max_consequent=a.rules_max_consequent or 1,
                     count_itemsets=a.count_itemsets, count_only=a.count_only, verify_counts=a.verify_counts,
                     evaluate=a.evaluate, evaluate_ranks=a.evaluate_ranks, combine=a.combine)
