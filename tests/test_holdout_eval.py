"""Leave-one-out evaluation (--evaluate) on the CPU path: ops.holdout_rank on a rule table whose
every rank is worked out by hand, the composition from recommend_topn on a mined case,
AssociationRules.evaluate / holdout_ranks_shard against the brute-force oracle, the command
line and the reduction across ranks."""
import functools
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from fastapriori_amd.models.apriori import FastApriori, MinerConfig
from fastapriori_amd.models.oracle import OracleResult, holdout_ranks, run_oracle
from fastapriori_amd.models.rules import AssociationRules, Evaluation
from fastapriori_amd.ops import primitives as prim
from fastapriori_amd.parallel.comm import Comm
from fastapriori_amd.parallel.launch import spawn_local
from fastapriori_amd.utils.io import generate_shard, parse_bytes
from fastapriori_amd.utils.jvm import java_split_ws
from fastapriori_amd.utils.metrics import Logger

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = ["n", "n_lines", "n_lines_skipped", "n_trials", "n_infrequent_tokens", "hits", "hit_rate", "mrr", "ndcg"]


# ---------------------------------------------------------------------------
# helpers shared with test_gpu_holdout_eval.py
# ---------------------------------------------------------------------------
def rules_tensors(rules, dev="cpu"):
    """[(antecedent ascending, consequent)] -> (ante_off int64, ante int32, cons int32) on dev."""
    off = np.zeros(len(rules) + 1, np.int64)
    np.cumsum([len(a) for a, _ in rules], out=off[1:])
    ante = np.array([x for a, _ in rules for x in a], np.int32)
    cons = np.array([c for _, c in rules], np.int32)
    return tuple(torch.from_numpy(x).to(dev) for x in (off, ante, cons))


def csr_tensors(baskets, dev="cpu"):
    boff = np.zeros(len(baskets) + 1, np.int64)
    np.cumsum([len(b) for b in baskets], out=boff[1:])
    bask = np.array([x for b in baskets for x in b], np.int32)
    return torch.from_numpy(boff).to(dev), torch.from_numpy(bask).to(dev)


def brute_ranks(rules, baskets, n):
    """The definition over Python sets: per element of the CSR the place of the hidden item in
    the first n firing rules with distinct consequents of the basket without it, or 0."""
    out = []
    for b in baskets:
        for h in b:
            rest, seen, rank = set(b) - {h}, [], 0
            for ante, c in rules:
                if len(seen) == n or not rest:
                    break
                if c not in rest and c not in seen and set(ante) <= rest:
                    seen.append(c)
                    if c == h:
                        rank = len(seen)
                        break
            out.append(rank)
    return out


HAND_F1 = 70


@functools.lru_cache(maxsize=None)
def hand_table():
    """(rules, baskets, place of every trial's hidden item in the unbounded list, 0 = never).
    A trial's rank for a given n is its place when that is at most n, else 0.

    With item 0 alone left in the basket the consequents come in the order 1, 2, 3, 4, 5,
    6 .. 69 (rules 1, 2, 3, 7, 8, 9 .. 72), so item c stands at place c."""
    rules = [((1,), 2),          # 0
             ((0,), 1),          # 1
             ((0,), 2),          # 2
             ((0,), 3),          # 3
             ((0,), 2),          # 4: consequent 2 again
             ((0,), 1),          # 5: consequent 1 again
             ((0, 2), 4),        # 6
             ((0,), 4),          # 7
             ((0,), 5)]          # 8
    rules += [((0,), c) for c in range(6, HAND_F1)]          # 9 .. 72
    cases = [
        # {0, 1}.  hide 0: rule 0 fires, item 0 is nobody's consequent.  hide 1: rule 0 has the hidden
        # item in its antecedent and would otherwise come first; rule 1 gives item 1 at place 1
        ([0, 1], [0, 1]),
        # {1, 2}.  hide 1: nothing fires on {2}.  hide 2: the consequent of rule 0
        ([1, 2], [0, 1]),
        # {0, 3}.  hide 3: behind consequents 1 and 2 (a miss for n <= 2); rules 4 and 5 repeat them after
        ([0, 3], [0, 3]),
        # {0, 2}.  hide 2: behind consequent 1 only: rank n for n = 2, a miss for n = 1
        ([0, 2], [0, 2]),
        # {0, 1, 3}.  hide 0: rule 0 fires on {1, 3}.  hide 1: rule 0 out, rule 1 -> 1.  hide 3: rule 0 -> 2,
        # rule 1's consequent 1 is another basket item, rule 2's is taken, rule 3 -> 3 at place 2
        ([0, 1, 3], [0, 1, 2]),
        # {0, 4}.  hide 4: 1, 2, 3, then rules 4 and 5 repeat consequents before item 4's rule 7: place 4
        ([0, 4], [0, 4]),
        # {0, 2, 5}.  hide 2: rule 1 -> 1, rule 2 -> 2.  hide 5: 1, (2 in the basket), 3, rule 6 -> 4,
        # rule 7 repeats 4, rule 8 -> 5 at place 4
        ([0, 2, 5], [0, 2, 4]),
        ([0], [0]),              # one item: nothing is left to fire a rule
        ([], []),                # empty basket: no trial
        ([0, 65], [0, 65]),      # behind 64 other consequents: a miss even for n = 64
        ([0, 64], [0, 64]),      # behind exactly 63: rank 64
    ]
    assert len({c for _, c in rules}) >= 65
    return rules, [b for b, _ in cases], [p for _, ps in cases for p in ps]


def hand_want(n):
    return [p if p <= n else 0 for p in hand_table()[2]]


@functools.lru_cache(maxsize=None)
def mined_case():
    """The mined case of test_gpu_recommend_topn.py: (result, users, CPU rules, (rule tensors, F1,
    basket CSR of every line))."""
    sh = generate_shard(20000, Comm(), "cpu", 8.0, 3.0, 80, 100, seed=9)
    res = FastApriori(0.01, config=MinerConfig(min_support=0.01), logger=Logger(enabled=False)).run(sh)
    users = generate_shard(3000, Comm(), "cpu", 8.0, 3.0, 80, 100, seed=9, users=True)
    ar = AssociationRules(res, logger=Logger(enabled=False))
    ar.dedup_baskets = False
    rules, _, F1, boff, bask, inv = ar._prepare_baskets(users)
    assert inv is None
    return res, users, ar, (rules, F1, boff, bask)


@functools.lru_cache(maxsize=None)
def composed(n):
    """The ranks from the parts that existed before: one explicit basket B - {h} per trial,
    recommend_topn over all of them, then the place of h in its list.  -> (ranks int32 [nnz],
    trials with no firing rule, misses behind a full list), the two masks over all elements."""
    _, _, _, ((a_off, ante, cons), F1, boff, bask) = mined_case()
    bo, bk = boff.tolist(), bask.tolist()
    rest = [[x for x in bk[bo[u]:bo[u + 1]] if x != h] for u in range(len(bo) - 1) for h in bk[bo[u]:bo[u + 1]]]
    toff, tbask = csr_tensors(rest)
    top = prim.recommend_topn(a_off, ante, cons, F1, toff, tbask, n)
    item = torch.where(top >= 0, cons[top.clamp(min=0).to(torch.int64)], torch.full_like(top, -1))
    at = item == bask[:, None]
    ranks = torch.where(at.any(1), at.to(torch.int32).argmax(1).to(torch.int32) + 1, torch.zeros((), dtype=torch.int32))
    return ranks.to(torch.int32), top[:, 0] < 0, (top[:, n - 1] >= 0) & (ranks == 0)


def metrics(n, hits, T):
    """The issue's formulas: sums over r ascending in float64, one division by T at the end."""
    if T == 0:
        return [0.0] * n, 0.0, 0.0
    acc, rate, rr, dcg = 0, [], 0.0, 0.0
    for r in range(1, n + 1):
        acc += hits[r - 1]
        rate.append(acc / T)
        rr += hits[r - 1] / r
        dcg += hits[r - 1] / math.log2(r + 1)
    return rate, rr / T, dcg / T


def oracle_evaluation(res, ulines, n):
    """(Evaluation fields as a dict in key order, rank-file lines) from oracle.holdout_ranks."""
    rank = set(res.items)
    per = holdout_ranks(res, ulines, n)
    trials = [r for line in per if len(line) >= 2 for _, r in line]
    assert all(r == 0 for line in per if len(line) < 2 for _, r in line)
    hits = [trials.count(r) for r in range(1, n + 1)]
    rate, mrr, ndcg = metrics(n, hits, len(trials))
    d = dict(n=n, n_lines=len(ulines), n_lines_skipped=sum(len(line) < 2 for line in per), n_trials=len(trials),
             n_infrequent_tokens=sum(t not in rank for toks in ulines for t in toks), hits=hits, hit_rate=rate,
             mrr=mrr, ndcg=ndcg)
    return d, [" ".join(f"{t}:{r}" for t, r in line) if line else "0" for line in per]


def _oracle_from(res) -> OracleResult:
    return OracleResult(items=res.items, counts1=res.counts[0].tolist(), itemsets=res.as_dict(),
                        min_count=res.min_count, n_lines=res.n_lines)


def _text(rows):
    return "\n".join(" ".join(r) for r in rows) + "\n"


# ---------------------------------------------------------------------------
# ops.holdout_rank
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 64])
def test_hand_table(native, n):
    rules, baskets, place = hand_table()
    want = hand_want(n)
    assert want == brute_ranks(rules, baskets, n)              # the hand's work, checked by the definition
    assert n in want and 0 in want
    boff, bask = csr_tensors(baskets)
    got = prim.holdout_rank(*rules_tensors(rules), HAND_F1, boff, bask, n)
    assert got.dtype == torch.int32 and tuple(got.shape) == (len(place),)
    assert got.tolist() == want


def test_no_rules_no_trials_and_bad_n(native):
    rules, baskets, place = hand_table()
    boff, bask = csr_tensors(baskets)
    none = (torch.zeros(1, dtype=torch.int64), torch.zeros(0, dtype=torch.int32), torch.zeros(0, dtype=torch.int32))
    assert prim.holdout_rank(*none, HAND_F1, boff, bask, 3).tolist() == [0] * len(place)          # R = 0
    got = prim.holdout_rank(*rules_tensors(rules), HAND_F1, *csr_tensors([[], []]), 3)            # nnz = 0
    assert got.dtype == torch.int32 and got.numel() == 0
    for n in (0, 65, -1):
        with pytest.raises(ValueError):
            prim.holdout_rank(*rules_tensors(rules), HAND_F1, boff, bask, n)


@pytest.mark.parametrize("n", [1, 3, 10])
def test_mined_case_equals_the_composition(native, n):
    _, _, _, ((a_off, ante, cons), F1, boff, bask) = mined_case()
    # at the ops level every element of the CSR is a trial (a one-item basket's is a miss)
    assert cons.numel() == 4681 and F1 == 73 and bask.numel() == 7247
    ref, nofire, full_miss = composed(n)
    # the spread the comparison needs: every rank, misses behind a full list, trials where nothing fires
    hist = torch.bincount(ref.to(torch.int64), minlength=n + 1).tolist()
    assert all(h > 0 for h in hist) and int(nofire.sum()) > 0 and int(full_miss.sum()) > 0
    if n == 10:
        assert hist == [3349, 1023, 728, 522, 441, 306, 243, 185, 174, 160, 116]
        assert int(nofire.sum()) == 851 and int(full_miss.sum()) == 2433
    got = prim.holdout_rank(a_off, ante, cons, F1, boff, bask, n)
    assert torch.equal(got, ref)


# ---------------------------------------------------------------------------
# AssociationRules.evaluate / holdout_ranks_shard against the oracle
# ---------------------------------------------------------------------------
def _small():
    rng = np.random.default_rng(5)
    drows = [" ".join(map(str, rng.choice(12, size=rng.integers(1, 6), replace=False))) for _ in range(400)]
    res = FastApriori(0.05, config=MinerConfig(min_support=0.05),
                      logger=Logger(enabled=False)).run(parse_bytes(("\n".join(drows) + "\n").encode()))
    pool = [[1, 2], [3], [2, 4, 5], [], [7, 1], [11, 10, 3], [1, 2, 3, 4, 5, 6], [40, 41], [2, 99, 4]]
    urows = []
    for _ in range(300):
        b = list(pool[rng.integers(len(pool))])
        rng.shuffle(b)
        urows.append(" ".join(map(str, b + b[:1])))          # shuffled, with a repeated token
    for _ in range(60):
        urows.append(" ".join(map(str, rng.choice(14, size=rng.integers(0, 7), replace=False))))
    return res, urows


@pytest.mark.parametrize("n", [1, 3, 64])
def test_evaluate_matches_oracle_with_and_without_dedup(native, n):
    res, urows = _small()
    users = parse_bytes(("\n".join(urows) + "\n").encode())
    want, want_lines = oracle_evaluation(_oracle_from(res), [java_split_ws(r) for r in urows], n)
    assert want["n_trials"] > 0 and want["n_lines_skipped"] > 0 and want["n_infrequent_tokens"] > 0
    assert sum(want["hits"]) > 0 and sum(want["hits"]) < want["n_trials"]
    outs = []
    for dedup in (True, False):
        ar = AssociationRules(res, logger=Logger(enabled=False))
        ar.dedup_baskets = dedup
        ev = ar.evaluate(users, n)
        assert isinstance(ev, Evaluation)
        assert {k: getattr(ev, k) for k in KEYS} == want           # every integer and every float, exactly
        assert list(json.loads(ev.as_json())) == KEYS and json.loads(ev.as_json()) == want
        boff, ranks = ar.holdout_ranks_shard(users, n)
        assert boff.dtype == torch.int64 and ranks.dtype == torch.int32 and boff.numel() == len(urows) + 1
        flat = [int(e.rsplit(":", 1)[1]) for l in want_lines if l != "0" for e in l.split(" ")]
        assert ranks.tolist() == flat
        assert torch.diff(boff).tolist() == [0 if l == "0" else l.count(" ") + 1 for l in want_lines]
        ev2, lines = ar.run_evaluate(users, n, rank_lines=True)
        assert lines == want_lines and ev2 == ev
        outs.append((ev.as_json(), lines, ar.stats["distinct_baskets"]))
    assert outs[0][:2] == outs[1][:2] and outs[0][2] < outs[1][2] == len(urows)


def test_as_json_is_repr_floats_in_key_order():
    ev = Evaluation.from_counts(3, 5, 1, 7, 2, [1, 2, 0])
    rate, mrr, ndcg = metrics(3, [1, 2, 0], 7)
    assert ev.as_json() == ('{"n": 3, "n_lines": 5, "n_lines_skipped": 1, "n_trials": 7, "n_infrequent_tokens": 2, '
                            f'"hits": [1, 2, 0], "hit_rate": [{rate[0]!r}, {rate[1]!r}, {rate[2]!r}], '
                            f'"mrr": {mrr!r}, "ndcg": {ndcg!r}}}')
    zero = Evaluation.from_counts(2, 0, 0, 0, 0, [0, 0])
    assert (zero.hit_rate, zero.mrr, zero.ndcg) == ([0.0, 0.0], 0.0, 0.0)


def test_empty_and_infrequent_users(native):
    res, _ = _small()
    ar = AssociationRules(res, logger=Logger(enabled=False))
    ev = ar.evaluate(parse_bytes(b""), 4)
    assert {k: getattr(ev, k) for k in KEYS} == dict(n=4, n_lines=0, n_lines_skipped=0, n_trials=0,
                                                     n_infrequent_tokens=0, hits=[0] * 4, hit_rate=[0.0] * 4,
                                                     mrr=0.0, ndcg=0.0)
    boff, ranks = ar.holdout_ranks_shard(parse_bytes(b""), 4)
    assert boff.tolist() == [0] and ranks.numel() == 0 and ranks.dtype == torch.int32
    # no token of U.dat is a frequent item
    ev, lines = ar.run_evaluate(parse_bytes(b"77 78\n\n79 77 77\n"), 4, rank_lines=True)
    # occurrences: 77 three times, and the blank line is one (empty) token, as for D.dat
    assert (ev.n_lines, ev.n_lines_skipped, ev.n_trials, ev.n_infrequent_tokens) == (3, 3, 0, 6)
    want, _ = oracle_evaluation(_oracle_from(res), [java_split_ws(l) for l in ["77 78", "", "79 77 77"]], 4)
    assert {k: getattr(ev, k) for k in KEYS} == want
    assert ev.hits == [0] * 4 and ev.mrr == 0.0 and lines == ["0", "0", "0"]
    for n in (0, 65):
        with pytest.raises(ValueError):
            ar.evaluate(parse_bytes(b"1 2\n"), n)
    # no rules at all
    none = AssociationRules(FastApriori(0.5).run(parse_bytes(b"1\n1\n2\n2\n")), logger=Logger(enabled=False))
    assert none.rules().n_rules == 0
    ev = none.evaluate(parse_bytes(b"1 2\n1\n"), 2)
    assert (ev.n_trials, ev.n_lines_skipped, ev.hits) == (2, 1, [0, 0])


def test_evaluation_is_exported():
    import fastapriori_amd
    assert fastapriori_amd.Evaluation is Evaluation


# ---------------------------------------------------------------------------
# command line
# ---------------------------------------------------------------------------
D = "1 2 3\n1 2 4\n2 3 4\n1 2 4\n2 4\n4 5\n1 2\n"
U = "1\n2\n7 8\n2 4\n4 1 2\n3\n1\n\n2 4 9 9\n"


def _cli(tmp_path, out, *flags):
    env = dict(os.environ, PYTHONPATH=ROOT)
    return subprocess.run([sys.executable, "-m", "fastapriori_amd", f"{tmp_path}/", f"{tmp_path}/{out}",
                           f"{tmp_path}/tmp", "--min-support", "0.25", "--device", "cpu", *flags],
                          capture_output=True, text=True, env=env, timeout=300)


def _oracle_files(n):
    _, _, res = run_oracle(D.splitlines(), U.splitlines(), 0.25)
    d, lines = oracle_evaluation(res, [java_split_ws(l) for l in U.splitlines()], n)
    return json.dumps(d) + "\n", "\n".join(lines) + "\n"


@pytest.fixture(scope="module")
def cli_runs(tmp_path_factory):
    """One job without the flag (a_), one with both flags (b_), then --rules-only from b's checkpoint."""
    d = tmp_path_factory.mktemp("evaluate")
    (d / "D.dat").write_text(D)
    (d / "U.dat").write_text(U)
    runs = {"a": _cli(d, "a_"), "b": _cli(d, "b_", "--evaluate", "2", "--evaluate-ranks", "--overwrite")}
    os.rename(d / "b_evaluation", d / "b_first")
    os.rename(d / "b_evaluationRanks", d / "b_firstRanks")
    runs["c"] = _cli(d, "b_", "--rules-only", "--evaluate", "2", "--evaluate-ranks", "--overwrite")
    return d, runs


def test_cli_writes_both_files(cli_runs):
    d, runs = cli_runs
    assert all(r.returncode == 0 for r in runs.values()), [r.stderr for r in runs.values()]
    want_json, want_ranks = _oracle_files(2)
    ev = json.loads(want_json)
    assert ev["n_trials"] > 0 and sum(ev["hits"]) > 0 and ev["n_infrequent_tokens"] == 5 and ev["n_lines"] == 9
    assert "0" in want_ranks.splitlines() and any(l.endswith(":0") and " " not in l for l in want_ranks.splitlines())
    assert (d / "b_first" / "part-00000").read_text() == want_json
    assert (d / "b_firstRanks" / "part-00000").read_text() == want_ranks
    assert (d / "b_first" / "_SUCCESS").exists()
    assert "Total time for get evaluation" in runs["b"].stdout
    assert runs["b"].stdout.index("Total time for get recommends") < runs["b"].stdout.index("Total time for get evaluation")
    # the other outputs do not change with the flag, and without it nothing of it appears
    assert (d / "a_recommends" / "part-00000").read_bytes() == (d / "b_recommends" / "part-00000").read_bytes()
    assert not (d / "a_evaluation").exists() and not (d / "a_evaluationRanks").exists()
    assert "evaluation" not in runs["a"].stdout


def test_cli_rules_only_reproduces_the_files(cli_runs):
    d, _ = cli_runs
    for first, again in (("b_first", "b_evaluation"), ("b_firstRanks", "b_evaluationRanks")):
        assert (d / first / "part-00000").read_bytes() == (d / again / "part-00000").read_bytes()


@pytest.mark.parametrize("flags", [("--evaluate", "65"), ("--evaluate", "-1"), ("--evaluate-ranks",),
                                   ("--evaluate", "3", "--count-itemsets", "q.txt", "--count-only"),
                                   ("--evaluate", "3", "--evaluate-ranks", "--count-itemsets", "q.txt", "--count-only")])
def test_cli_rejects_bad_flags(flags):
    from fastapriori_amd.config import parse_args
    with pytest.raises(SystemExit) as e:
        parse_args(["in/", "out/", *flags])
    assert e.value.code == 2                                   # argparse's usage error
    cfg = parse_args(["in/", "out/", "--evaluate", "64", "--evaluate-ranks"])
    assert cfg.evaluate == 64 and cfg.evaluate_ranks
    off = parse_args(["in/", "out/"])
    assert off.evaluate == 0 and not off.evaluate_ranks


def test_summary_and_metric(tmp_path):
    from fastapriori_amd.config import JobConfig
    from fastapriori_amd.pipeline import run_job
    (tmp_path / "D.dat").write_text(D)
    (tmp_path / "U.dat").write_text(U)
    mpath = str(tmp_path / "metrics.jsonl")
    s = run_job(JobConfig(input=f"{tmp_path}/", output=f"{tmp_path}/o_", min_support=0.25, device="cpu", evaluate=2,
                          metrics_path=mpath), Comm())
    ev = json.loads(_oracle_files(2)[0])
    assert (s["evaluate_n"], s["n_trials"], s["hit_rate_at_n"], s["mrr"]) == (2, ev["n_trials"], ev["hit_rate"][-1],
                                                                             ev["mrr"])
    assert not (tmp_path / "o_evaluationRanks").exists()
    recs = [json.loads(l) for l in open(mpath)]
    m = [r for r in recs if r.get("phase") == "evaluate"]
    assert len(m) == 1 and all(m[0][k] == ev[k] for k in KEYS[:6])
    s0 = run_job(JobConfig(input=f"{tmp_path}/", output=f"{tmp_path}/p_", min_support=0.25, device="cpu"), Comm())
    assert not {"evaluate_n", "n_trials", "hit_rate_at_n", "mrr"} & set(s0)
    assert not (tmp_path / "p_evaluation").exists()


# ---------------------------------------------------------------------------
# across ranks (gloo)
# ---------------------------------------------------------------------------
def _evaluate_files(path_prefix: str, ms: float, n: int):
    from fastapriori_amd.parallel.comm import init_comm, shutdown_comm
    from fastapriori_amd.utils.io import read_shard

    comm = init_comm("cpu")
    try:
        shard = read_shard(path_prefix + "D.dat", comm)
        res = FastApriori(ms, comm, MinerConfig(trim_min_rows=0, min_support=ms),
                          Logger(comm.rank, enabled=False)).run(shard)
        users = read_shard(path_prefix + "U.dat", comm)
        ev, lines = AssociationRules(res, comm, Logger(comm.rank, enabled=False)).run_evaluate(users, n, rank_lines=True)
        return ev.as_json(), lines
    finally:
        shutdown_comm(comm)


def test_world_size_two_gives_the_same_files(tmp_path):
    from fastapriori_amd.utils.io import write_quest_file
    write_quest_file(str(tmp_path / "D.dat"), 2000, 8.0, 3.0, 60, 50, seed=2)
    write_quest_file(str(tmp_path / "U.dat"), 301, 8.0, 3.0, 60, 50, seed=2, users=True)
    ref = spawn_local(_evaluate_files, 1, f"{tmp_path}/", 0.02, 3)[0]
    outs = spawn_local(_evaluate_files, 2, f"{tmp_path}/", 0.02, 3)
    assert outs[0] == ref and outs[1] == (ref[0], None)       # the metrics on every rank, the lines on rank 0
    ev = json.loads(ref[0])
    assert ev["n_lines"] == 301 == len(ref[1]) and all(h > 0 for h in ev["hits"]) and ev["n_trials"] > sum(ev["hits"])
