"""Combined scoring (--combine sum | votes) on the CPU path: ops.recommend_combined and
ops.holdout_rank_combined on a table worked out by hand and against a brute-force helper, the
model against the oracle on the mined case of test_holdout_eval.py, the printed lines, the
evaluation, the command line and the reduction across ranks."""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from fastapriori_amd.models.oracle import holdout_ranks_combined, recommend_combined, recommend_topn, run_oracle
from fastapriori_amd.models.rules import AssociationRules, Evaluation
from fastapriori_amd.ops import primitives as prim
from fastapriori_amd.parallel.launch import spawn_local
from fastapriori_amd.utils.io import parse_bytes
from fastapriori_amd.utils.jvm import java_split_ws
from fastapriori_amd.utils.metrics import Logger
from test_holdout_eval import D, KEYS, U, _oracle_from, _small, csr_tensors, metrics, mined_case, rules_tensors

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODES = ("sum", "votes")


# ---------------------------------------------------------------------------
# helpers shared with test_gpu_recommend_combined.py
# ---------------------------------------------------------------------------
def brute_list(rules, weights, basket):
    """The definition over Python sets and ints: [(consequent, S, f)] of the basket, S descending
    then f ascending, uncut."""
    b, S, f = set(basket), {}, {}
    for r, (ante, c) in enumerate(rules):
        if b and c not in b and set(ante) <= b:
            S[c] = S.get(c, 0) + int(weights[r])
            f.setdefault(c, r)
    return sorted(((c, S[c], f[c]) for c in S), key=lambda t: (-t[1], t[2]))


def brute_combined(rules, weights, baskets, n):
    """(rule rows, score rows), padded with -1 / 0 to n entries."""
    lists = [brute_list(rules, weights, b)[:n] for b in baskets]
    return ([[f for _, _, f in l] + [-1] * (n - len(l)) for l in lists],
            [[s for _, s, _ in l] + [0] * (n - len(l)) for l in lists])


def brute_places(rules, weights, baskets, n):
    """Per element of the CSR the place of the hidden item in the list of the basket without it."""
    out = []
    for b in baskets:
        for h in b:
            order = [c for c, _, _ in brute_list(rules, weights, set(b) - {h})[:n]]
            out.append(order.index(h) + 1 if h in order else 0)
    return out


def weight_tensor(weights, dev="cpu"):
    return torch.tensor([int(w) for w in weights], dtype=torch.int64).to(dev)


def shard_lines(users):
    """The token lists of a shard's lines."""
    off, items = users.offsets.tolist(), users.items.tolist()
    return [[users.vocab.token(i) for i in items[off[l]:off[l + 1]]] for l in range(len(off) - 1)]


def format_combined(lists, mode, scores):
    """The file format: entries joined by one space, "0" for an empty list; a score is
    repr(S / 2**32) for sum and the integer for votes."""
    def ent(t, s):
        if not scores:
            return t
        return f"{t}:{s / 2 ** 32!r}" if mode == "sum" else f"{t}:{s}"
    return [" ".join(ent(t, s) for t, s in l) if l else "0" for l in lists]


def oracle_evaluation_combined(res, ulines, n, mode):
    """(Evaluation fields as a dict in as_json's key order, rank-file lines) from
    oracle.holdout_ranks_combined and the formulas of test_holdout_eval.metrics."""
    rank = set(res.items)
    per = holdout_ranks_combined(res, ulines, n, mode)
    trials = [r for line in per if len(line) >= 2 for _, r in line]
    assert all(r == 0 for line in per if len(line) < 2 for _, r in line)
    hits = [trials.count(r) for r in range(1, n + 1)]
    rate, mrr, ndcg = metrics(n, hits, len(trials))
    d = dict(n=n, combine=mode, n_lines=len(ulines), n_lines_skipped=sum(len(line) < 2 for line in per),
             n_trials=len(trials), n_infrequent_tokens=sum(t not in rank for toks in ulines for t in toks), hits=hits,
             hit_rate=rate, mrr=mrr, ndcg=ndcg)
    return d, [" ".join(f"{t}:{r}" for t, r in line) if line else "0" for line in per]


# ---------------------------------------------------------------------------
# ops: the hand-built table
# ---------------------------------------------------------------------------
HAND_F1 = 6
HAND_RULES = [((0,), 2),        # 0  w 5
              ((1,), 3),        # 1  w 4
              ((0,), 3),        # 2  w 3
              ((0, 1), 2),      # 3  w 1
              ((1,), 4),        # 4  w 6
              ((0,), 4),        # 5  w 1
              ((2,), 0)]        # 6  w 7
HAND_W = [5, 4, 3, 1, 6, 1, 7]
# basket -> (its uncut list as (f, S), the place of every hidden item in the uncut list, 0 = never)
HAND_CASES = [
    # {0, 1}: all of rules 0..5 fire.  S(2) = 5 + 1, S(3) = 4 + 3, S(4) = 6 + 1: items 3 and 4 tie at 7 and
    # item 3's first rule (1) comes before item 4's (4); first-match order would be 2, 3, 4.
    # hide 0: rules 1 and 4 fire, nothing names 0.  hide 1: 1 is nobody's consequent
    ([0, 1], [(1, 7), (4, 7), (0, 6)], [0, 0]),
    # {0}: rules 0, 2, 5.  One item: no trial
    ([0], [(0, 5), (2, 3), (5, 1)], [0]),
    # {0, 2}: rule 0's and rule 6's consequents are in the basket.  hide 0: rule 6 fires on {2}.  hide 2: on
    # {0} item 2 leads with 5
    ([0, 2], [(2, 3), (5, 1)], [1, 1]),
    # {0, 1, 4}.  hide 4: the list of {0, 1}, item 4 second.  hide 0 / 1: not a consequent of what fires
    ([0, 1, 4], [(1, 7), (0, 6)], [0, 0, 2]),
    # {0, 1, 2}.  hide 0: on {1, 2} S(0) = 7 beats S(4) = 6 and S(3) = 4.  hide 2: third in {0, 1}'s list
    ([0, 1, 2], [(1, 7), (4, 7)], [1, 0, 3]),
    ([], [], []),
    ([5], [], [0]),
]


@pytest.mark.parametrize("n", [1, 2, 3, 64])
def test_hand_table(native, n):
    baskets = [b for b, _, _ in HAND_CASES]
    want_rule = [[f for f, _ in l[:n]] + [-1] * (n - len(l[:n])) for _, l, _ in HAND_CASES]
    want_score = [[s for _, s in l[:n]] + [0] * (n - len(l[:n])) for _, l, _ in HAND_CASES]
    want_place = [p if p <= n else 0 for _, _, ps in HAND_CASES for p in ps]
    # the hand's work, checked by the definition
    assert (want_rule, want_score) == brute_combined(HAND_RULES, HAND_W, baskets, n)
    assert want_place == brute_places(HAND_RULES, HAND_W, baskets, n)
    boff, bask = csr_tensors(baskets)
    rule, score = prim.recommend_combined(*rules_tensors(HAND_RULES), weight_tensor(HAND_W), HAND_F1, boff, bask, n)
    assert rule.dtype == torch.int32 and score.dtype == torch.int64
    assert tuple(rule.shape) == tuple(score.shape) == (len(baskets), n)
    assert rule.tolist() == want_rule and score.tolist() == want_score
    place = prim.holdout_rank_combined(*rules_tensors(HAND_RULES), weight_tensor(HAND_W), HAND_F1, boff, bask, n)
    assert place.dtype == torch.int32 and place.tolist() == want_place


def test_no_rules_no_baskets_and_bad_n(native):
    baskets = [b for b, _, _ in HAND_CASES]
    boff, bask = csr_tensors(baskets)
    none = (torch.zeros(1, dtype=torch.int64), torch.zeros(0, dtype=torch.int32), torch.zeros(0, dtype=torch.int32))
    w0 = torch.zeros(0, dtype=torch.int64)
    rule, score = prim.recommend_combined(*none, w0, HAND_F1, boff, bask, 3)                       # R = 0
    assert rule.tolist() == [[-1] * 3] * len(baskets) and score.tolist() == [[0] * 3] * len(baskets)
    assert prim.holdout_rank_combined(*none, w0, HAND_F1, boff, bask, 3).tolist() == [0] * bask.numel()
    rule, score = prim.recommend_combined(*rules_tensors(HAND_RULES), weight_tensor(HAND_W), HAND_F1,
                                          *csr_tensors([]), 3)                                  # M = 0
    assert tuple(rule.shape) == (0, 3) and tuple(score.shape) == (0, 3)
    for n in (0, 65, -1):
        for fn in (prim.recommend_combined, prim.holdout_rank_combined):
            with pytest.raises(ValueError):
                fn(*rules_tensors(HAND_RULES), weight_tensor(HAND_W), HAND_F1, boff, bask, n)


def test_combine_weights():
    conf = np.array([1.0, 0.5, 1 / 3, 0.02563, 2.0 ** -32])
    w = prim.combine_weights(conf, "sum")
    assert w.dtype == torch.int64 and w.tolist() == [2 ** 32, 2 ** 31, 1431655765, int(0.02563 * 2 ** 32), 1]
    assert prim.combine_weights(conf, "votes").tolist() == [1] * 5
    assert prim.combine_weights(np.zeros(0), "sum").numel() == 0
    for bad in ("first", "mean"):
        with pytest.raises(ValueError):
            prim.combine_weights(conf, bad)
    with pytest.raises(ValueError):
        prim.combine_weights(np.array([2.0 ** -33]), "sum")           # a weight of 0 would not count as firing


def random_table(R, F1, sizes, seed, wmax=1 << 32):
    """(rules, weights, baskets): antecedents of 1..3 items, few distinct weights so that sums tie;
    a basket is filled with whole rules (antecedent + consequent) and single items."""
    rng = np.random.default_rng(9100 + 131 * R + F1 + 17 * sum(sizes) + seed)
    rules = []
    for _ in range(R):
        it = rng.choice(F1, 1 + min(F1 - 1, int(rng.integers(1, 4))), replace=False)
        rules.append((tuple(sorted(it[1:].tolist())), int(it[0])))
    pool = [1, 2, wmax - 1, wmax]
    weights = [pool[int(rng.integers(len(pool)))] for _ in range(R)]
    baskets = []
    for s in sizes:
        b = []
        while len(b) < min(s, F1):
            fits = [r for r in rng.permutation(R)[:32].tolist() if len(set((*rules[r][0], rules[r][1], *b))) <= s]
            if fits and rng.random() < 0.8:
                new = [x for x in (*rules[fits[0]][0], rules[fits[0]][1]) if x not in b]
            else:
                new = [x for x in [int(rng.integers(F1))] if x not in b]
            b += new
        baskets.append(sorted(b))
    return rules, weights, baskets


@pytest.mark.parametrize("R,F1", [(1, 2), (40, 7), (300, 12), (700, 40)])
def test_cpu_equals_brute_force_on_random_tables(native, R, F1):
    rules, weights, baskets = random_table(R, F1, (1, 2, 3, 4, 5, 6, 2, 3, 0, 7), seed=R)
    boff, bask = csr_tensors(baskets)
    some_hit = False
    for n in (1, 2, 5, 64):
        rule, score = prim.recommend_combined(*rules_tensors(rules), weight_tensor(weights), F1, boff, bask, n)
        assert (rule.tolist(), score.tolist()) == brute_combined(rules, weights, baskets, n)
        place = prim.holdout_rank_combined(*rules_tensors(rules), weight_tensor(weights), F1, boff, bask, n)
        assert place.tolist() == brute_places(rules, weights, baskets, n)
        some_hit = some_hit or any(place.tolist())
    assert some_hit or R == 1


# ---------------------------------------------------------------------------
# the model against the oracle on the mined case
# ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _mined_oracle(mode):
    """The oracle's uncut-enough lists (n = 64: no basket of the case has more than 61 firing
    consequents) and, per n, what the oracle returns is its prefix -- checked below for n = 3."""
    res, users, _, _ = mined_case()
    return recommend_combined(_oracle_from(res), shard_lines(users), 64, mode)


@pytest.mark.parametrize("mode", MODES)
def test_mined_case_equals_the_oracle(native, mode):
    res, users, _, _ = mined_case()
    ulines = shard_lines(users)
    full = _mined_oracle(mode)
    assert max(len(l) for l in full) == 61                   # below 64: n = 64 cuts nothing
    assert recommend_combined(_oracle_from(res), ulines[:400], 3, mode) == [l[:3] for l in full[:400]]
    ar = AssociationRules(res, logger=Logger(enabled=False))
    first = {n: recommend_topn(_oracle_from(res), ulines, n) for n in (10,)}
    for n in (1, 3, 10, 64):
        want = [l[:n] for l in full]
        assert ar.run_topn(users, n, scores=True, combine=mode) == format_combined(want, mode, True)
        assert ar.run_topn(users, n, combine=mode) == format_combined(want, mode, False)
    # the case checks something: lists that differ from today's, and consequents of equal score
    differ = sum([t for t, _ in a[:10]] != [t for t, _ in b] for a, b in zip(full, first[10]))
    ties = sum(len({s for _, s in l}) < len(l) for l in full)
    assert differ >= 1 and ties >= 1
    if mode == "sum":
        assert (differ, ties) == (2087, 904)


@pytest.mark.parametrize("mode", MODES)
def test_n64_lists_hold_the_items_of_topn(native, mode):
    res, users, ar, _ = mined_case()
    top = ar.recommend_topn_shard(users, 64)
    rule, score = ar.recommend_combined_shard(users, 64, mode)
    assert rule.dtype == torch.int32 and score.dtype == torch.int64 and tuple(rule.shape) == (users.n_lines, 64)
    cons = torch.from_numpy(ar.rules().cons)
    items = lambda t: [sorted(cons[r[r >= 0].to(torch.int64)].tolist()) for r in t]
    a, b = items(top), items(rule)
    assert a == b and max(len(x) for x in a) == 61
    assert torch.equal(rule >= 0, score > 0)


def test_votes_reproduce_topn_when_every_consequent_has_one_rule(native):
    # every rule has a consequent of its own: every score is 1 and f orders the list, as first-match does
    rng = np.random.default_rng(3)
    F1 = 40
    cons = rng.permutation(F1)[:30].tolist()
    rules = []
    for c in cons:
        a = [x for x in rng.choice(F1, int(rng.integers(1, 3)), replace=False).tolist() if x != c] or [(c + 1) % F1]
        rules.append((tuple(sorted(a)), c))
    baskets = [sorted(rng.choice(F1, int(rng.integers(0, 12)), replace=False).tolist()) for _ in range(60)]
    boff, bask = csr_tensors(baskets)
    for n in (1, 4, 64):
        top = prim.recommend_topn(*rules_tensors(rules), F1, boff, bask, n)
        rule, score = prim.recommend_combined(*rules_tensors(rules), weight_tensor([1] * 30), F1, boff, bask, n)
        assert torch.equal(rule, top) and torch.equal(score, (top >= 0).to(torch.int64))
        assert int((top >= 0).sum(1).max()) == min(n, 6)       # lists of several entries


# ---------------------------------------------------------------------------
# printed lines, evaluation, JSON
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
def test_printed_lines_with_and_without_dedup(native, mode):
    res, urows = _small()
    users = parse_bytes(("\n".join(urows) + "\n").encode())
    want = recommend_combined(_oracle_from(res), [java_split_ws(r) for r in urows], 4, mode)
    outs = []
    for dedup in (True, False):
        ar = AssociationRules(res, logger=Logger(enabled=False))
        ar.dedup_baskets = dedup
        got = ar.run_topn(users, 4, scores=True, combine=mode)
        assert got == format_combined(want, mode, True)
        assert ar.run_topn(users, 4, combine=mode) == format_combined(want, mode, False)
        outs.append((got, ar.stats["distinct_baskets"]))
    assert outs[0][0] == outs[1][0] and outs[0][1] < outs[1][1] == len(urows)
    got = outs[0][0]
    assert "0" in got and max(l.count(" ") for l in got) >= 1
    tails = [e.rsplit(":", 1)[1] for l in got if l != "0" for e in l.split(" ")]
    if mode == "sum":
        assert all(repr(float(t)) == t and float(t) > 0 for t in tails) and any(float(t) > 1 for t in tails)
    else:
        assert all(t.isdigit() and int(t) >= 1 for t in tails) and any(int(t) > 1 for t in tails)
    with pytest.raises(ValueError):
        AssociationRules(res, logger=Logger(enabled=False)).run_topn(users, 4, combine="mean")
    with pytest.raises(ValueError):
        AssociationRules(res, logger=Logger(enabled=False)).recommend_combined_shard(users, 65, mode)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("n", [1, 3, 64])
def test_evaluate_matches_oracle(native, n, mode):
    res, urows = _small()
    users = parse_bytes(("\n".join(urows) + "\n").encode())
    want, want_lines = oracle_evaluation_combined(_oracle_from(res), [java_split_ws(r) for r in urows], n, mode)
    assert want["n_trials"] > 0 and 0 < sum(want["hits"]) < want["n_trials"]
    for dedup in (True, False):
        ar = AssociationRules(res, logger=Logger(enabled=False))
        ar.dedup_baskets = dedup
        ev = ar.evaluate(users, n, combine=mode)
        assert ev.combine == mode and json.loads(ev.as_json()) == want
        assert list(json.loads(ev.as_json())) == ["n", "combine"] + KEYS[1:]
        ev2, lines = ar.run_evaluate(users, n, rank_lines=True, combine=mode)
        assert ev2 == ev and lines == want_lines
        boff, ranks = ar.holdout_ranks_shard(users, n, combine=mode)
        assert ranks.tolist() == [int(e.rsplit(":", 1)[1]) for l in want_lines if l != "0" for e in l.split(" ")]


def test_as_json_without_combine_is_unchanged(native):
    rate, mrr, ndcg = metrics(3, [1, 2, 0], 7)
    today = ('{"n": 3, "n_lines": 5, "n_lines_skipped": 1, "n_trials": 7, "n_infrequent_tokens": 2, '
             f'"hits": [1, 2, 0], "hit_rate": [{rate[0]!r}, {rate[1]!r}, {rate[2]!r}], "mrr": {mrr!r}, "ndcg": {ndcg!r}}}')
    assert Evaluation.from_counts(3, 5, 1, 7, 2, [1, 2, 0]).as_json() == today
    assert Evaluation.from_counts(3, 5, 1, 7, 2, [1, 2, 0], "first").as_json() == today
    assert Evaluation.from_counts(3, 5, 1, 7, 2, [1, 2, 0], "votes").as_json() == today.replace(
        '{"n": 3, ', '{"n": 3, "combine": "votes", ')
    res, urows = _small()
    users = parse_bytes(("\n".join(urows) + "\n").encode())
    ar = AssociationRules(res, logger=Logger(enabled=False))
    assert ar.evaluate(users, 3, combine="first").as_json() == ar.evaluate(users, 3).as_json()
    assert "combine" not in ar.evaluate(users, 3).as_json()


# ---------------------------------------------------------------------------
# command line
# ---------------------------------------------------------------------------
def _cli(tmp_path, out, *flags):
    env = dict(os.environ, PYTHONPATH=ROOT)
    return subprocess.run([sys.executable, "-m", "fastapriori_amd", f"{tmp_path}/", f"{tmp_path}/{out}",
                           f"{tmp_path}/tmp", "--min-support", "0.25", "--device", "cpu", *flags],
                          capture_output=True, text=True, env=env, timeout=300)


FLAGS = ("--top-n", "3", "--top-n-scores", "--combine", "sum", "--evaluate", "3", "--evaluate-ranks", "--overwrite")
FILES = ("recommendsTopN", "evaluation", "evaluationRanks")


@pytest.fixture(scope="module")
def cli_runs(tmp_path_factory):
    """One job without the flags (a_), one with them (b_), then --rules-only from b's checkpoint."""
    d = tmp_path_factory.mktemp("combine")
    (d / "D.dat").write_text(D)
    (d / "U.dat").write_text(U)
    runs = {"a": _cli(d, "a_"), "b": _cli(d, "b_", *FLAGS)}
    for f in FILES:
        os.rename(d / f"b_{f}", d / f"b_first_{f}")
    runs["c"] = _cli(d, "b_", "--rules-only", *FLAGS)
    return d, runs


def test_cli_writes_the_oracles_lines(cli_runs):
    d, runs = cli_runs
    assert all(r.returncode == 0 for r in runs.values()), [r.stderr for r in runs.values()]
    _, _, res = run_oracle(D.splitlines(), U.splitlines(), 0.25)
    ulines = [java_split_ws(l) for l in U.splitlines()]
    top = format_combined(recommend_combined(res, ulines, 3, "sum"), "sum", True)
    ev, ranks = oracle_evaluation_combined(res, ulines, 3, "sum")
    assert any(" " in l for l in top) and "0" in top and ev["n_trials"] > 0 and sum(ev["hits"]) > 0
    assert (d / "b_first_recommendsTopN" / "part-00000").read_text() == "\n".join(top) + "\n"
    assert (d / "b_first_evaluation" / "part-00000").read_text() == json.dumps(ev) + "\n"
    assert (d / "b_first_evaluationRanks" / "part-00000").read_text() == "\n".join(ranks) + "\n"
    # recommends/ is the reference's first match, whatever the flag says
    assert (d / "a_recommends" / "part-00000").read_bytes() == (d / "b_recommends" / "part-00000").read_bytes()


def test_cli_rules_only_reproduces_the_files(cli_runs):
    d, runs = cli_runs
    assert runs["c"].returncode == 0, runs["c"].stderr
    for f in FILES:
        assert (d / f"b_first_{f}" / "part-00000").read_bytes() == (d / f"b_{f}" / "part-00000").read_bytes()


def test_cli_combine_needs_a_list():
    from fastapriori_amd.config import parse_args
    for flags in (("--combine", "sum"), ("--combine", "votes", "--rules"), ("--combine", "mean", "--top-n", "3")):
        with pytest.raises(SystemExit) as e:
            parse_args(["in/", "out/", *flags])
        assert e.value.code == 2                               # argparse's usage error
    assert parse_args(["in/", "out/"]).combine == "first"
    assert parse_args(["in/", "out/", "--combine", "first"]).combine == "first"
    assert parse_args(["in/", "out/", "--combine", "votes", "--evaluate", "5"]).combine == "votes"
    assert parse_args(["in/", "out/", "--combine", "sum", "--top-n", "5"]).combine == "sum"


def test_summary_and_metric(tmp_path):
    from fastapriori_amd.config import JobConfig
    from fastapriori_amd.parallel.comm import Comm
    from fastapriori_amd.pipeline import run_job
    (tmp_path / "D.dat").write_text(D)
    (tmp_path / "U.dat").write_text(U)
    mpath = str(tmp_path / "metrics.jsonl")
    s = run_job(JobConfig(input=f"{tmp_path}/", output=f"{tmp_path}/o_", min_support=0.25, device="cpu", evaluate=2,
                          top_n=2, combine="votes", metrics_path=mpath), Comm())
    assert s["combine"] == "votes"
    recs = [json.loads(l) for l in open(mpath)]
    assert [r["combine"] for r in recs if r.get("phase") in ("evaluate", "job")] == ["votes", "votes"]
    s0 = run_job(JobConfig(input=f"{tmp_path}/", output=f"{tmp_path}/p_", min_support=0.25, device="cpu", evaluate=2,
                           top_n=2), Comm())
    assert "combine" not in s0


# ---------------------------------------------------------------------------
# across ranks (gloo)
# ---------------------------------------------------------------------------
def _combined_files(path_prefix: str, ms: float, n: int, mode: str):
    from fastapriori_amd.models.apriori import FastApriori, MinerConfig
    from fastapriori_amd.parallel.comm import init_comm, shutdown_comm
    from fastapriori_amd.utils.io import read_shard

    comm = init_comm("cpu")
    try:
        shard = read_shard(path_prefix + "D.dat", comm)
        res = FastApriori(ms, comm, MinerConfig(trim_min_rows=0, min_support=ms),
                          Logger(comm.rank, enabled=False)).run(shard)
        users = read_shard(path_prefix + "U.dat", comm)
        ar = AssociationRules(res, comm, Logger(comm.rank, enabled=False))
        top = ar.run_topn(users, n, scores=True, combine=mode)
        ev, lines = ar.run_evaluate(users, n, rank_lines=True, combine=mode)
        return top, ev.as_json(), lines
    finally:
        shutdown_comm(comm)


def test_world_size_two_gives_the_same_files(tmp_path):
    from fastapriori_amd.utils.io import write_quest_file
    write_quest_file(str(tmp_path / "D.dat"), 2000, 8.0, 3.0, 60, 50, seed=2)
    write_quest_file(str(tmp_path / "U.dat"), 301, 8.0, 3.0, 60, 50, seed=2, users=True)
    ref = spawn_local(_combined_files, 1, f"{tmp_path}/", 0.02, 3, "sum")[0]
    outs = spawn_local(_combined_files, 2, f"{tmp_path}/", 0.02, 3, "sum")
    assert outs[0] == ref and outs[1] == (None, ref[1], None)  # the metrics on every rank, the lines on rank 0
    ev = json.loads(ref[1])
    assert ev["combine"] == "sum" and ev["n_lines"] == 301 == len(ref[0]) == len(ref[2]) and sum(ev["hits"]) > 0
    assert any(l.count(" ") == 2 for l in ref[0])
    # a summed score above 2^32 crossed the ranks as int64
    assert any(float(e.rsplit(":", 1)[1]) > 1.0 for l in ref[0] if l != "0" for e in l.split(" "))
