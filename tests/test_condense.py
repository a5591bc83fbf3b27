"""Closed and maximal frequent itemsets (--closed, --maximal) on the CPU path:
MiningResult.condensed against a hand example and a brute force over every proper
superset, the properties that make the two forms useful, edge shapes of
ops.primitives.condense_flags, the command line and two gloo ranks."""
import functools
import itertools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from fastapriori_amd.models.apriori import FastApriori, MinerConfig
from fastapriori_amd.ops import primitives as prim
from fastapriori_amd.parallel.comm import Comm
from fastapriori_amd.parallel.launch import spawn_local
from fastapriori_amd.utils import io
from fastapriori_amd.utils.metrics import Logger

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
D = "1 2 3\n1 2 3\n1 2\n3\n"           # min count 2: all 7 non-empty subsets of {1, 2, 3} are frequent
U = "1\n2 3\n4\n"
CLOSED = {(frozenset("3"), 3), (frozenset("12"), 3), (frozenset("123"), 2)}
MAXIMAL = {(frozenset("123"), 2)}


def _mine(text: str, ms: float, **kw):
    return FastApriori(ms, config=MinerConfig(min_support=ms, **kw), logger=Logger(enabled=False)).run(
        io.parse_bytes(text.encode()))


def _tokens(res) -> set:
    return {(frozenset(res.items[r] for r in s), c) for s, c in res.as_dict().items()}


def test_hand_example():
    res = _mine(D, 0.5)
    assert res.n_itemsets == 7 and res.min_count == 2
    closed, maximal = res.condensed("closed"), res.condensed("maximal")
    assert _tokens(closed) == CLOSED and _tokens(maximal) == MAXIMAL
    for c in (closed, maximal):
        assert c.items == res.items and c.min_count == res.min_count and c.n_lines == res.n_lines
        assert [l.shape[1] for l in c.levels] == [1, 2, 3] and all(l.dtype == np.int32 for l in c.levels)
        assert [len(l) for l in c.levels] == [len(n) for n in c.counts]
    assert closed.stats == {"condensed": "closed", "n_all": 7}
    assert maximal.stats == {"condensed": "maximal", "n_all": 7}
    assert [len(l) for l in maximal.levels] == [0, 0, 1]          # emptied levels keep their place
    assert len(maximal.digest()) == 64 and maximal.digest() != closed.digest()
    with pytest.raises(ValueError):
        res.condensed("free")


@functools.lru_cache(maxsize=None)
def quest300():
    """The mined case both test files share: (result, its closed form, its maximal form) on the
    C++ path.  Both the "equal count" and the "smaller count" branch are live at every level."""
    sh = io.generate_shard(300, Comm(), "cpu", 8.0, 3.0, 20, 30, seed=5)
    res = FastApriori(0.02, config=MinerConfig(min_support=0.02), logger=Logger(enabled=False)).run(sh)
    return res, res.condensed("closed"), res.condensed("maximal")


def _proper_subsets(s: frozenset):
    for m in range(1, len(s)):
        yield from map(frozenset, itertools.combinations(sorted(s), m))


def test_brute_force():
    res, closed, maximal = quest300()
    d = res.as_dict()
    assert (res.n_itemsets, len(res.levels)) == (9215, 10)
    # every proper subset of every frequent S, of any size: T is not maximal, and not closed
    # when the counts are equal (the code under test looks one level up only)
    has_sup, has_eq = set(), set()
    for s, c in d.items():
        for t in _proper_subsets(s):
            has_sup.add(t)
            if d[t] == c:
                has_eq.add(t)
    want_closed = {s: c for s, c in d.items() if s not in has_eq}
    want_maximal = {s: c for s, c in d.items() if s not in has_sup}
    assert (len(want_closed), len(want_maximal)) == (3815, 503)
    assert closed.as_dict() == want_closed and closed.n_itemsets == 3815
    assert maximal.as_dict() == want_maximal and maximal.n_itemsets == 503
    # both branches at every level that has a level above it
    for k in range(1, len(res.levels)):
        level = [frozenset(r) for r in res.levels[k - 1].tolist()]
        assert any(t in has_eq for t in level) and any(t not in has_eq for t in level), k


def test_properties():
    res, closed, maximal = quest300()
    d, dc, dm = res.as_dict(), closed.as_dict(), maximal.as_dict()
    assert set(dm) <= set(dc) <= set(d)
    assert all(d[s] == c for s, c in dc.items())
    # lossless: a frequent itemset's count is the largest count among its closed supersets
    best: dict = {}
    for s, c in dc.items():
        for t in itertools.chain(_proper_subsets(s), [s]):
            if best.get(t, 0) < c:
                best[t] = c
    assert best == d
    # every frequent itemset is inside a maximal one
    covered = set()
    for s in dm:
        covered.update(_proper_subsets(s))
        covered.add(s)
    assert covered == set(d)
    for c in (closed, maximal):
        for rows in c.levels:
            r = rows.tolist()
            assert all(a < b for a, b in zip(r, r[1:]))                     # still strictly lexicographic
            assert all(all(x < y for x, y in zip(a, a[1:])) for a in r)


# ---------------------------------------------------------------------------
# an analytic lattice (no mining): the flags follow from the weights
# ---------------------------------------------------------------------------
BIG = 2 ** 33 + 1000


def lattice(with_16_17: bool = False):
    """levels, counts and the expected (has_superset, has_equal_superset) per level.

    Every k-combination of items 0..10, the 3-clique on {11, 12, 13}, the pair {14, 15}
    and, on request, the pair {16, 17}; count(S) = BIG - sum of w_i over S with
    w_2 = w_7 = w_14 = w_15 = w_16 = 0, w_5 = 2^32 and every other weight a distinct small
    positive number.  On 0..10, S is closed iff {2, 7} is inside it (adding 2 or 7
    changes nothing, adding anything else lowers the count; S and S + {5} differ in
    the high word only) and only the 11-set is maximal.  The clique's sets are all
    closed, its triple maximal; {14}, {15} and {17} are not closed, {16} is, and the
    pairs {14, 15} and {16, 17} are closed and maximal.
    One (itemset, position) per thread: 11264 = 44 x 256 elements above level 1, and
    11266 with {16, 17} (two live threads in a 45th workgroup of 256)."""
    w = {i: i + 1 for i in range(18)}
    w.update({2: 0, 7: 0, 14: 0, 15: 0, 16: 0, 5: 2 ** 32})
    groups = [tuple(range(11)), (11, 12, 13), (14, 15)] + ([(16, 17)] if with_16_17 else [])
    levels, counts, want = [], [], []
    for k in range(1, 12):
        rows = sorted(c for g in groups for c in itertools.combinations(g, k))
        levels.append(np.array(rows, dtype=np.int32).reshape(-1, k))
        counts.append(np.array([BIG - sum(w[i] for i in r) for r in rows], dtype=np.int64))
        sup, eq = [], []
        for r in rows:
            g = next(g for g in groups if r[0] in g)
            sup.append(int(k < len(g)))
            if g[0] == 0:
                eq.append(int(not {2, 7} <= set(r)))
            else:
                eq.append(int(r in ((14,), (15,), (17,))))
        want.append((np.array(sup, dtype=np.uint8), np.array(eq, dtype=np.uint8)))
    n_elements = sum(len(l) * k for k, l in enumerate(levels, 1) if k >= 2)
    assert n_elements == (11266 if with_16_17 else 11264)
    return levels, counts, want


def check_flags(got, want):
    assert len(got) == len(want)
    for k, ((sup, eq), (wsup, weq)) in enumerate(zip(got, want), 1):
        assert sup.dtype == torch.uint8 and eq.dtype == torch.uint8
        assert np.array_equal(sup.cpu().numpy(), wsup), k
        assert np.array_equal(eq.cpu().numpy(), weq), k


@pytest.mark.parametrize("with_16_17", [False, True])
def test_lattice_on_the_host(with_16_17):
    levels, counts, want = lattice(with_16_17)
    assert all(w[1].any() and not w[1].all() for w in want[:10])
    check_flags(prim.condense_flags(levels, counts, "cpu"), want)


# ---------------------------------------------------------------------------
# edge shapes
# ---------------------------------------------------------------------------
def _lv(rows, k):
    return np.array(rows, dtype=np.int32).reshape(-1, k)


def edge_cases():
    """name -> (levels, counts, expected flags as lists): shapes with nothing, or little, to mark."""
    l1, c1 = _lv([[0], [1], [2]], 1), np.array([5, 4, 3], dtype=np.int64)
    return {
        "level1_only": ([l1], [c1], [([0, 0, 0], [0, 0, 0])]),
        "empty_level2": ([l1, _lv([], 2)], [c1, np.zeros(0, np.int64)], [([0, 0, 0], [0, 0, 0]), ([], [])]),
        "trailing_empty": ([l1, _lv([[0, 1], [0, 2]], 2), _lv([], 3)],
                           [c1, np.array([4, 2], dtype=np.int64), np.zeros(0, np.int64)],
                           [([1, 1, 1], [0, 1, 0]), ([0, 0], [0, 0]), ([], [])]),
        "one_row": ([l1, _lv([[1, 2]], 2)], [c1, np.array([3], dtype=np.int64)],
                    [([0, 1, 1], [0, 0, 1]), ([0], [0])]),
    }


@pytest.mark.parametrize("name", sorted(edge_cases()))
def test_edge_shapes(name):
    levels, counts, want = edge_cases()[name]
    got = prim.condense_flags(levels, counts, "cpu")
    assert [(s.tolist(), e.tolist()) for s, e in got] == want
    assert all(s.device.type == "cpu" and s.dtype == torch.uint8 and e.dtype == torch.uint8 for s, e in got)


def test_no_levels_at_all():
    assert prim.condense_flags([], [], "cpu") == []


def test_not_downward_closed_raises():
    res, _, _ = quest300()
    levels, counts = [l.copy() for l in res.levels], [c.copy() for c in res.counts]
    sub = levels[3][0][:3]                                   # a 3-subset of the first 4-itemset
    hit = int(np.flatnonzero((levels[2] == sub).all(1))[0])
    levels[2], counts[2] = np.delete(levels[2], hit, 0), np.delete(counts[2], hit)
    with pytest.raises(RuntimeError, match="size 4 has a subset that is not in level 3"):
        prim.condense_flags(levels, counts, "cpu")
    from fastapriori_amd.models.data import MiningResult
    with pytest.raises(RuntimeError, match="not downward closed"):
        MiningResult(res.items, levels, counts, res.min_count, res.n_lines).condensed("closed")
    with pytest.raises(ValueError):
        prim.condense_flags(levels[:2], counts[:1], "cpu")


# ---------------------------------------------------------------------------
# command line
# ---------------------------------------------------------------------------
def _cli(d, out, *flags, temp=True):
    env = dict(os.environ, PYTHONPATH=ROOT)
    args = [f"{d}/", f"{d}/{out}"] + ([f"{d}/tmp_{out}"] if temp else [])
    return subprocess.run([sys.executable, "-m", "fastapriori_amd", *args, "--min-support", "0.5", "--device", "cpu",
                           *flags], capture_output=True, text=True, env=env, timeout=300)


def _read(path) -> set:
    """The "a b c[cnt]" lines of a part file as a set of (token set, count)."""
    out = set()
    for line in open(path, encoding="utf-8").read().splitlines():
        body, cnt = line[:-1].rsplit("[", 1)
        assert line.endswith("]")
        out.add((frozenset(body.split(" ")), int(cnt)))
    return out


@pytest.fixture(scope="module")
def cli_runs(tmp_path_factory):
    """a_: no flag; b_: both flags with --with-counts, then --rules-only --maximal from b_'s saved
    files (no temp path, so no checkpoint); d_: --max-level 2 --closed."""
    d = tmp_path_factory.mktemp("condense")
    (d / "D.dat").write_text(D)
    (d / "U.dat").write_text(U)
    runs = {"a": _cli(d, "a_"), "b": _cli(d, "b_", "--closed", "--maximal", "--with-counts")}
    os.rename(d / "b_maximalItemset", d / "b_max_first")
    runs["c"] = _cli(d, "b_", "--rules-only", "--maximal", "--overwrite", temp=False)
    runs["d"] = _cli(d, "d_", "--max-level", "2", "--closed")
    return d, runs


def test_cli_writes_both_forms(cli_runs):
    d, runs = cli_runs
    assert all(r.returncode == 0 for r in runs.values()), [r.stderr for r in runs.values()]
    assert _read(d / "b_closedItemset" / "part-00000") == CLOSED
    assert _read(d / "b_max_first" / "part-00000") == MAXIMAL
    assert (d / "b_closedItemset" / "_SUCCESS").exists() and (d / "b_max_first" / "_SUCCESS").exists()
    assert "==== Total time for get closedItemsets " in runs["b"].stdout
    assert "==== Total time for get maximalItemsets " in runs["b"].stdout
    out = runs["b"].stdout
    assert (out.index("Total time for get freqItemsets") < out.index("Total time for get closedItemsets")
            < out.index("Total time for get maximalItemsets") < out.index("Total time for get recommends"))


def test_cli_without_the_flags_nothing_changes(cli_runs):
    d, runs = cli_runs
    for name in ("freqItemset", "recommends"):
        assert (d / f"a_{name}" / "part-00000").read_bytes() == (d / f"b_{name}" / "part-00000").read_bytes()
    assert not (d / "a_closedItemset").exists() and not (d / "a_maximalItemset").exists()
    assert "closedItemsets" not in runs["a"].stdout and "maximalItemsets" not in runs["a"].stdout


def test_cli_round_trip_and_rules_only(cli_runs):
    d, runs = cli_runs
    back = io.load_saved_results(str(d / "b_closedItemset"), str(d / "b_ItemsToRank"))
    assert _tokens(back) == CLOSED
    # --rules-only from the saved files: the same maximalItemset as the mining run wrote
    assert (d / "b_maximalItemset" / "part-00000").read_bytes() == (d / "b_max_first" / "part-00000").read_bytes()
    assert "maximalItemsets" in runs["c"].stdout and "closedItemsets" not in runs["c"].stdout


def test_cli_max_level_two_reports_every_pair_closed(cli_runs):
    d, _ = cli_runs
    got = _read(d / "d_closedItemset" / "part-00000")
    pairs = {(s, c) for s, c in got if len(s) == 2}
    assert pairs == {(frozenset("12"), 3), (frozenset("13"), 2), (frozenset("23"), 2)}
    assert max(len(s) for s, _ in got) == 2 and (frozenset("3"), 3) in got and (frozenset("1"), 3) not in got
    assert pairs != {x for x in CLOSED if len(x[0]) == 2}          # without the cap only {1, 2} is closed


def test_flags_and_summary(tmp_path):
    from fastapriori_amd.config import JobConfig, parse_args
    from fastapriori_amd.pipeline import run_job
    cfg = parse_args(["in/", "out/", "--closed"])
    assert cfg.closed and not cfg.maximal and not parse_args(["in/", "out/"]).closed
    assert parse_args(["in/", "out/", "--maximal"]).maximal
    (tmp_path / "D.dat").write_text(D)
    (tmp_path / "U.dat").write_text(U)
    log = tmp_path / "metrics.jsonl"
    s = run_job(JobConfig(input=f"{tmp_path}/", output=f"{tmp_path}/o_", min_support=0.5, device="cpu", closed=True,
                          maximal=True, metrics_path=str(log)), Comm())
    assert (s["n_closed"], s["n_maximal"], s["n_itemsets"]) == (3, 1, 7)
    import json
    recs = [r for r in map(json.loads, log.read_text().splitlines()) if r.get("phase") == "condense"]
    assert [(r["kind"], r["n_all"], r["n_kept"]) for r in recs] == [("closed", 7, 3), ("maximal", 7, 1)]
    assert all("ms" in r for r in recs)
    s0 = run_job(JobConfig(input=f"{tmp_path}/", output=f"{tmp_path}/p_", min_support=0.5, device="cpu"), Comm())
    assert "n_closed" not in s0 and "n_maximal" not in s0
    os.makedirs(tmp_path / "q_closedItemset")                              # --overwrite applies as elsewhere
    q = dict(input=f"{tmp_path}/", output=f"{tmp_path}/q_", min_support=0.5, device="cpu", closed=True)
    with pytest.raises(RuntimeError, match="--closed failed on rank 0: OutputExistsError"):
        run_job(JobConfig(**q), Comm())
    assert run_job(JobConfig(**q, overwrite=True), Comm())["n_closed"] == 3


# ---------------------------------------------------------------------------
# across ranks (gloo)
# ---------------------------------------------------------------------------
def _job(d: str, out: str):
    from fastapriori_amd.config import JobConfig
    from fastapriori_amd.parallel.comm import init_comm, shutdown_comm
    from fastapriori_amd.pipeline import run_job

    comm = init_comm("cpu")
    try:
        s = run_job(JobConfig(input=f"{d}/", output=f"{d}/{out}", min_support=0.02, device="cpu", closed=True,
                              maximal=True, checkpoint=False), comm)
        return s["n_itemsets"], s["n_closed"], s["n_maximal"]
    finally:
        shutdown_comm(comm)


def test_world_size_two_writes_the_same_files(tmp_path):
    io.write_quest_file(str(tmp_path / "D.dat"), 2000, 8.0, 3.0, 60, 50, seed=2)
    io.write_quest_file(str(tmp_path / "U.dat"), 101, 8.0, 3.0, 60, 50, seed=2, users=True)
    ref = spawn_local(_job, 1, str(tmp_path), "w1_", timeout=300)[0]
    outs = spawn_local(_job, 2, str(tmp_path), "w2_", timeout=300)        # a hang at the meeting point times out
    assert outs[0] == ref and outs[1] == ref and ref[0] > ref[1] >= ref[2] > 0
    for name in ("closedItemset", "maximalItemset", "freqItemset"):
        assert (tmp_path / f"w1_{name}" / "part-00000").read_bytes() == \
            (tmp_path / f"w2_{name}" / "part-00000").read_bytes()
    assert len(_read(tmp_path / "w2_closedItemset" / "part-00000")) == ref[1]
