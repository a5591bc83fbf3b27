"""Ranked top-N recommendations (--top-n) on the CPU path: AssociationRules.run_topn against the
brute-force oracle, basket de-duplication, the command line and the gather across ranks."""
import os
import subprocess
import sys

import numpy as np
import pytest
from hypothesis import given, settings
from hypothesis import strategies as st

from fastapriori_amd.models.apriori import FastApriori, MinerConfig
from fastapriori_amd.models.oracle import OracleResult, recommend_topn, run_oracle
from fastapriori_amd.models.rules import AssociationRules
from fastapriori_amd.parallel.launch import spawn_local
from fastapriori_amd.utils.io import parse_bytes
from fastapriori_amd.utils.jvm import java_split_ws
from fastapriori_amd.utils.metrics import Logger

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
row = st.lists(st.sampled_from([str(i) for i in range(1, 10)]), min_size=0, max_size=7)


def _text(rows):
    return "\n".join(" ".join(r) for r in rows) + "\n"


def _oracle_from(res) -> OracleResult:
    """Oracle object over the miner's own rank space (so rules compare rank-for-rank)."""
    return OracleResult(items=res.items, counts1=res.counts[0].tolist(), itemsets=res.as_dict(),
                        min_count=res.min_count, n_lines=res.n_lines)


def _format(tops, scores):
    """The file format: entries in list order joined by one space, "0" for an empty list."""
    return [" ".join(f"{t}:{c!r}" if scores else t for t, c in top) if top else "0" for top in tops]


@settings(max_examples=60, deadline=None)
@given(st.lists(row, min_size=1, max_size=50), st.lists(row, min_size=0, max_size=20),
       st.sampled_from([0.05, 0.1, 0.2]))
def test_topn_matches_oracle(drows, urows, ms):
    res = FastApriori(ms, config=MinerConfig(min_support=ms), logger=Logger(enabled=False)).run(
        parse_bytes(_text(drows).encode()))
    ar = AssociationRules(res, logger=Logger(enabled=False))
    orc = _oracle_from(res)
    utext = _text(urows) if urows else ""
    users = parse_bytes(utext.encode())
    ulines = [java_split_ws(l) for l in utext.splitlines()]
    for n in (1, 3):
        want = recommend_topn(orc, ulines, n)
        assert all(len(t) <= n and len({tok for tok, _ in t}) == len(t) for t in want)
        assert ar.run_topn(users, n, scores=True) == _format(want, True)      # bit-identical confidences
        assert ar.run_topn(users, n) == _format(want, False)
    first = ar.run_topn(users, 1, scores=True)
    assert [l.split(" ")[0].rsplit(":", 1)[0] for l in first] == ar.run(users)


def test_topn_lists_are_longer_than_one():
    # the property test's data must not be all short lists: here a user gets three ranked items
    d = "1 2 3 4\n" * 6 + "1 2\n" * 3 + "1 3\n" * 2 + "1\n"
    res = FastApriori(0.1, config=MinerConfig(min_support=0.1), logger=Logger(enabled=False)).run(
        parse_bytes(d.encode()))
    ar = AssociationRules(res, logger=Logger(enabled=False))
    users = parse_bytes(b"1\n9\n\n1 2\n")
    got = ar.run_topn(users, 3, scores=True)
    want = recommend_topn(_oracle_from(res), [["1"], ["9"], [], ["1", "2"]], 3)
    assert got == _format(want, True)
    assert [t for t, _ in want[0]] == ["2", "3", "4"] and want[1] == [] and got[1] == got[2] == "0"
    confs = [float(e.rsplit(":", 1)[1]) for e in got[0].split(" ")]
    assert confs == sorted(confs, reverse=True) and confs == [c for _, c in want[0]]
    with pytest.raises(ValueError):
        ar.run_topn(users, 0)
    with pytest.raises(ValueError):
        ar.recommend_topn_shard(users, 65)


def test_duplicate_baskets_give_identical_lines():
    # the data of test_rules.test_duplicate_baskets_recommended_once
    rng = np.random.default_rng(5)
    drows = [" ".join(map(str, rng.choice(12, size=rng.integers(1, 6), replace=False))) for _ in range(400)]
    res = FastApriori(0.05, config=MinerConfig(min_support=0.05),
                      logger=Logger(enabled=False)).run(parse_bytes(("\n".join(drows) + "\n").encode()))
    pool = [[1, 2], [3], [2, 4, 5], [], [7, 1], [11, 10, 3]]
    urows = []
    for _ in range(300):
        b = list(pool[rng.integers(len(pool))])
        rng.shuffle(b)
        urows.append(" ".join(map(str, b + b[:1])))      # shuffled, with a repeated token
    users = parse_bytes(("\n".join(urows) + "\n").encode())
    on = AssociationRules(res, logger=Logger(enabled=False))
    got = on.run_topn(users, 4, scores=True)
    off = AssociationRules(res, logger=Logger(enabled=False))
    off.dedup_baskets = False
    assert got == off.run_topn(users, 4, scores=True)
    assert on.stats["distinct_baskets"] <= len(pool) < off.stats["distinct_baskets"] == 300
    assert got == _format(recommend_topn(_oracle_from(res), [java_split_ws(r) for r in urows], 4), True)
    assert max(l.count(" ") for l in got) >= 1 and "0" in got
    top = on.recommend_topn_shard(users, 4)
    assert tuple(top.shape) == (300, 4) and str(top.dtype) == "torch.int32"


def test_no_rules_gives_all_zero():
    res = FastApriori(0.5).run(parse_bytes(b"1\n1\n2\n"))
    ar = AssociationRules(res)
    assert ar.rules().n_rules == 0
    assert ar.run_topn(parse_bytes(b"1\n2\n\n3 4\n"), 3, scores=True) == ["0", "0", "0", "0"]
    assert ar.run_topn(parse_bytes(b""), 3) == []


# ---------------------------------------------------------------------------
# command line
# ---------------------------------------------------------------------------
D = "1 2 3\n1 2 4\n2 3 4\n1 2 4\n2 4\n4 5\n1 2\n"
U = "1\n2\n7 8\n2 4\n4 1 2\n3\n1\n"


def _cli(tmp_path, out, *flags):
    env = dict(os.environ, PYTHONPATH=ROOT)
    return subprocess.run([sys.executable, "-m", "fastapriori_amd", f"{tmp_path}/", f"{tmp_path}/{out}",
                           f"{tmp_path}/tmp", "--min-support", "0.25", "--device", "cpu", *flags],
                          capture_output=True, text=True, env=env, timeout=300)


@pytest.fixture(scope="module")
def cli_runs(tmp_path_factory):
    """One job without the flag (a_), one with --top-n 2 (b_), then --rules-only from b's checkpoint."""
    d = tmp_path_factory.mktemp("topn")
    (d / "D.dat").write_text(D)
    (d / "U.dat").write_text(U)
    runs = {"a": _cli(d, "a_"), "b": _cli(d, "b_", "--top-n", "2", "--overwrite")}
    os.rename(d / "b_recommendsTopN", d / "b_first")
    runs["c"] = _cli(d, "b_", "--rules-only", "--top-n", "2", "--top-n-scores", "--overwrite")
    return d, runs


def _oracle_lines(n, scores):
    _, _, res = run_oracle(D.splitlines(), U.splitlines(), 0.25)
    return _format(recommend_topn(res, [java_split_ws(l) for l in U.splitlines()], n), scores)


def test_cli_writes_top_n(cli_runs):
    d, runs = cli_runs
    assert all(r.returncode == 0 for r in runs.values()), [r.stderr for r in runs.values()]
    want = _oracle_lines(2, False)
    assert any(" " in l for l in want) and "0" in want
    assert (d / "b_first" / "part-00000").read_text() == "\n".join(want) + "\n"
    assert (d / "b_first" / "_SUCCESS").exists()
    # recommends/ does not change with the flag, and without it no top-N directory appears
    assert (d / "a_recommends" / "part-00000").read_bytes() == (d / "b_recommends" / "part-00000").read_bytes()
    assert not (d / "a_recommendsTopN").exists()


def test_cli_rules_only_reproduces_the_file(cli_runs):
    d, _ = cli_runs
    scored = (d / "b_recommendsTopN" / "part-00000").read_text()
    assert scored == "\n".join(_oracle_lines(2, True)) + "\n"
    strip = [" ".join(e.rsplit(":", 1)[0] for e in l.split(" ")) for l in scored.splitlines()]
    assert "\n".join(strip) + "\n" == (d / "b_first" / "part-00000").read_text()


@pytest.mark.parametrize("flags", [("--top-n", "65"), ("--top-n", "-1"), ("--top-n-scores",)])
def test_cli_rejects_bad_flags(flags):
    from fastapriori_amd.config import parse_args
    with pytest.raises(SystemExit) as e:
        parse_args(["in/", "out/", *flags])
    assert e.value.code == 2                                   # argparse's usage error
    cfg = parse_args(["in/", "out/", "--top-n", "64", "--top-n-scores"])
    assert cfg.top_n == 64 and cfg.top_n_scores and parse_args(["in/", "out/"]).top_n == 0


def test_summary_and_steps(tmp_path):
    from fastapriori_amd.config import JobConfig
    from fastapriori_amd.parallel.comm import Comm
    from fastapriori_amd.pipeline import run_job
    (tmp_path / "D.dat").write_text(D)
    (tmp_path / "U.dat").write_text(U)
    s = run_job(JobConfig(input=f"{tmp_path}/", output=f"{tmp_path}/o_", min_support=0.25, device="cpu", top_n=2),
                Comm())
    want = _oracle_lines(2, False)
    assert s["top_n"] == 2 and s["n_topn_entries"] == sum(len(l.split(" ")) for l in want if l != "0")
    assert "topn" in s["recommend_steps_ms"]
    s0 = run_job(JobConfig(input=f"{tmp_path}/", output=f"{tmp_path}/p_", min_support=0.25, device="cpu"), Comm())
    assert "top_n" not in s0 and "topn" not in s0["recommend_steps_ms"]


# ---------------------------------------------------------------------------
# across ranks (gloo)
# ---------------------------------------------------------------------------
def _topn_file(path_prefix: str, ms: float, n: int):
    from fastapriori_amd.parallel.comm import init_comm, shutdown_comm
    from fastapriori_amd.utils.io import read_shard

    comm = init_comm("cpu")
    try:
        shard = read_shard(path_prefix + "D.dat", comm)
        res = FastApriori(ms, comm, MinerConfig(trim_min_rows=0, min_support=ms),
                          Logger(comm.rank, enabled=False)).run(shard)
        users = read_shard(path_prefix + "U.dat", comm)
        return AssociationRules(res, comm, Logger(comm.rank, enabled=False)).run_topn(users, n, scores=True)
    finally:
        shutdown_comm(comm)


def test_world_size_two_gives_the_same_lines(tmp_path):
    from fastapriori_amd.utils.io import write_quest_file
    write_quest_file(str(tmp_path / "D.dat"), 2000, 8.0, 3.0, 60, 50, seed=2)
    write_quest_file(str(tmp_path / "U.dat"), 301, 8.0, 3.0, 60, 50, seed=2, users=True)
    ref = spawn_local(_topn_file, 1, f"{tmp_path}/", 0.02, 3)[0]
    outs = spawn_local(_topn_file, 2, f"{tmp_path}/", 0.02, 3)
    assert outs[0] == ref and outs[1] is None
    assert len(ref) == 301 and any(l.count(" ") == 2 for l in ref)
