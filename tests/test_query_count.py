"""The query counter on the CPU (models/query.py count_itemsets -> csrc/host/query.cpp):
the support of GIVEN itemsets over the raw parsed rows, against brute force with Python
sets (models/oracle.py count_itemsets).  Every comparison is exact integer equality."""
import itertools
import os
import random

import numpy as np
import pytest

from fastapriori_amd.parallel.launch import spawn_local


def _db(mode: str, n: int = 400, seed: int = 1, repeats: bool = True):
    """(text, lines as token lists): random lines over 40 tokens, some blank, some with a
    repeated token, CRLF now and then."""
    from fastapriori_amd.utils.jvm import java_split_ws
    rng = random.Random(seed)
    voc = [str(i) for i in range(40)] if mode == "numeric" else \
        [f"w{i}" for i in range(34)] + ["é", "ß", "1", "2", "7", "39"]
    rows = []
    for _ in range(n):
        toks = rng.sample(voc, rng.randint(0, 14))
        if repeats and toks and rng.random() < 0.3:
            toks.append(toks[0])
        rows.append(" ".join(toks))
    text = "".join(r + ("\r\n" if rng.random() < 0.1 else "\n") for r in rows)
    return text, [java_split_ws(r) for r in rows], voc


def _queries(voc, lines, seed=2):
    rng = random.Random(seed)
    qs = [rng.sample(voc, k) for k in (1, 2, 3) for _ in range(60)]
    qs += [[voc[0]], [voc[0]], [voc[1], voc[0]], [voc[0], voc[1]]]              # duplicates, either order
    qs += [[voc[3], voc[3]], [voc[3], voc[4], voc[3]]]                             # repeated tokens
    qs += [["absent"], [voc[2], "absent"], ["4x"], [""], ["", voc[5]]]             # absent tokens, the blank line
    qs += [list(voc)]                                                              # 40 items
    qs += [list(l) for l in lines[:5] if l]                                        # whole lines
    return qs


@pytest.mark.parametrize("db_mode", ["numeric", "dict"])
@pytest.mark.parametrize("q_mode", ["lists", "numeric_file", "dict_file"])
def test_counts_match_brute_force(native, tmp_path, db_mode, q_mode):
    from fastapriori_amd import ItemsetQueries, count_itemsets
    from fastapriori_amd.models import oracle
    from fastapriori_amd.utils.io import parse_bytes
    text, lines, voc = _db(db_mode)
    shard = parse_bytes(text.encode("utf-8"))
    assert shard.vocab.numeric == (db_mode == "numeric")
    qs = _queries(voc, lines)
    if q_mode == "lists":
        queries = ItemsetQueries.from_lists(qs)
    else:
        # a numeric query file against either database, and a dictionary one (a file line
        # cannot say "the empty token and another": it is trimmed)
        qs = [q for q in qs if "" not in q or len(q) == 1]
        if q_mode == "numeric_file":
            qs = [q for q in qs if all(t == "" or t.isdigit() for t in q)] + [["1", "2"], ["7"], ["39", "1", "39"],
                                                                             ["12345"]]
        else:
            qs = qs + [["1", "w2"], ["w1"]]
        p = tmp_path / "q.dat"
        p.write_bytes("".join(" ".join(q) + "\n" for q in qs).encode("utf-8"))
        queries = ItemsetQueries.from_file(str(p))
        assert queries.n_queries == len(qs)
        assert (queries.hashes is None) == (q_mode == "numeric_file")
        for i in (0, len(qs) - 1):
            assert queries.query_tokens(i) == list(dict.fromkeys(qs[i]))
    want = oracle.count_itemsets(lines, qs)
    got = count_itemsets(shard, queries)
    assert got.dtype == np.int64 and got.tolist() == want
    assert sum(want) > 0 and any(w == 0 for w in want)


def test_one_item_query_is_a_line_count_below_the_mined_occurrence_count(native):
    from fastapriori_amd import ItemsetQueries, count_itemsets, mine
    from fastapriori_amd.utils.io import parse_bytes
    text = "1 1 2\n1 2\n1 1 1\n3\n2 1\n"
    shard = parse_bytes(text.encode())
    res = mine(shard, 0.2)
    mined = {res.items[r[0]]: int(c) for r, c in zip(res.levels[0].tolist(), res.counts[0].tolist())}
    got = count_itemsets(shard, ItemsetQueries.from_lists([["1"], ["2"], ["1", "2"]])).tolist()
    assert mined["1"] == 7 and got[0] == 4 and got[0] < mined["1"]       # occurrences against lines
    assert mined["2"] == 3 and got[1] == 3                                 # no repeats: they agree
    pair = {frozenset(res.items[i] for i in r): int(c) for r, c in zip(res.levels[1].tolist(), res.counts[1].tolist())}
    assert got[2] == 3 == pair[frozenset(["1", "2"])]                      # from two items on they agree


def test_empty_query_list_and_empty_database(native):
    from fastapriori_amd import ItemsetQueries, count_itemsets
    from fastapriori_amd.utils.io import parse_bytes
    shard = parse_bytes(b"1 2\n2 3\n")
    assert count_itemsets(shard, ItemsetQueries.from_lists([])).tolist() == []
    assert count_itemsets(parse_bytes(b""), ItemsetQueries.from_lists([["1"], ["2", "3"]])).tolist() == [0, 0]
    with pytest.raises(ValueError, match="no token"):
        ItemsetQueries.from_lists([["1"], []])
    with pytest.raises(ValueError, match="strategy"):
        count_itemsets(shard, ItemsetQueries.from_lists([["1"]]), strategy="rows")


def test_limits_export_matches_the_plan(native):
    from fastapriori_amd.ops import primitives as prim
    L = prim.query_limits()
    assert L.kQThreads == 1024 and L.kQAcc >= 1025 and L.kQMaxItems < L.kQAbsent + 1 == 1 << 16
    assert L.kQMaxWidth == 16 and L.kQLdsMax == 160 * 1024 and L.kQWinFields == len(prim.QUERY_WIN_FIELDS)
    # the footprint: slab + accumulators + tile offsets, each from a 16-B boundary
    al = lambda b: (b + 15) // 16 * 16
    for n_items, sw, n_q in ((1, 1, 1), (40, 16, 300), (1000, 8, 8192), (7, 2, 3)):
        assert prim.query_window_lds(n_items, sw, n_q) == al(n_items * sw * 8) + al(n_q * 4) + al((64 * sw + 1) * 8)
    # the width rule: the widest of 16, 8, 4, 2, 1 that fits
    for n_items, n_q, lds in ((40, 100, 160 * 1024 - 512), (40, 100, 4096), (2000, 8192, 160 * 1024 - 512),
                              (100, 10, 2000), (100, 10, 1400)):
        fits = [sw for sw in (16, 8, 4, 2, 1) if prim.query_window_lds(n_items, sw, n_q) <= lds]
        assert prim.query_width(n_items, n_q, lds) == (fits[0] if fits else 0)
    assert prim.query_width(10 ** 6, 1, 160 * 1024) == 0


def _random_live_queries(n_used, Q, seed, max_len=4):
    rng = np.random.default_rng(seed)
    rows = [np.sort(rng.choice(n_used, size=int(rng.integers(1, max_len + 1)), replace=False)) for _ in range(Q)]
    off = np.zeros(Q + 1, dtype=np.int64)
    off[1:] = np.cumsum([len(r) for r in rows])
    return off, np.concatenate(rows).astype(np.int32), rows


@pytest.mark.parametrize("acc", [1, 3, 1025, 0])
def test_plan_properties(native, acc):
    from fastapriori_amd.ops import primitives as prim
    L = prim.query_limits()
    n_used, Q = 50, 2100
    off, idx, rows = _random_live_queries(n_used, Q, seed=acc)
    index = np.arange(Q, dtype=np.int64)[::-1].copy()               # places: the reverse order
    lds = 160 * 1024 - 512
    plan = prim.query_plan(off, idx, index, n_used, Q, acc=acc, lds=lds)
    wins = plan["wins"].numpy()
    F = {n: i for i, n in enumerate(prim.QUERY_WIN_FIELDS)}
    cap = acc or L.kQAcc
    assert len(wins) >= -(-Q // cap) and wins[:, F["n_q"]].sum() == Q
    perm = plan["perm"].numpy()[:Q]
    assert sorted(perm.tolist()) == list(range(Q))                  # a bijection: every live query once
    tab, qoff, qrow = plan["tab"].numpy(), plan["qoff"].numpy(), plan["qrow"].numpy()
    seen_in = {}
    for w in wins:
        n_q, n_items, sw = int(w[F["n_q"]]), int(w[F["n_items"]]), int(w[F["sw"]])
        assert 1 <= n_q <= cap and 1 <= n_items <= L.kQMaxItems and sw in (16, 8, 4, 2, 1)
        assert prim.query_window_lds(n_items, sw, n_q) <= lds
        assert sw == prim.query_width(n_items, n_q, lds)
        t = tab[w[F["tab_off"]]:w[F["tab_off"]] + n_used]
        inside = np.flatnonzero(t != L.kQAbsent)
        assert len(inside) == n_items and sorted(t[inside].tolist()) == list(range(n_items))
        inv = np.empty(n_items, dtype=np.int64)
        inv[t[inside]] = inside                                     # slab row -> used index
        qo = qoff[w[F["qoff_off"]]:w[F["qoff_off"]] + n_q + 1]
        for i in range(n_q):
            r = qrow[w[F["qrow_off"]] + qo[i]:w[F["qrow_off"]] + qo[i + 1]]
            place = int(perm[w[F["q_base"]] + i])
            assert sorted(inv[r].tolist()) == rows[Q - 1 - place].tolist()
        for u in inside.tolist():
            seen_in.setdefault(u, 0)
            seen_in[u] += 1
    if len(wins) > 1:
        assert max(seen_in.values()) > 1                            # an item shared by windows


@pytest.mark.parametrize("acc", [1, 3, 1025])
def test_items_shared_by_windows_count_in_each(native, tune, acc):
    from fastapriori_amd import ItemsetQueries, count_itemsets
    from fastapriori_amd.models import oracle
    from fastapriori_amd.utils.io import parse_bytes
    text, lines, voc = _db("numeric", n=300, seed=5)
    qs = [list(c) for c in itertools.combinations(voc[:48], 2)][:1100] + [[voc[0]]] * 3
    tune(query_acc=acc)
    got = count_itemsets(parse_bytes(text.encode()), ItemsetQueries.from_lists(qs))
    assert got.tolist() == oracle.count_itemsets(lines, qs)


def test_oversize_query_raises(native, tune):
    from fastapriori_amd import ItemsetQueries, count_itemsets
    from fastapriori_amd.ops import primitives as prim
    from fastapriori_amd.utils.io import parse_bytes
    voc = [str(i) for i in range(300)]
    shard = parse_bytes((" ".join(voc) + "\n").encode())
    q = ItemsetQueries.from_lists([voc[:200], voc])
    assert count_itemsets(shard, q).tolist() == [1, 1]
    tune(query_lds_bytes=prim.query_window_lds(250, 1, 1))          # room for 250 items beside one query
    with pytest.raises(ValueError, match=r"query 1 has 300 distinct items.*at most 250"):
        count_itemsets(shard, q)
    assert count_itemsets(shard, ItemsetQueries.from_lists([voc[:250]])).tolist() == [1]
    with pytest.raises(ValueError, match="kQAcc"):
        prim.query_plan(np.zeros(1, np.int64), np.zeros(0, np.int32), np.zeros(0, np.int64), 0, 0,
                        acc=prim.query_limits().kQAcc + 1)
    with pytest.raises(ValueError, match="kQLdsMax"):
        prim.query_plan(np.zeros(1, np.int64), np.zeros(0, np.int32), np.zeros(0, np.int64), 0, 0,
                        lds=prim.query_limits().kQLdsMax + 1)


def test_cpu_path_refuses_windows_outside_the_limits(native):
    import torch
    from fastapriori_amd.ops import primitives as prim
    off, idx, _ = _random_live_queries(10, 5, seed=0)
    plan = prim.query_plan(off, idx, np.arange(5), 10, 5)
    offsets, items = torch.tensor([0, 2], dtype=torch.int64), torch.tensor([0, 1], dtype=torch.int32)
    lut = torch.arange(10, dtype=torch.int32)
    assert prim.query_count(offsets, items, lut, plan).numel() == 5
    bad = dict(plan, wins=plan["wins"].clone())
    bad["wins"][0, prim.QUERY_WIN_FIELDS.index("sw")] = 3
    with pytest.raises(ValueError, match="limits"):
        prim.query_count(offsets, items, lut, bad)


# ---------------------------------------------------------------------------
# end to end: a mined result recounted, and infrequent sets
def _q20k(tmp_path_factory):
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, os.path.join(root, "tests", "fixtures"))
    from make_oracle_fixture import MIN_SUPPORT, write_inputs
    d = str(tmp_path_factory.mktemp("q20k")) + "/"
    write_inputs(d)
    return d, MIN_SUPPORT


@pytest.fixture(scope="module")
def q20k(tmp_path_factory):
    return _q20k(tmp_path_factory)


def check_mined_recount(d: str, ms: float, device: str):
    """Mine <d>D.dat on ``device``; the recount of every itemset of >= 2 items equals the
    mined counts, and a sample of infrequent 3-sets built from frequent pairs counts below
    min_count and equal to brute force.  (Shared with the GPU file.)"""
    import torch
    from fastapriori_amd import ItemsetQueries, count_itemsets, mine
    from fastapriori_amd.models import oracle
    from fastapriori_amd.models.query import result_counts
    from fastapriori_amd.parallel.comm import Comm
    from fastapriori_amd.utils.io import read_shard
    from fastapriori_amd.utils.jvm import java_split_ws
    shard = read_shard(d + "D.dat", Comm(device=torch.device(device)))
    res = mine(shard, ms)
    q = ItemsetQueries.from_result(res, min_size=2)
    assert q.n_queries == res.n_itemsets - len(res.counts[0]) > 20000
    got = count_itemsets(shard, q)
    assert np.array_equal(got, result_counts(res, min_size=2))
    # infrequent 3-sets: two frequent pairs sharing an item whose union was not mined
    f3 = {frozenset(r) for r in res.levels[2].tolist()}
    pairs = res.levels[1].tolist()
    by_first: dict = {}
    for a, b in pairs:
        by_first.setdefault(a, []).append(b)
    rare = []
    for a, bs in by_first.items():
        for b, c in itertools.combinations(bs, 2):
            if frozenset((a, b, c)) not in f3:
                rare.append([res.items[a], res.items[b], res.items[c]])
    rare = rare[::max(1, len(rare) // 200)][:200]
    assert len(rare) >= 100
    got = count_itemsets(shard, ItemsetQueries.from_lists(rare)).tolist()
    lines = [java_split_ws(l) for l in open(d + "D.dat").read().splitlines()]
    assert got == oracle.count_itemsets(lines, rare)
    assert max(got) < res.min_count
    return res


def test_mined_itemsets_recount_to_their_counts(native, q20k):
    check_mined_recount(q20k[0], q20k[1], "cpu")


# ---------------------------------------------------------------------------
# ranks
def _rank_counts(path, qlists, strategy, device, knobs):
    import torch
    from fastapriori_amd import ItemsetQueries, count_itemsets
    from fastapriori_amd.parallel.comm import Comm, init_comm, shutdown_comm
    from fastapriori_amd.tuning import override
    from fastapriori_amd.utils.io import read_shard
    comm = init_comm(device)
    try:
        shard = read_shard(path, comm if strategy == "count" else Comm(device=comm.device))
        with override(**knobs):
            got = count_itemsets(shard, ItemsetQueries.from_lists(qlists), comm, strategy)
        return got.tolist(), shard.n_lines
    finally:
        shutdown_comm(comm)


def ranks_case(tmp_path, mode):
    """A database whose last third is one long line, so the last rank of 3 starts inside
    it and holds an empty shard; (path, queries, expected counts)."""
    from fastapriori_amd.models import oracle
    text, lines, voc = _db(mode, n=240, seed=9)
    long_line = " ".join(voc * 60)
    text += long_line + "\n"
    lines = lines + [long_line.split(" ")]
    p = tmp_path / f"D_{mode}.dat"
    p.write_bytes(text.encode("utf-8"))
    qs = _queries(voc, lines, seed=4)
    return str(p), qs, oracle.count_itemsets(lines, qs)


@pytest.mark.parametrize("strategy", ["count", "candidate"])
@pytest.mark.parametrize("world,mode", [(1, "dict"), (2, "dict"), (3, "dict"), (3, "numeric")])
def test_ranks_agree(native, tmp_path, world, strategy, mode):
    path, qs, want = ranks_case(tmp_path, mode)
    outs = spawn_local(_rank_counts, world, path, qs, strategy, "cpu", {"query_acc": 50})
    for got, _ in outs:
        assert got == want
    if strategy == "count" and world == 3:
        assert outs[-1][1] == 0                                      # the empty shard took the collective


# ---------------------------------------------------------------------------
# the command line
@pytest.fixture(scope="module")
def job_dir(tmp_path_factory):
    d = tmp_path_factory.mktemp("job")
    rng = random.Random(3)
    words = ["apple", "bread", "milk", "tea", "jam", "é"]
    rows = [" ".join(rng.sample(words, rng.randint(1, 4))) for _ in range(60)] + ["", "tea tea milk"]
    (d / "D.dat").write_text("\n".join(rows) + "\n", encoding="utf-8")
    (d / "U.dat").write_text("apple\nmilk tea\n", encoding="utf-8")
    (d / "q.dat").write_text("milk tea\ntea milk tea\n\napple\nnothing milk\njam bread apple\n", encoding="utf-8")
    return d, rows


def _expected_lines(rows, qtext):
    from fastapriori_amd.models import oracle
    from fastapriori_amd.utils.jvm import java_split_ws
    qs = [java_split_ws(l) for l in qtext.splitlines()]
    cnt = oracle.count_itemsets([java_split_ws(r) for r in rows], qs)
    return [" ".join(dict.fromkeys(q)) + f"[{c}]" for q, c in zip(qs, cnt)]


def test_cli_count_only_writes_only_the_counts(native, job_dir, capsys):
    from fastapriori_amd.pipeline import main
    d, rows = job_dir
    out = d / "only"
    out.mkdir()
    assert main([f"{d}/", f"{out}/", f"{out}/tmp", "--count-itemsets", str(d / "q.dat"), "--count-only",
                 "--device", "cpu"]) == 0
    assert sorted(os.listdir(out)) == ["itemsetCounts"]
    assert sorted(os.listdir(out / "itemsetCounts")) == ["_SUCCESS", "part-00000"]
    got = (out / "itemsetCounts" / "part-00000").read_text(encoding="utf-8").splitlines()
    want = _expected_lines(rows, (d / "q.dat").read_text(encoding="utf-8"))
    assert got == want
    assert got[2].startswith("[") and got[1].startswith("tea milk[") and got[4] == "nothing milk[0]"
    assert "==== Total time for get itemsetCounts " in capsys.readouterr().out
    # an existing directory is refused without --overwrite and replaced with it
    from fastapriori_amd.utils.io import OutputExistsError
    with pytest.raises((OutputExistsError, RuntimeError), match="already exists"):
        main([f"{d}/", f"{out}/", "--count-itemsets", str(d / "q.dat"), "--count-only", "--device", "cpu"])
    (d / "q2.dat").write_text("jam\n", encoding="utf-8")
    assert main([f"{d}/", f"{out}/", "--count-itemsets", str(d / "q2.dat"), "--count-only", "--device", "cpu",
                 "--overwrite"]) == 0
    assert (out / "itemsetCounts" / "part-00000").read_text().splitlines() == _expected_lines(rows, "jam\n")


def test_job_counts_and_verifies_beside_the_mining(native, job_dir, capsys):
    from fastapriori_amd.config import JobConfig
    from fastapriori_amd.pipeline import run_job
    d, rows = job_dir
    s = run_job(JobConfig(input=f"{d}/", output=f"{d}/full_", min_support=0.1, device="cpu",
                          count_itemsets=str(d / "q.dat"), verify_counts=True, metrics_path=str(d / "m.jsonl")))
    mined = (d / "full_freqItemset" / "part-00000").read_text(encoding="utf-8").splitlines()
    assert s["n_counted"] == 6 and s["n_verified"] == sum(1 for l in mined if " " in l) > 0
    assert os.path.exists(d / "full_recommends")
    got = (d / "full_itemsetCounts" / "part-00000").read_text(encoding="utf-8").splitlines()
    assert got == _expected_lines(rows, (d / "q.dat").read_text(encoding="utf-8"))
    text = capsys.readouterr().out
    assert f"==== verified {s['n_verified']} itemset counts" in text
    import json
    phases = [json.loads(l).get("phase") for l in open(d / "m.jsonl")]
    assert "count_itemsets" in phases and "verify_counts" in phases


def test_verify_counts_names_the_first_wrong_itemset(native, job_dir, monkeypatch):
    from fastapriori_amd import pipeline
    from fastapriori_amd.config import JobConfig
    d, _ = job_dir
    real = pipeline.mine_window

    def tampered(*a, **k):
        res = real(*a, **k)
        res.counts[1][0] += 1
        return res

    monkeypatch.setattr(pipeline, "mine_window", tampered)
    with pytest.raises(RuntimeError, match=r"--verify-counts: itemset \{.+\} was mined with count \d+ but \d+ lines"):
        pipeline.run_job(JobConfig(input=f"{d}/", output=f"{d}/bad_", min_support=0.1, device="cpu",
                                   verify_counts=True))


@pytest.mark.parametrize("argv,msg", [
    (["--count-only"], "--count-only requires --count-itemsets"),
    (["--count-itemsets", "q", "--rules-only"], "--count-itemsets cannot be combined with --rules-only"),
    (["--count-itemsets", "q", "--count-only", "--rules-only"], "cannot be combined with --rules-only"),
    (["--verify-counts", "--rules-only"], "--verify-counts cannot be combined with --rules-only"),
    (["--count-itemsets", "q", "--count-only", "--verify-counts"],
     "--verify-counts cannot be combined with --count-only"),
])
def test_argument_errors(argv, msg, capsys):
    from fastapriori_amd.config import parse_args
    with pytest.raises(SystemExit):
        parse_args(["in/", "out/"] + argv)
    assert msg in capsys.readouterr().err


def test_missing_query_file_fails_on_every_rank(native, job_dir):
    from fastapriori_amd.config import JobConfig
    from fastapriori_amd.pipeline import run_job
    d, _ = job_dir
    with pytest.raises(RuntimeError, match="--count-itemsets: reading .* failed on rank 0"):
        run_job(JobConfig(input=f"{d}/", output=f"{d}/miss_", device="cpu", count_itemsets=str(d / "none.dat"),
                          count_only=True))
