"""The corpus of tests/small_dbs.py on the CPU: every entry mined by the C++ CPU miner equals
the brute-force oracle, and meets the expectations that say what it is there to exercise --
checked here, without a GPU, before tests/test_gpu_small_dbs.py relies on the corpus.

The comparison (``compare``) is exact: min_count, the items in rank order, the token-set
dictionary; and, because ``as_dict()`` would hide a duplicated row, every level's rows
strictly ascending in lexicographic order, every row strictly ascending within itself, and
as many rows as dictionary entries.
"""
import functools

import numpy as np
import pytest

from fastapriori_amd.models.apriori import FastApriori, MinerConfig
from fastapriori_amd.models.oracle import mine as oracle_mine
from fastapriori_amd.utils.io import parse_bytes
from fastapriori_amd.utils.jvm import java_split_ws
from fastapriori_amd.utils.metrics import Logger
from small_dbs import BY_NAME, CORE, ENTRIES, F1_EDGES, SLAB_EDGE_T, SLOW_CPU
from test_miner_property import token_sets


@functools.lru_cache(maxsize=None)
def oracle(name: str):
    """(OracleResult, its token-set dictionary, the oracle branch taken) of entry ``name``:
    computed once, shared by every test, never changed."""
    e = BY_NAME[name]
    lines = [java_split_ws(l) for l in e.text.decode().splitlines()]
    exp = oracle_mine(lines, e.min_support)
    rank = {t: i for i, t in enumerate(exp.items)}
    longest = max((len({rank[t] for t in toks if t in rank}) for toks in lines), default=0)
    return exp, token_sets(exp.items, exp.itemsets), "brute" if longest <= 16 else "levelwise"


def first_difference(got: dict, want: dict) -> str:
    """The first itemset (by size, then tokens) on which two token-set dictionaries differ."""
    keys = sorted(set(got) | set(want), key=lambda s: (len(s), sorted(s)))
    for s in keys:
        if got.get(s) != want.get(s):
            return f"{sorted(s)}: got {got.get(s)}, oracle {want.get(s)}"
    return "none"


def compare(res, name: str, what: str, max_level: int = 0) -> None:
    """res (a MiningResult) against the oracle of entry ``name``; ``what`` names the run."""
    exp, want, _ = oracle(name)
    if max_level:
        want = {s: c for s, c in want.items() if len(s) <= max_level}
    tag = f"{name} [{what}]"
    assert res.min_count == exp.min_count, tag
    assert list(res.items) == exp.items, tag
    got = token_sets(res.items, res.as_dict())
    assert got == want, f"{tag}: first difference {first_difference(got, want)}"
    for k, (rows, cnt) in enumerate(zip(res.levels, res.counts), 1):
        rows = np.asarray(rows).reshape(-1, k)
        assert len(rows) == len(cnt) and (k == 1 or len(rows) > 0), f"{tag}: level {k}"
        assert k == 1 or (rows[:, 1:] > rows[:, :-1]).all(), f"{tag}: a level-{k} row is not ascending"
        flat = rows.tolist()
        assert all(a < b for a, b in zip(flat, flat[1:])), f"{tag}: level {k} is not strictly lexicographic"
    assert sum(len(l) for l in res.levels) == len(res.as_dict()), f"{tag}: a row appears twice"
    if max_level:
        assert len(res.levels) <= max_level, tag


def check_expectations(name: str) -> None:
    e = BY_NAME[name]
    x = e.expectations
    exp, d, branch = oracle(name)
    sizes = {}
    for s in d:
        sizes[len(s)] = sizes.get(len(s), 0) + 1
    levels = max(sizes, default=0)
    assert branch == x.get("oracle_branch", "brute"), name
    assert sum(sizes.values()) <= 41000, name
    if "levels" in x:
        assert levels == x["levels"], (name, sizes)
    if "min_levels" in x:
        assert levels >= x["min_levels"], (name, sizes)
    if x.get("F1") is not None:
        assert len(exp.items) == x["F1"], name
    if "min_count" in x:
        assert exp.min_count == x["min_count"], name
    if "n_itemsets" in x:
        assert len(d) == x["n_itemsets"], name
    for k, n in x.get("level_sizes", {}).items():
        assert sizes.get(k, 0) == n, (name, k, sizes)
    for k, c in x.get("max_count_ge", {}).items():
        assert max(v for s, v in d.items() if len(s) == k) >= c, (name, k)
    for s, c in x.get("present", {}).items():
        assert d.get(s) == c, (name, sorted(s), d.get(s))
    for s in x.get("rejected", ()):
        assert s not in d and all(s - {t} in d for t in s), (name, sorted(s))
    # the compressed rows, from the text and the oracle's frequent items alone
    freq = set(exp.items)
    kept = [frozenset(t for t in java_split_ws(l) if t in freq) for l in e.text.decode().splitlines()]
    kept = [r for r in kept if len(r) >= 2]
    if "kept_rows" in x:
        assert len(kept) == x["kept_rows"], (name, len(kept))
    if "distinct_rows" in x:
        assert len(set(kept)) == x["distinct_rows"], (name, len(set(kept)))
    if "tail_bundle" in x:
        import math
        t, F1 = x["tail_bundle"], len(exp.items)
        assert sizes[t["first_level"] - 1] == math.comb(F1, t["first_level"] - 1) and t["used"] == F1, name
        assert t["candidates"] == sum(math.comb(F1, k) for k in range(t["first_level"], F1 + 1)), name
    if "trim_loses" in x:
        used = set().union(*[s for s in d if len(s) == 2 and any(s < t for t in d if len(t) == 3)])
        lost = sum(1 for r in kept if len(r & used) < 3)
        assert lost >= x["trim_loses"] * len(kept), (name, lost, len(kept))


def _mine_cpu(e, **cfg):
    m = FastApriori(e.min_support, config=MinerConfig(min_support=e.min_support, **cfg), logger=Logger(enabled=False))
    return m.run(parse_bytes(e.text))


_PARAMS = [pytest.param(e.name, marks=pytest.mark.slow) if e.name in SLOW_CPU else e.name for e in ENTRIES]


@pytest.mark.parametrize("name", _PARAMS)
def test_entry_meets_its_expectations(name):
    check_expectations(name)


@pytest.mark.parametrize("name", _PARAMS)
def test_cpu_miner_equals_oracle(native, name):
    e = BY_NAME[name]
    runs = [dict(dedup="on"), dict(dedup="off"), dict(trim=True, trim_min_rows=0)]
    if e.expectations.get("dedup"):
        runs.append(dict(dedup=e.expectations["dedup"], trim=True, trim_min_rows=0))
    for cfg in runs:
        compare(_mine_cpu(e, **cfg), name, f"cpu {cfg}")


def test_corpus_shape():
    """The corpus holds the parts it is meant to hold, and its random parts are not vacuous."""
    names = [e.name for e in ENTRIES]
    assert all(f"lattice_n{n}_x{c}" in BY_NAME for n in (2, 3, 4, 10, 13, 15) for c in (1, 3))
    assert all(f"slab_edge_T{T}" in BY_NAME for T in SLAB_EDGE_T)
    assert all(f"f1_edge_{f}" in BY_NAME for f in F1_EDGES)
    assert sum(n.startswith("noise_seed") for n in names) == 30
    assert sum(n.startswith("dense_seed") for n in names) == 40
    assert 18 <= len(CORE) <= 32 and len(set(CORE)) == len(CORE)
    noise = [BY_NAME[n] for n in names if n.startswith("noise_seed")]
    lines = [l for e in noise for l in e.text.decode().splitlines()]
    assert any(l == "" for l in lines)                                       # blank lines
    assert any(len(set(l.split())) < len(l.split()) for l in lines)          # a token twice in a line
    assert any("x" in l.split() and "3" in l.split() for l in lines)         # words beside numbers
    deep = lambda fam: sum(max((len(s) for s in oracle(n)[1]), default=0) >= 4 for n in names if n.startswith(fam))  # noqa: E731
    assert deep("noise_seed") >= 8 and deep("dense_seed") >= 15
    for e in noise:
        exp, d, _ = oracle(e.name)
        freq = set(exp.items)
        rows = [set(l.split()) & freq for l in e.text.decode().splitlines()]
        if any(len(r) < 2 for r in rows) and any(t not in freq for l in e.text.decode().split() for t in [l]):
            break
    else:
        raise AssertionError("no noise entry has both a line that compresses away and a token below support")
