"""A corpus of small adversarial transaction databases, each cheap enough for the brute-force
oracle (models.oracle.mine: every subset of every distinct row), for the miner as a whole --
the composition of kernels in FastApriori._mine_device_loop, which the kernels' own edge
tests do not reach.

``ENTRIES`` is a list of ``Entry(name, text, min_support, expectations)``; ``BY_NAME`` indexes
it.  Everything is deterministic: random entries draw from ``numpy.random.default_rng`` with a
fixed seed.  Unless an entry says ``oracle_branch="levelwise"``, every row compresses to at
most 16 frequent items, so the oracle takes its brute-force branch.

``expectations`` says what the entry is there to exercise; tests/test_small_dbs.py asserts it
against the oracle's result, so an entry that drifts away from its purpose fails:

  levels / min_levels   number of levels with a frequent itemset (exactly / at least)
  F1                    number of frequent items
  min_count             the support threshold in rows
  n_itemsets            frequent itemsets of every size
  level_sizes           {k: |F_k|}
  max_count_ge          {k: c}: some k-itemset has a count >= c
  present               {token set: count} that must be frequent with exactly this count
  rejected              token sets that are NOT frequent while every subset one item
                        smaller is: candidates that reach the count and fail the threshold
  kept_rows             rows that keep >= 2 frequent items (the counted columns, dedup off)
  distinct_rows         distinct compressed rows (the weighted layout's columns)
  oracle_branch         "brute" (default) or "levelwise"
  dedup                 the MinerConfig.dedup the entry is meant for (it runs under that too)
  tail_bundle           {first_level, used, candidates}: every itemset of first_level - 1 items
                        is frequent, so the levels from first_level on have C(F1, k) candidates
                        each, `candidates` in all, over `used` items: the run's last bundle
  trim_loses            share of the kept rows that hold fewer than 3 items of level 3's
                        candidates: a forced trim before level 3 drops at least this share

To add an entry: write a builder that returns ``Entry``, give it a name that says what it
pins, state its purpose in ``expectations``, append it in ``_build()``, and add it to ``CORE``
when every device configuration should run it.  ``pytest tests/test_small_dbs.py`` then checks
it on the CPU before any device run depends on it.
"""
from __future__ import annotations

import itertools
from typing import NamedTuple

import numpy as np


class Entry(NamedTuple):
    name: str
    text: bytes
    min_support: float
    expectations: dict


def _text(rows) -> bytes:
    return ("\n".join(" ".join(str(t) for t in r) for r in rows) + "\n").encode()


def _support_for(mc: int, n: int) -> float:
    """A support whose ceil(support * n) is mc, away from the rounding edge."""
    return (mc - 0.5) / n


# ---- (a) full lattices ---------------------------------------------------------------------
def _lattice(n: int, copies: int) -> Entry:
    row = [str(i) for i in range(1, n + 1)]
    import math
    return Entry(f"lattice_n{n}_x{copies}", _text([row] * copies), 1.0,
                 dict(levels=n, F1=n, min_count=copies, n_itemsets=2 ** n - 1,
                      level_sizes={k: math.comb(n, k) for k in range(1, n + 1)},
                      present={frozenset(row): copies}, kept_rows=copies, distinct_rows=1))


# ---- (b) threshold ties at every level -----------------------------------------------------
def _ties(mc: int, filler: int = 0, support: float | None = None, name: str | None = None) -> Entry:
    """Core items 1..5.  For k = 2..6, with P = {1..k-1}: mc rows P + {t_k} (t_k occurs nowhere
    else, so P + {t_k} and every subset holding t_k count exactly mc), mc - 1 rows P + {s_k},
    and one row (P - {i}) + {s_k} per i in P: every (k-1)-subset of P + {s_k} that holds s_k
    counts exactly mc, so P + {s_k} is generated, counted, and fails with mc - 1."""
    rows, present, rejected = [], {}, []
    for k in range(2, 7):
        P = [str(i) for i in range(1, k)]
        t, s = str(60 + k), str(70 + k)
        rows += [P + [t]] * mc + [P + [s]] * (mc - 1)
        rows += [[p for p in P if p != i] + [s] for i in P]
        present[frozenset(P + [t])] = mc
        for i in P:
            present[frozenset([p for p in P if p != i] + [s])] = mc
        rejected.append(frozenset(P + [s]))
    rows += [[str(900 + i)] for i in range(filler)]          # lines that only raise N
    n = len(rows)
    return Entry(name or f"ties_mc{mc}", _text(rows), _support_for(mc, n) if support is None else support,
                 dict(levels=6, F1=15, min_count=mc, present=present, rejected=rejected))


# ---- (c) row counts at slab edges ----------------------------------------------------------
SLAB_EDGE_T = (1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2049)


def _slab_edge(T: int) -> Entry:
    """T dense random rows over 10 items (p = 0.5), every row with at least 5 items so that the
    kept rows are exactly T and one row alone already has 5 levels."""
    rng = np.random.default_rng(7000 + T)
    B = rng.random((T, 10)) < 0.5
    for r in range(T):
        while B[r].sum() < 5:
            B[r] = rng.random(10) < 0.5
    rows = [[str(i + 1) for i in np.flatnonzero(b)] for b in B]
    ms = 1.0 if T == 1 else 0.02
    return Entry(f"slab_edge_T{T}", _text(rows), ms, dict(min_levels=5, kept_rows=T, F1=None if T == 1 else 10))


# ---- (d) counts past the narrow accumulators -----------------------------------------------
def _core_plus_two(T: int) -> Entry:
    """T rows of a core {a, b, c, d} plus 2 of 8 other items, the 28 choices in turn: the core's
    subsets count T (past a byte at 300, past 16 bits at 66,000)."""
    core = ["1", "2", "3", "4"]
    pairs = list(itertools.combinations([str(i) for i in range(11, 19)], 2))
    rows = [core + list(pairs[r % 28]) for r in range(T)]
    return Entry(f"core_plus_two_T{T}", _text(rows), 0.02,
                 dict(levels=6, F1=12, max_count_ge={3: T, 4: T}, present={frozenset(core): T},
                      kept_rows=T, distinct_rows=28, dedup="off"))


# ---- (e) weight classes --------------------------------------------------------------------
def _distinct_rows(n: int, n_items: int = 8):
    """n distinct rows of 3 to 5 items over n_items items, in a fixed order."""
    items = [str(i) for i in range(1, n_items + 1)]
    out = [list(c) for k in (5, 4, 3) for c in itertools.combinations(items, k)]
    assert len(out) >= n
    return out[:n]


def _weights_1_to_70() -> Entry:
    rows = [r for i, r in enumerate(_distinct_rows(70), 1) for _ in range(i)]
    return Entry("weights_1_to_70", _text(rows), 0.02,
                 dict(min_levels=4, F1=8, kept_rows=70 * 71 // 2, distinct_rows=70, dedup="on"))


def _one_class(n: int) -> Entry:
    rows = [r for r in _distinct_rows(n) for _ in range(5)]
    return Entry(f"one_class_{n}_cols", _text(rows), 0.02,
                 dict(min_levels=4, F1=8, kept_rows=5 * n, distinct_rows=n, dedup="on"))


def _heavy_row() -> Entry:
    heavy = ["1", "2", "3", "4"]
    unit = [r for r in _distinct_rows(51, 7) if r != heavy][:50]
    rows = unit[:25] + [heavy] * 70000 + unit[25:]
    n = len(rows)
    return Entry("heavy_row_70000", _text(rows), _support_for(2, n),
                 dict(min_levels=4, F1=7, min_count=2, max_count_ge={4: 70000}, distinct_rows=51,
                      kept_rows=n, dedup="on"))


def _nothing_survives() -> Entry:
    """Two frequent items that never share a row: every row compresses to one item."""
    rows = [["1", "100"], ["1", "101"], ["2", "102"], ["2", "103"], ["104"]]
    return Entry("nothing_survives_compression", _text(rows), _support_for(2, 5),
                 dict(levels=1, F1=2, min_count=2, n_itemsets=2, kept_rows=0, distinct_rows=0, dedup="on"))


# ---- (f) token-level noise -----------------------------------------------------------------
NOISE_TOKENS = [str(i) for i in range(1, 13)] + ["x", "y"]


def _noise(seed: int) -> Entry:
    """The row strategy of tests/test_miner_property.py with a fixed seed: 0 to 9 tokens per line
    drawn with repetition from twelve numbers and two words, so lines repeat tokens (counted
    for F_1 only), are blank (the empty token), hold tokens below support, and compress to
    zero or one item."""
    rng = np.random.default_rng(8000 + seed)
    n = int(rng.integers(1, 401))
    ms = float(rng.choice([0.01, 0.02, 0.05, 0.1, 0.2, 0.34]))
    rows = [[NOISE_TOKENS[j] for j in rng.integers(0, 14, int(rng.integers(0, 10)))] for _ in range(n)]
    return Entry(f"noise_seed{seed}", _text(rows), ms, dict(min_levels=0))


# ---- (g), (h) disjoint triples -------------------------------------------------------------
def _triples(F1: int, mc: int):
    """F1 items in disjoint triples (a leftover pair or single item last), each group repeated
    mc times: every group and its subsets count mc, nothing else is frequent."""
    items = [str(i) for i in range(1, F1 + 1)]
    groups = [items[i:i + 3] for i in range(0, F1, 3)]
    return items, groups, [g for g in groups for _ in range(mc)]


def _long_row() -> Entry:
    items, groups, rows = _triples(80, 3)
    rows.append(items)                                   # one row with all 80 frequent items
    n = len(rows)
    present = {frozenset(g): 4 for g in groups}
    return Entry("long_row_80_items", _text(rows), _support_for(3, n),
                 dict(levels=3, F1=80, min_count=3, level_sizes={1: 80, 2: 26 * 3 + 1, 3: 26},
                      present=present, oracle_branch="levelwise", kept_rows=n))


F1_EDGES = (2, 3, 32, 33, 64, 65, 2048, 2049, 4096, 4097)


def _f1_edge(F1: int) -> Entry:
    items, groups, rows = _triples(F1, 2)
    n2 = sum(len(g) * (len(g) - 1) // 2 for g in groups)
    sizes = {1: F1, 2: n2}
    if F1 >= 3:
        sizes[3] = F1 // 3
    return Entry(f"f1_edge_{F1}", _text(rows), _support_for(2, len(rows)),
                 dict(levels=len(sizes), F1=F1, min_count=2, level_sizes=sizes, n_itemsets=sum(sizes.values()),
                      kept_rows=2 * sum(1 for g in groups if len(g) > 1)))


# ---- (i) seeded random dense databases -----------------------------------------------------
def _dense(seed: int) -> Entry:
    rng = np.random.default_rng(9000 + seed)
    n, n_items = int(rng.integers(1, 401)), int(rng.integers(6, 15))
    dens = float(rng.uniform(0.2, 0.7))
    ms = float(rng.choice([0.02, 0.05, 0.1, 0.2, 0.4]))
    B = rng.random((n, n_items)) < dens
    rows = [[str(i + 1) for i in np.flatnonzero(b)] for b in B]
    return Entry(f"dense_seed{seed}", _text(rows), ms, dict(min_levels=0))


# ---- rows a trim before level 3 drops ------------------------------------------------------
def _trim_sheds() -> Entry:
    """200 dense rows over items 1..6 (deep levels) and 200 rows that hold only a frequent pair
    of other items: those pairs make no triple, so the rows hold no level-3 candidate item
    and a trim before level 3 drops half of the rows."""
    rng = np.random.default_rng(31)
    B = rng.random((200, 6)) < 0.7
    B[B.sum(1) < 3, :3] = True
    rows = [[str(i + 1) for i in np.flatnonzero(b)] for b in B]
    rows += [["21", "22"] if r % 2 else ["23", "24"] for r in range(200)]
    return Entry("trim_sheds_pair_rows", _text(rows), 0.05,
                 dict(min_levels=4, F1=10, kept_rows=400, trim_loses=0.5, present={frozenset(["21", "22"]): 100}))


# ---- levels wider than one accumulator pass; a last bundle wider than u32 accumulators ------
def _all_subsets(n_items: int, size: int, name: str, x: dict) -> Entry:
    """Every `size`-subset of n_items items once, and every third one a second time, at
    min_count 1: every itemset of up to `size` items is frequent, and the levels past `size`
    are generated from candidates and counted as zeros."""
    rows = [list(c) for c in itertools.combinations([str(i) for i in range(1, n_items + 1)], size)]
    rows += rows[::3]
    return Entry(name, _text(rows), _support_for(1, len(rows)), dict(x, levels=size, F1=n_items, min_count=1))


def _wide_level3() -> Entry:
    """C(20, 3) = 1140 candidates at level 3, over the 1024 accumulators a shrunk LDS budget
    leaves at slab width 4: the smallest level that has to be counted window by window."""
    return _all_subsets(20, 4, "wide_level3_1140_candidates", dict(level_sizes={3: 1140, 4: 4845}))


def _wide_tail() -> Entry:
    """Every 8-subset of 16 items: 39,202 frequent itemsets, and from level 6 on 58,651
    candidates in one growth-accepted chain that ends the run -- more than the u32
    accumulators of one pass hold at the default LDS budget, so the tail rule's packed pass
    (thinned row padding, byte accumulators) is what counts them in one bundle."""
    return _all_subsets(16, 8, "wide_tail_all_8_subsets_of_16", dict(level_sizes={5: 4368, 6: 8008, 7: 11440, 8: 12870},
                             tail_bundle=dict(first_level=6, used=16, candidates=58651)))


def _build() -> list[Entry]:
    out = [_lattice(n, c) for n in (2, 3, 4, 10, 13, 15) for c in (1, 3)]
    out += [_ties(1), _ties(2), _ties(7)]
    # 0.07 * 100 is 7.000000000000001 in IEEE double: min_count rounds up to 8
    out.append(_ties(8, filler=10, support=0.07, name="ties_mc8_rounding_0.07x100"))
    out += [_slab_edge(T) for T in SLAB_EDGE_T]
    out += [_core_plus_two(300), _core_plus_two(66000)]
    out += [_weights_1_to_70(), _one_class(64), _one_class(65), _heavy_row(), _nothing_survives()]
    out += [_noise(s) for s in range(30)]
    out.append(_long_row())
    out += [_f1_edge(f) for f in F1_EDGES]
    out += [_dense(s) for s in range(40)]
    out.append(_trim_sheds())
    out += [_wide_level3(), _wide_tail()]
    return out


ENTRIES = _build()
BY_NAME = {e.name: e for e in ENTRIES}
assert len(BY_NAME) == len(ENTRIES)

# the entries whose CPU validation dominates the module's time (marked slow there)
SLOW_CPU = ("f1_edge_4097", "f1_edge_4096", "core_plus_two_T66000", "heavy_row_70000",
            "wide_tail_all_8_subsets_of_16")

# five of the dense random entries: no frequent item at all, 5 levels, 7 rows with 7 levels,
# a full lattice over 14 items, 8 levels
DENSE_CORE = (3, 7, 16, 21, 28)

# the entries every device configuration runs
CORE = (["lattice_n4_x1", "lattice_n10_x3", "lattice_n15_x1"]
        + ["ties_mc1", "ties_mc2", "ties_mc7", "ties_mc8_rounding_0.07x100"]
        + [f"slab_edge_T{T}" for T in (64, 65, 1024, 1025)]
        + ["core_plus_two_T300", "core_plus_two_T66000"]
        + ["weights_1_to_70", "one_class_64_cols", "one_class_65_cols", "heavy_row_70000",
           "nothing_survives_compression"]
        + ["long_row_80_items"]
        + [f"f1_edge_{f}" for f in (3, 65, 4097)]
        + [f"dense_seed{s}" for s in DENSE_CORE]
        + ["trim_sheds_pair_rows", "wide_level3_1140_candidates", "wide_tail_all_8_subsets_of_16"])
assert all(n in BY_NAME for n in CORE)
