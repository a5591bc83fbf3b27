"""Edge shapes of the ranked top-N kernels: k_recommend_topn / k_recommend_topn_indexed /
fa_recommend_topn_cpu.

In the style of section 6 of test_kernel_edges.py: rules and baskets are built on purpose,
the planted baskets hold reserved high items only, so they meet exactly the planted rules
(every random rule needs a low item), and the builder asserts which rule ids fire and which
are expected.  The expectation is the brute force below over the Python rule list, never
another path of this project; every comparison is exact equality over the whole [M, N] output.
"""
import functools

import numpy as np
import pytest
import torch

from fastapriori_amd import ops
from fastapriori_amd.ops import primitives as prim
from test_kernel_edges import _rules_tensors

BOTH = ["cpu", pytest.param("cuda", marks=pytest.mark.gpu)]
N_RESERVED = 14


def _firing(rules, basket):
    """Ids of the rules whose antecedent is inside the basket and whose consequent is not."""
    have = set(basket)
    return [r for r, (ante, cons) in enumerate(rules) if set(ante) <= have and cons not in have]


def _top(rules, basket, n):
    """The reference: the first n firing rules with pairwise distinct consequents, -1 padded."""
    out, seen = [], set()
    for r in _firing(rules, basket):
        if len(out) < n and rules[r][1] not in seen:
            seen.add(rules[r][1])
            out.append(r)
    return out + [-1] * (n - len(out))


@functools.lru_cache(maxsize=None)
def _topn_table(R, F1):
    """(rules [(antecedent ascending, consequent)], baskets, names).  Random rules live on the
    low items [0, lo); the 14 highest items are the planted rules' antecedents (their
    consequents are low items, which no planted basket holds unless it says so)."""
    rng = np.random.default_rng(900 + 1000 * R + F1)
    lo = F1 - N_RESERVED
    a0, a1, b0, b1, c0, n0, q0, q1, q2, q3, q4, q5, q6, h = range(lo, F1)
    assert lo >= 9

    def rand_rule():
        it = rng.choice(lo, int(rng.integers(2, 5)), replace=False)
        return tuple(sorted(it[1:].tolist())), int(it[0])

    rules = [rand_rule() for _ in range(R)]
    baskets, names = [], []

    def add(name, items, fire=None, top=None):
        """fire: the rule ids that must fire; top: the whole unbounded list expected."""
        names.append(name)
        baskets.append(sorted(set(items)))
        if fire is not None:
            assert _firing(rules, baskets[-1]) == fire, (name, _firing(rules, baskets[-1]))
        if top is not None:
            assert [r for r in _top(rules, baskets[-1], R) if r >= 0] == top, name

    if R == 1:
        rules[0] = ((a0,), 0)
        add("match", [a0], [0], [0])
        add("consequent in the basket", [a0, 0], [], [])
    else:
        assert R >= 64
        b2 = 64 if R == 65 else 192            # B's second rule: the first id of a later step
        # A: two firing rules of one consequent inside a step, then a new consequent
        rules[2], rules[5], rules[9] = ((a0,), 0), ((a1,), 0), ((a0, a1), 1)
        # B: the same consequent firing in step 0 and again in a later step
        rules[3] = ((b0,), 2)
        if R >= 65:
            rules[b2] = ((b1,), 2)
        if R >= 200:
            rules[195] = ((b0, b1), 3)
        # C: rule 7 takes item 4; rules 12 (197) need 4 in the basket itself
        rules[7], rules[12] = ((c0,), 4), ((4, c0), 5)
        if R >= 200:
            rules[197] = ((4, c0), 6)
        # indexed: q1's list, visited after q0's, lowers consequent 7 from rule 30 to rule 11
        rules[30], rules[11] = ((q0,), 7), ((q1,), 7)
        # indexed: q2's list fills the buffer (rules 40..45), q3's list brings rule 20 with a new
        # consequent (the worst entry leaves), q4's list brings back consequents 4, 1, 0 -- kept,
        # evicted or never admitted, by N -- under the ids 13, 14, 15
        for k in range(6):
            rules[40 + k] = ((q2,), k)
        rules[20] = ((q3,), 6)
        rules[13], rules[14], rules[15] = ((q4,), 4), ((q4,), 1), ((q4,), 0)
        # indexed: q6's list starts at rule 50, past rule 25 of q5's: skipped by a full buffer
        # (N = 1), scanned by one with room
        rules[25], rules[50] = ((q5,), 0), ((q6,), 1)
        if R >= 200:
            # the hub: 128 rules end in h and fill steps 1 and 2 (its list spans two steps, too)
            for k in range(128):
                rules[64 + k] = ((h,), k % lo)

        add("same consequent twice in a step, then a new one", [a0, a1], [2, 5, 9], [2, 9])
        add("antecedent longer than the basket", [a0], [2], [2])
        if R >= 65:
            add("same consequent again in a later step", [b0, b1], [3, b2] + [195] * (R >= 200),
                [3] + [195] * (R >= 200))
            add("entries in two steps", [a0, a1, b1], [2, 5, 9, b2], [2, 9, b2])
            add("only a later step fires", [b1], [b2], [b2])
        add("taken consequent is not in the basket", [c0], [7], [7])
        add("that item in the basket", [4, c0])          # low item 4: random rules may fire, too
        assert 12 in _firing(rules, baskets[-1]) and 7 not in _firing(rules, baskets[-1])
        add("later list lowers a kept consequent", [q0, q1], [11, 30], [11])
        add("later lists evict, re-admit and lower", [q2, q3, q4], [13, 14, 15, 20] + list(range(40, 46)),
            [13, 14, 15, 20, 42, 43, 45])
        assert _top(rules, baskets[-1], 5) == [13, 14, 15, 20, 42] and _top(rules, baskets[-1], 2) == [13, 14]
        add("list head past the kept id", [q5, q6], [25, 50], [25, 50])
        add("first list only", [q2], list(range(40, 46)), list(range(40, 46)))
        if R >= 200:
            add("hub alone", [h], list(range(64, 192)))
            add("hub, three consequents in the basket", [h, 0, 1, 2])
            assert not {64, 65, 66} & set(_firing(rules, baskets[-1]))
            add("hub after step 0", [h, a0, a1])
            assert _top(rules, baskets[-1], 5)[:2] == [2, 9]
            if F1 == 200:
                # >= 100 firing rules with distinct consequents, steps 1 and 2 firing in all 64 lanes
                assert lo >= 128 and len({rules[r][1] for r in range(64, 192)}) == 128
                assert _top(rules, [h], 64) == list(range(64, 128))
    add("no rule", [n0], [], [])
    add("empty", [], [], [])
    add("all items", range(F1), [], [])
    Bk = (rng.random((6, F1)) < 0.3).astype(np.int64)
    for x in range(6):
        add(f"random {x}", np.flatnonzero(Bk[x]).tolist())
    assert all(len(a) >= 1 and list(a) == sorted(set(a)) and c not in a for a, c in rules)
    return rules, baskets, names


@pytest.mark.parametrize("dev", BOTH)
@pytest.mark.parametrize("indexed", [False, True], ids=["scan", "indexed"])
@pytest.mark.parametrize("M", [1, 5])
@pytest.mark.parametrize("N", [1, 2, 5, 64])
@pytest.mark.parametrize("F1", [33, 70, 200])
@pytest.mark.parametrize("R", [1, 64, 65, 200])
def test_recommend_topn(native, R, F1, N, M, indexed, dev):
    rules, baskets, names = _topn_table(R, F1)
    want = [_top(rules, b, N) for b in baskets]
    assert any(w[0] < 0 for w in want) and any(w[0] >= 0 for w in want)
    if R >= 64 and N > 1:
        assert any(w[N - 1] >= 0 for w in want) == (N < 64 or (R, F1) == (200, 200))     # a full list
        assert any(w[0] >= 0 and w[N - 1] < 0 for w in want)                             # a padded one
    ante_off, ante, cons = _rules_tensors(rules, dev)
    index = prim.recommend_index(ante_off, ante, F1) if indexed else None
    if indexed and R >= 200:
        assert int(torch.diff(index[0]).max()) > 64          # one item's list holds > 64 rules
    cons_l = [c for _, c in rules]
    # M baskets per call (one wave each, 4 waves a workgroup); the last call wraps round
    K = len(baskets)
    for k0 in range(0, K, M):
        ids = [(k0 + j) % K for j in range(M)]
        boff = np.zeros(M + 1, np.int64)
        np.cumsum([len(baskets[i]) for i in ids], out=boff[1:])
        bask = np.array([x for i in ids for x in baskets[i]], np.int32)
        boff_t, bask_t = torch.from_numpy(boff).to(dev), torch.from_numpy(bask).to(dev)
        got = ops.recommend_topn(ante_off, ante, cons, F1, boff_t, bask_t, N, index=index)
        assert got.dtype == torch.int32 and tuple(got.shape) == (M, N) and got.device.type == dev
        got = got.cpu().tolist()
        assert got == [want[i] for i in ids], [names[i] for i in ids]
        # column 0 is the rule behind the first-match recommendation
        first = ops.recommend(ante_off, ante, cons, F1, boff_t, bask_t, index=index).cpu().tolist()
        assert [cons_l[g[0]] if g[0] >= 0 else -1 for g in got] == first


@pytest.mark.parametrize("n", [0, 65, -1])
def test_n_out_of_range(native, n):
    rules, baskets, _ = _topn_table(64, 33)
    ante_off, ante, cons = _rules_tensors(rules, "cpu")
    boff, bask = torch.tensor([0, len(baskets[0])]), torch.tensor(baskets[0], dtype=torch.int32)
    for index in (None, prim.recommend_index(ante_off, ante, 33)):
        with pytest.raises(ValueError):
            ops.recommend_topn(ante_off, ante, cons, 33, boff, bask, n, index=index)


@pytest.mark.gpu
@pytest.mark.parametrize("n", [0, 65])
def test_launchers_refuse_n_out_of_range(n):
    # the launchers return before they look at a pointer
    lib = ops._native.hip()
    assert lib.fa_hip_recommend_topn(None, None, None, 1, 33, None, None, 1, n, None, None) != 0
    assert lib.fa_hip_recommend_topn_indexed(None, None, None, None, None, 1, 33, None, None, 1, n, None,
                                             None) != 0


def test_empty_inputs(native):
    rules, baskets, _ = _topn_table(64, 33)
    ante_off, ante, cons = _rules_tensors(rules, "cpu")
    boff, bask = torch.tensor([0, 2, 2]), torch.tensor(baskets[0][:2], dtype=torch.int32)
    none = tuple(torch.zeros(k, dtype=t) for k, t in ((1, torch.int64), (0, torch.int32), (0, torch.int32)))
    assert ops.recommend_topn(*none, 33, boff, bask, 3).tolist() == [[-1] * 3] * 2          # R = 0
    assert tuple(ops.recommend_topn(ante_off, ante, cons, 33, boff[:1], bask[:0], 3).shape) == (0, 3)   # M = 0
