"""The regrouping rule of one-pass device bundles, on its host model (csrc/host/fa_regroup.h,
regroup.cpp; ops.host.dl_regroup): every candidate under one parent that is a (k-1)-subset of
it and a parent row of its level, the extension the item left out, pieces of at most 8,
never more pieces than the generator's prefix groups.

The levels come from the brute-force chains of tests/test_gen_edges.py (parent rows, extensions
per row, candidates), as the device generator leaves them; tests/test_gpu_regroup.py holds the
device step to this model on the same cases.
"""
import functools
import itertools

import numpy as np
import pytest

from fastapriori_amd.ops import host
from fastapriori_amd.ops import primitives as prim
from test_gen_edges import _chain, bundle_case


def _triangles(n):
    rows = []
    for t in range(n):
        a = 3 * t
        rows += [(a, a + 1), (a, a + 2), (a + 1, a + 2)]
    return rows


# id: (F1, chain of (parent rows, extensions per row, candidates), levels of the bundle)
@functools.lru_cache(maxsize=None)
def regroup_case(name):
    if name == "one_candidate":
        return 70, _chain([(0, 1), (0, 2), (1, 2)], 1), 1
    if name == "nine_children":
        # (0, 1) with the extensions 2 .. 10 and no pair among those: nine candidates, each with
        # the parents (0, 1), (0, x), (1, x)
        rows = [(0, 1)] + [(0, x) for x in range(2, 11)] + [(1, x) for x in range(2, 11)]
        return 70, _chain(sorted(rows), 1), 1
    if name == "k5_triples":
        return 70, _chain(list(itertools.combinations(range(5), 2)), 1), 1
    if name == "disjoint":
        return 70, _chain(_triangles(20), 1), 1
    if name == "two_levels":
        return 70, _chain(list(itertools.combinations(range(9), 2)), 2), 2
    if name == "rows528":
        F1, ch = bundle_case("lat33_F70", 1)
        return F1, ch, 1
    if name == "rows12300":
        # 4,100 triangles apart: 12,300 parent rows, past the rows a level may regroup with
        return 12300, _chain(_triangles(4100), 1), 1
    if name == "m11_m12":
        F1, ch = bundle_case("lat15_F70_m11", 4)
        return F1, ch[:2], 2
    if name == "m12_m13":
        F1, ch = bundle_case("lat15_F70_m11", 4)
        return F1, ch[1:3], 2
    raise KeyError(name)


CASES = ["one_candidate", "nine_children", "k5_triples", "disjoint", "two_levels", "rows528", "rows12300", "m11_m12",
         "m12_m13"]


def model_levels(ch, L):
    return [(rows, cnt, cand[:, -1]) for rows, cnt, cand in ch[:L]]


def pieces(cnt):
    return int(((np.asarray(cnt, dtype=np.int64) + 7) // 8).sum())


def check_level(rows, cnt, cand, o):
    """One regrouped level against the rule's invariants."""
    n, m = rows.shape
    C = len(cand)
    assert o["cnt"].shape == (n,) and int(o["cnt"].sum()) == C
    assert np.array_equal(o["off"], np.concatenate([[0], np.cumsum(o["cnt"])]))
    assert np.array_equal(np.sort(o["perm"]), np.arange(C))          # every candidate exactly once
    owner = np.repeat(np.arange(n), o["cnt"])
    for new in range(C):
        p, y, old = rows[owner[new]], int(o["ex"][new]), cand[o["perm"][new]]
        assert y not in p and sorted(list(p) + [y]) == list(old), (new, p, y, old)
    for i in range(n):                                                # candidate order inside a parent
        seg = o["perm"][o["off"][i]:o["off"][i + 1]]
        assert np.all(np.diff(seg) > 0)
    # pieces are cut 8 extensions at a time from a parent's list: never more than the prefix plan
    assert o["pieces_prefix"] == pieces(cnt)
    assert pieces(o["cnt"]) == min(o["pieces_rule"], o["pieces_prefix"]) <= pieces(cnt)
    assert o["kept_prefix"] == int(o["pieces_rule"] >= o["pieces_prefix"])
    if o["kept_prefix"]:
        assert np.array_equal(o["cnt"], cnt) and np.array_equal(o["perm"], np.arange(C))
        assert np.array_equal(o["ex"], cand[:, -1])


@pytest.mark.parametrize("case", CASES)
def test_rule_invariants(native, case):
    _, ch, L = regroup_case(case)
    regrouped, out = host.dl_regroup(model_levels(ch, L))
    assert regrouped == (case != "m12_m13")
    for (rows, cnt, cand), o in zip(ch[:L], out):
        check_level(rows, cnt, cand, o)
        if not regrouped:
            assert o["kept_prefix"] == 1 and o["rounds"] == 0
    again = host.dl_regroup(model_levels(ch, L))
    assert again[0] == regrouped
    for a, b in zip(out, again[1]):
        assert all(np.array_equal(a[k], b[k]) for k in a)


def test_rounds_alone_do_not_lose_to_the_prefix_plan(native):
    """Before the fallback: on the lattices and cliques here the rounds themselves give no more
    pieces than the prefix groups (the fallback is for inputs where they would)."""
    for case in CASES:
        _, ch, L = regroup_case(case)
        for o in host.dl_regroup(model_levels(ch, L))[1]:
            assert o["pieces_rule"] <= o["pieces_prefix"], case


def test_rule_shapes(native):
    """The cases' own figures: what each of them is there to reach."""
    got = {}
    for case in CASES:
        _, ch, L = regroup_case(case)
        got[case] = host.dl_regroup(model_levels(ch, L))[1]
    assert len(regroup_case("one_candidate")[1][0][2]) == 1 and pieces(got["one_candidate"][0]["cnt"]) == 1
    nine = got["nine_children"][0]
    assert len(regroup_case("nine_children")[1][0][2]) == 9 and pieces(nine["cnt"]) == 2
    k5 = got["k5_triples"][0]
    assert k5["pieces_prefix"] == 6 and pieces(k5["cnt"]) <= 4 and not k5["kept_prefix"]
    dj = got["disjoint"][0]
    assert dj["kept_prefix"] and pieces(dj["cnt"]) == 20
    two = regroup_case("two_levels")[1]
    assert [r.shape[1] for r, _, _ in two[:2]] == [2, 3] and all(not o["kept_prefix"] for o in got["two_levels"])
    assert regroup_case("rows528")[1][0][0].shape[0] == 528 > 256 and not got["rows528"][0]["kept_prefix"]
    K = prim.dl()
    assert [r.shape[1] for r, _, _ in regroup_case("m11_m12")[1]] == [11, 12] and K.kDlInline == 12
    assert [r.shape[1] for r, _, _ in regroup_case("m12_m13")[1]] == [12, 13]
    big = got["rows12300"][0]
    assert regroup_case("rows12300")[1][0][0].shape[0] == 12300 > host._native.host().fa_dl_regroup_const(0) == 12288
    assert big["kept_prefix"] and big["rounds"] == 0 and big["pieces_prefix"] == big["pieces_rule"] == 4100
    assert not got["m11_m12"][1]["kept_prefix"]        # m = 12 regroups ...
    assert all(o["kept_prefix"] for o in got["m12_m13"])   # ... a bundle with m = 13 keeps the prefix plan
