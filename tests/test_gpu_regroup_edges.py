"""Edge shapes of the device regrouping step (csrc/hip/regroup.hip: k_dl_rg_parents, the parent
search over all levels; k_dl_rg_rounds, the rounds out of LDS with packed 16-bit counters, a
compacted list of the unassigned candidates and a fallback that reads the lists from global
memory when they do not fit the LDS cap, csrc/host/fa_regroup.h rg_lds_fits).

Every case holds prim.dl_regroup to the host model (ops.host.dl_regroup) field by field -- cnt,
off, extension ids, perm, the four statistics, rounds among them -- and runs the device step
twice.  The levels are the brute-force chains of tests/test_gen_edges.py, laid out in device
memory as the generator leaves them (tests/test_gpu_regroup.py runs the generator itself);
levels are independent, so a bundle here may put any of them side by side.  What a case is
there for is asserted on a plain replay of the rule's rounds (_trace), itself held to the
model's round count and children per parent.
"""
import functools
import itertools

import numpy as np
import pytest
import torch

from fastapriori_amd.ops import _native, host
from fastapriori_amd.ops import primitives as prim
from test_gen_edges import _chain
from test_regroup_rule import CASES, regroup_case

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
THR = (8, 6, 4, 3, 2, 1)


@pytest.fixture(scope="module")
def dl_state():
    return prim.DeviceLevelState(DEV)


def _star(E):
    """(0, 1) with the extensions 2 .. E + 1 and no pair among those: E candidates under one parent."""
    return sorted([(0, 1)] + [(0, x) for x in range(2, E + 2)] + [(1, x) for x in range(2, E + 2)])


@functools.lru_cache(maxsize=None)
def edge_case(name):
    """-> the levels [(parent rows, extensions per row, candidates)] of one bundle."""
    if name in CASES:
        _, ch, L = regroup_case(name)
        return ch[:L]
    if name in ("star256", "star300"):
        return _chain(_star(int(name[4:])), 1)
    if name == "fan300":
        # (x, 400, 401), x < 300: every prefix (x, 400) has one child, the last row (400, 401) all 300
        return _chain(sorted([(x, y) for x in range(300) for y in (400, 401)] + [(400, 401)]), 1)
    if name in ("k6_triples", "k7_triples"):
        return _chain(list(itertools.combinations(range(int(name[1])), 2)), 1)
    if name == "n1_c1":
        # one parent row, one candidate (no generator leaves this: the other parent is not a row)
        return [(np.array([[5]], np.int32), np.array([1], np.int64), np.array([[5, 9]], np.int32))]
    if name == "clique12":
        ch = _chain(list(itertools.combinations(range(12), 2)), 10)
        assert [len(c) for _, _, c in ch] == [220, 495, 792, 924, 792, 495, 220, 66, 12, 1]
        return ch
    if name == "rows12300_k5":
        return edge_case("rows12300") + edge_case("k5_triples")
    if name == "k5_rows12300_two":
        return edge_case("k5_triples") + edge_case("rows12300") + edge_case("two_levels")
    raise KeyError(name)


def _trace(rows, cand):
    """The rule's rounds replayed in plain Python -> ([(thr, votes per parent, parents that took
    their voters)] per round, children per parent at the end of the rounds)."""
    index = {tuple(r): i for i, r in enumerate(rows.tolist())}
    par = [[index.get(tuple(np.delete(c, j).tolist()), -1) for j in range(len(c))] for c in cand]
    asg, out = [-1] * len(cand), []
    for thr in THR:
        while True:
            u, votes, cho = {}, {}, {}
            for c, ps in enumerate(par):
                if asg[c] < 0:
                    for p in ps:
                        if p >= 0:
                            u[p] = u.get(p, 0) + 1
            for c, ps in enumerate(par):
                if asg[c] >= 0:
                    continue
                best, bp = -1, -1
                for p in reversed(ps):
                    if p >= 0 and u[p] >= thr and u[p] > best:
                        best, bp = u[p], p
                cho[c] = bp
                if bp >= 0:
                    votes[bp] = votes.get(bp, 0) + 1
            took = {p for p, x in votes.items() if x >= thr}
            for c, bp in cho.items():
                if bp in took:
                    asg[c] = bp
            out.append((thr, votes, took))
            if not took:
                break
    return out, np.bincount(asg, minlength=len(rows))


def _lay_out(S, levels):
    """The levels in device memory and in S.desc, as the generator leaves them -> the tensors."""
    keep, base = [], 0
    S.desc[:] = 0
    for l, (rows, cnt, cand) in enumerate(levels):
        n, m = rows.shape
        C = len(cand)
        t = dict(P=torch.from_numpy(np.ascontiguousarray(rows, np.int32)).to(DEV),
                 cnt=torch.from_numpy(np.concatenate([cnt, cand[:, -1]]).astype(np.int32)).to(DEV),
                 off=torch.from_numpy(np.concatenate([[0], np.cumsum(cnt)]).astype(np.int64)).to(DEV),
                 rows=torch.from_numpy(np.ascontiguousarray(cand, np.int32)).to(DEV))
        d = S.desc[l]
        for f, x in t.items():
            d[f] = x.data_ptr()
        d["m"], d["n"], d["C"], d["base"] = m, n, C, base
        base += C
        keep.append(t)
    return keep


def _at(buf, ptr, count, dtype):
    o, nb = int(ptr) - buf.data_ptr(), count * np.dtype(dtype).itemsize
    assert 0 <= o and o + nb <= buf.numel()
    return buf[o:o + nb].cpu().numpy().view(dtype)


def _fields(got, levels):
    """The device step's output per level, in the model's form."""
    stats, perm, out, base = got["stats"].cpu().numpy(), got["perm"].cpu().numpy(), [], 0
    for l, (rows, _, cand) in enumerate(levels):
        n, C, d = len(rows), len(cand), got["desc"][l]
        o = dict(perm=perm[base:base + C] - base, stats=stats[l].tolist())
        if n <= MAX_ROWS():
            o.update(cnt=_at(got["scratch"], d["cnt"], n, np.int32), off=_at(got["scratch"], d["off"], n + 1, np.int64),
                     ex=_at(got["scratch"], d["cnt"] + 4 * n, C, np.int32))
        out.append(o)
        base += C
    return out


def MAX_ROWS():
    return _native.host().fa_dl_regroup_const(0)


def _lds(levels):
    return [int(_native.hip().fa_hip_dl_regroup_lds(len(r), len(c), r.shape[1])) for r, _, c in levels]


def check(S, levels, lds_cap=None):
    """Device equals model on every field of every level, twice."""
    L = len(levels)
    keep = _lay_out(S, levels)
    regrouped, want = host.dl_regroup([(r, c, cand[:, -1]) for r, c, cand in levels])
    assert regrouped
    runs = []
    for _ in range(2):
        got = prim.dl_regroup(S, L, DEV, lds_cap=lds_cap)
        assert got is not None
        runs.append(_fields(got, levels))
        for l, ((rows, cnt, cand), o, g) in enumerate(zip(levels, want, runs[-1])):
            d, d0 = got["desc"][l], S.desc[l]
            assert all(d[f] == d0[f] for f in ("P", "rows", "m", "n", "C", "base")), l
            assert g["stats"] == [o["pieces_prefix"], o["pieces_rule"], o["rounds"], o["kept_prefix"]], l
            assert np.array_equal(g["perm"], o["perm"]), l
            if len(rows) > MAX_ROWS():
                # the generator's own table, the identity at the level's base
                assert d["cnt"] == d0["cnt"] and d["off"] == d0["off"] and o["kept_prefix"] and o["rounds"] == 0
                assert np.array_equal(g["perm"], np.arange(len(cand)))
                continue
            assert np.array_equal(g["cnt"], o["cnt"]), l
            assert np.array_equal(g["off"], o["off"]), l
            assert np.array_equal(g["ex"], o["ex"]), l
    for a, b in zip(*runs):
        assert a.keys() == b.keys() and all(np.array_equal(a[k], b[k]) for k in a)
    del keep
    return want


@pytest.mark.parametrize("case", [c for c in CASES if c != "m12_m13"])
def test_lists_in_global_memory(dl_state, case):
    """Every case of the rule's suite with no LDS for the lists: every level takes the fallback."""
    levels = edge_case(case)
    assert all(x > 0 for x in _lds(levels))
    check(dl_state, levels, lds_cap=0)


def test_not_eligible_whatever_the_cap(dl_state):
    levels = edge_case("m12_m13")
    keep = _lay_out(dl_state, levels)
    assert prim.dl_regroup(dl_state, len(levels), DEV, lds_cap=0) is None
    del keep


@pytest.mark.parametrize("case", ["two_levels", "m11_m12"])
def test_one_level_fits_the_other_does_not(dl_state, case):
    levels = edge_case(case)
    a, b = _lds(levels)
    assert a != b and min(a, b) > 0
    check(dl_state, levels, lds_cap=min(a, b))       # the smaller level's lists in LDS, the other's not
    check(dl_state, levels)


@pytest.mark.parametrize("case", ["star256", "star300", "fan300"])
@pytest.mark.parametrize("cap", [None, 0], ids=["lds", "global"])
def test_counters_past_a_byte(dl_state, case, cap):
    """More than 255 children of one parent (a packed 16-bit counter past a byte): of the prefix
    itself (star: the level keeps the prefix plan) and of the last parent row, at an even index,
    which takes them from 300 prefixes of one child each (fan).  300 candidates are neither whole
    waves nor a whole workgroup."""
    levels = edge_case(case)
    rows, cnt, cand = levels[0]
    E, p = len(cand), 0 if case[:4] == "star" else 600
    assert E > 255 and rows.shape == (2 * E + 1, 2) and (E == 256 or (E > 256 and E % 64 and E % 1024))
    o = check(dl_state, levels, lds_cap=cap)[0]
    assert o["cnt"][p] == E == o["cnt"].sum() and o["pieces_rule"] == (E + 7) // 8
    assert o["kept_prefix"] == (case != "fan300") and o["pieces_prefix"] == ((E + 7) // 8 if p == 0 else E)
    if case == "fan300":
        assert np.array_equal(o["ex"], np.arange(300)) and np.array_equal(o["perm"], np.arange(300))


@pytest.mark.parametrize("case", ["k6_triples", "k7_triples"])
@pytest.mark.parametrize("cap", [None, 0], ids=["lds", "global"])
def test_adjacent_counters_in_one_round(dl_state, case, cap):
    """An even parent row and the odd one after it -- the two halves of one counter word -- both
    receive votes in the same round."""
    levels = edge_case(case)
    rows, cnt, cand = levels[0]
    o = check(dl_state, levels, lds_cap=cap)[0]
    tr, children = _trace(rows, cand)
    assert len(tr) == o["rounds"]
    if not o["kept_prefix"]:
        assert np.array_equal(children, o["cnt"])
    assert any(p % 2 == 0 and p + 1 in votes for _, votes, _ in tr for p in votes)


@pytest.mark.parametrize("cap", [None, 0], ids=["lds", "global"])
def test_tiny_levels(dl_state, cap):
    """C = 1 with n = 1; C = 1 with n = 3; a level of fewer candidates than a wave."""
    for case in ("n1_c1", "one_candidate", "k5_triples"):
        levels = edge_case(case)
        assert len(levels) == 1 and len(levels[0][2]) < 64
        o = check(dl_state, levels, lds_cap=cap)[0]
        if case == "n1_c1":
            assert o["kept_prefix"] and o["cnt"].tolist() == [1] and o["ex"].tolist() == [9]


def test_ten_levels_ending_in_one_candidate(dl_state):
    levels = edge_case("clique12")
    assert len(levels) == 10 and len(levels[-1][2]) == 1 and levels[-1][0].shape[1] == 11
    want = check(dl_state, levels)
    assert not all(o["kept_prefix"] for o in want)
    sizes = sorted(set(_lds(levels)))
    check(dl_state, levels, lds_cap=sizes[len(sizes) // 2])      # half the levels' lists in LDS


@pytest.mark.parametrize("cap", [None, 0], ids=["lds", "global"])
def test_list_survives_rounds_that_assign_nothing(dl_state, cap):
    """Triangles apart: nothing is assigned at the thresholds 8 to 2, everything at 1."""
    levels = edge_case("disjoint")
    rows, cnt, cand = levels[0]
    o = check(dl_state, levels, lds_cap=cap)[0]
    tr, _ = _trace(rows, cand)
    assert len(tr) == o["rounds"] == 7
    assert [(thr, bool(took)) for thr, _, took in tr] == [(t, False) for t in THR[:-1]] + [(1, True), (1, False)]
    assert len(tr[5][2]) == len(cand) == 20


@pytest.mark.parametrize("case", ["rows12300_k5", "k5_rows12300_two"])
@pytest.mark.parametrize("cap", [None, 0], ids=["lds", "global"])
def test_skipped_level_beside_regrouped_ones(dl_state, case, cap):
    """A level past the rows a level regroups with keeps its table and the identity at its base,
    whatever stands before and after it in the bundle."""
    levels = edge_case(case)
    assert any(len(r) > MAX_ROWS() for r, _, _ in levels) and any(len(r) <= MAX_ROWS() for r, _, _ in levels)
    want = check(dl_state, levels, lds_cap=cap)
    assert any(not o["kept_prefix"] for o in want)
