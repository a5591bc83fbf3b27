"""Leave-one-out ranks on the device: k_holdout_rank and k_holdout_rank_indexed against
fa_holdout_rank_cpu, exact equality everywhere -- the hand-built table and the mined case of
test_holdout_eval.py, edge shapes (idle waves, step boundaries, bitset widths, a basket wider
than a wave, planted steps and lists), the LDS fallback and the model on the device."""
import functools

import numpy as np
import pytest
import torch

from fastapriori_amd.models.rules import AssociationRules
from fastapriori_amd.ops import primitives as prim
from fastapriori_amd.utils.metrics import Logger
from test_holdout_eval import (HAND_F1, brute_ranks, composed, csr_tensors, hand_table, hand_want, mined_case,
                               rules_tensors)

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
KERNELS = pytest.mark.parametrize("indexed", [False, True], ids=["scan", "indexed"])
LAUNCHERS = ("fa_hip_holdout_rank", "fa_hip_holdout_rank_indexed")


def _spy(monkeypatch):
    """Record which launcher runs."""
    calls = []
    for name in LAUNCHERS:
        fn = getattr(prim._native.hip(), name)
        monkeypatch.setattr(prim._native.hip(), name, lambda *a, _fn=fn, _name=name: calls.append(_name) or _fn(*a))
    return calls


def _both(rules, baskets, F1, n, indexed):
    """(device result of the asked kernel, run twice and equal; fa_holdout_rank_cpu's), as lists."""
    cpu = prim.holdout_rank(*rules_tensors(rules), F1, *csr_tensors(baskets), n)
    a_off, ante, cons = rules_tensors(rules, DEV)
    boff, bask = csr_tensors(baskets, DEV)
    index = prim.recommend_index(a_off, ante, F1) if indexed else None
    prim.reset_fallbacks()
    got = prim.holdout_rank(a_off, ante, cons, F1, boff, bask, n, index=index)
    again = prim.holdout_rank(a_off, ante, cons, F1, boff, bask, n, index=index)
    assert not prim.FALLBACKS
    assert got.device.type == "cuda" and got.dtype == torch.int32 and tuple(got.shape) == (bask.numel(),)
    assert torch.equal(got, again)
    return got.cpu().tolist(), cpu.tolist()


@KERNELS
@pytest.mark.parametrize("n", [1, 2, 64])
def test_hand_table_on_device(monkeypatch, n, indexed):
    rules, baskets, _ = hand_table()
    calls = _spy(monkeypatch)
    got, cpu = _both(rules, baskets, HAND_F1, n, indexed)
    assert got == hand_want(n) == cpu
    assert calls == [LAUNCHERS[indexed]] * 2


@KERNELS
@pytest.mark.parametrize("n", [1, 3, 10])
def test_mined_case_on_device(monkeypatch, n, indexed):
    _, _, _, (rules, F1, boff, bask) = mined_case()
    ref = prim.holdout_rank(*rules, F1, boff, bask, n)                 # fa_holdout_rank_cpu
    assert torch.equal(ref, composed(n)[0]) and len(set(ref.tolist())) == n + 1
    a_off, ante, cons = (x.to(DEV) for x in rules)
    index = prim.recommend_index(a_off, ante, F1) if indexed else None
    calls = _spy(monkeypatch)
    prim.reset_fallbacks()
    got = prim.holdout_rank(a_off, ante, cons, F1, boff.to(DEV), bask.to(DEV), n, index=index)
    assert torch.equal(got, prim.holdout_rank(a_off, ante, cons, F1, boff.to(DEV), bask.to(DEV), n, index=index))
    assert got.device.type == "cuda" and torch.equal(got.cpu(), ref)
    assert not prim.FALLBACKS and calls == [LAUNCHERS[indexed]] * 2


# ---------------------------------------------------------------------------
# edge shapes: random tables from a fixed seed
# ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _random_table(R, F1, sizes, seed=0):
    """(rules, baskets): every antecedent a random subset of 1..3 items; a basket of size s is
    filled with whole rules (antecedent + consequent) that still fit, so that rules fire and
    hidden items are consequents, and with single random items."""
    rng = np.random.default_rng(7000 + 131 * R + F1 + 17 * sum(sizes) + seed)
    if F1 == 1:
        rules = [((0,), 0)] * R                # the only table over one item: nothing can fire
    else:
        rules = []
        for _ in range(R):
            it = rng.choice(F1, 1 + min(F1 - 1, int(rng.integers(1, 4))), replace=False)
            rules.append((tuple(sorted(it[1:].tolist())), int(it[0])))
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
    return rules, baskets


def _check(rules, baskets, F1, n, indexed, need_hit=True):
    got, cpu = _both(rules, baskets, F1, n, indexed)
    assert cpu == brute_ranks(rules, baskets, n)
    assert got == cpu
    if need_hit:
        assert any(cpu), "no trial finds its hidden item: the case checks nothing"
    return cpu


@KERNELS
@pytest.mark.parametrize("sizes", [(1,), (3,), (2, 2), (2, 3)], ids=["T1", "T3", "T4", "T5"])
def test_trial_counts_leave_idle_waves(sizes, indexed):
    rules, baskets = _random_table(64, 33, sizes)
    _check(rules, baskets, 33, 3, indexed, need_hit=sum(sizes) > 1)


@KERNELS
@pytest.mark.parametrize("R", [1, 63, 64, 65, 129])
def test_rule_counts_at_step_boundaries(R, indexed):
    if R == 1:
        rules, baskets = [((0,), 1)], [[0, 1], [1], [0, 1, 2]]
    else:
        rules, baskets = _random_table(R, 12, (2, 3, 4, 5, 6, 3, 2))
        # the last rule decides a trial: its basket meets no rule before it
        rules = [((a if 11 not in a else (10,)), (c if c != 11 else 9)) for a, c in rules[:-1]] + [((11,), 10)]
        baskets = baskets + [[10, 11]]
        assert brute_ranks(rules, baskets, 64)[-2:] == [1, 0]
    for n in (1, 4, 64):
        _check(rules, baskets, 12 if R > 1 else 3, n, indexed)


@KERNELS
@pytest.mark.parametrize("F1", [1, 31, 32, 33, 2049])
def test_bitset_widths(F1, indexed):
    rules, baskets = _random_table(65, F1, (1,) if F1 == 1 else (2, 3, 4, 5, 2))
    if F1 > 1:
        # the highest item as consequent and as hidden item: the last bit of the last word
        rules = rules + [((0,), F1 - 1)]
        baskets = baskets + [[0, F1 - 1]]
    for n in (2, 64):
        want = _check(rules, baskets, F1, n, indexed, need_hit=F1 > 1)
        if F1 > 1 and n == 64:
            assert want[-1] > 0


@KERNELS
def test_basket_of_70_items(indexed):
    rules, baskets = _random_table(129, 200, (70, 2, 70))
    assert len(baskets[0]) == 70
    for n in (1, 5, 64):
        _check(rules, baskets, 200, n, indexed)


def _planted_step():
    """Step 0 (rules 0..63) takes consequents 1 and 2; in step 1 the hidden item's rule 70 shares
    the step with a taken consequent (64), two rules of one new consequent (65, 66) and a second
    rule of its own consequent (71)."""
    rules = [((0,), 1), ((0,), 2)] + [((39,), 3)] * 62
    rules += [((0,), 1), ((0,), 3), ((0,), 3), ((39,), 4), ((39,), 4), ((39,), 4), ((0,), 5), ((0,), 5), ((0,), 6)]
    return rules, [[0, 5], [0, 6], [0, 7]], 40


@KERNELS
def test_planted_step_and_short_lists(indexed):
    rules, baskets, F1 = _planted_step()
    # places: 5 behind 1, 2, 3; 6 behind 1, 2, 3, 5; 7 is nobody's consequent
    for n, want in ((3, [0, 0, 0, 0, 0, 0]), (4, [0, 4, 0, 0, 0, 0]), (5, [0, 4, 0, 5, 0, 0]),
                    (64, [0, 4, 0, 5, 0, 0])):       # n = 64: more slots than distinct firing consequents
        assert _check(rules, baskets, F1, n, indexed, need_hit=n > 3) == want


@KERNELS
def test_rules_listed_under_the_hidden_item(indexed):
    # every rule that fires on {2, 9} ends in 9: with 9 hidden nothing fires (and 2 is no consequent)
    rules = [((9,), 5), ((2, 9), 6)]
    assert _check(rules, [[2, 9]], 12, 3, indexed, need_hit=False) == [0, 0]
    # rule 0 is in the hidden item's list and must not take the place before rule 1's consequent
    rules = [((9,), 5), ((2,), 9), ((2, 9), 6)]
    assert _check(rules, [[2, 9]], 12, 3, indexed) == [0, 1]


@KERNELS
def test_early_hit_bounds_the_later_lists(indexed):
    # basket {3, 4, 8} hiding 8: item 3's list is visited first and holds the hidden item's rule 5;
    # of item 4's list only rule 2 (before it) still counts, rules 10.. are past the bound
    rules = [((7,), 1)] * 12
    rules[5] = ((3,), 8)
    rules[2] = ((4,), 7)
    rules[10], rules[11] = ((4,), 6), ((4,), 5)
    rules += [((4,), 9 + k % 3) for k in range(70)]           # a list longer than one step
    for n, want in ((1, 0), (2, 2), (64, 2)):
        got = _check(rules, [[3, 4, 8]], 16, n, indexed, need_hit=n > 1)
        assert got[2] == want


def test_wide_vocabulary_falls_back_once():
    F1 = 131073                                               # a bitset past 64 KiB
    rules, baskets = [((0,), F1 - 1), ((F1 - 1,), 0)], [[0, F1 - 1]]
    cpu = prim.holdout_rank(*rules_tensors(rules), F1, *csr_tensors(baskets), 2)
    assert cpu.tolist() == [1, 1]
    a_off, ante, cons = rules_tensors(rules, DEV)
    for index in (None, prim.recommend_index(a_off, ante, F1)):
        prim.reset_fallbacks()
        got = prim.holdout_rank(a_off, ante, cons, F1, *csr_tensors(baskets, DEV), 2, index=index)
        assert got.device.type == "cuda" and got.cpu().tolist() == cpu.tolist()
        assert len(prim.FALLBACKS) == 1 and "leave-one-out" in prim.FALLBACKS[0]
    prim.reset_fallbacks()


@pytest.mark.parametrize("n", [0, 65])
def test_launchers_refuse_n_out_of_range(n):
    # the launchers return before they look at a pointer
    lib = prim._native.hip()
    assert lib.fa_hip_holdout_rank(None, None, None, 1, 33, None, None, None, 1, n, None, None) != 0
    assert lib.fa_hip_holdout_rank_indexed(None, None, None, None, None, 1, 33, None, None, None, 1, n, None,
                                           None) != 0


# ---------------------------------------------------------------------------
# the model on the device
# ---------------------------------------------------------------------------
@KERNELS
def test_shard_picks_the_kernel(monkeypatch, indexed):
    res, users, ar, _ = mined_case()
    on = AssociationRules(res, logger=Logger(enabled=False))          # CPU, baskets de-duplicated
    boff_ref, ranks_ref = on.holdout_ranks_shard(users, 10)
    assert on.stats["distinct_baskets"] < users.n_lines
    assert torch.equal(ranks_ref, ar.holdout_ranks_shard(users, 10)[1])          # ar: without dedup
    monkeypatch.setattr(prim, "RECOMMEND_INDEX_MIN_RULES", 1 if indexed else 1 << 30)
    calls = _spy(monkeypatch)
    dev = AssociationRules(res, device="cpu", logger=Logger(enabled=False))      # the same (host-built) rule table
    prim.reset_fallbacks()
    boff, ranks = dev.holdout_ranks_shard(users.to(DEV), 10)
    assert ranks.device.type == "cuda" and ranks.dtype == torch.int32 and boff.dtype == torch.int64
    assert torch.equal(boff.cpu(), boff_ref) and torch.equal(ranks.cpu(), ranks_ref)
    assert not prim.FALLBACKS and calls == [LAUNCHERS[indexed]]


def test_evaluate_on_device_equals_cpu_json():
    res, users, _, _ = mined_case()
    want = AssociationRules(res, logger=Logger(enabled=False)).evaluate(users, 10).as_json()
    dev = AssociationRules(res, device=DEV, logger=Logger(enabled=False))        # rules built by the device, too
    assert dev.evaluate(users.to(DEV), 10).as_json() == want
    assert "fallbacks" not in dev.stats
    ev, lines = dev.run_evaluate(users.to(DEV), 10, rank_lines=True)
    assert ev.as_json() == want
    assert lines == AssociationRules(res, logger=Logger(enabled=False)).run_evaluate(users, 10, rank_lines=True)[1]
