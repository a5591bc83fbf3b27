"""Combined scoring on the device: k_recommend_combined and k_holdout_rank_combined against
fa_recommend_combined_cpu / fa_holdout_rank_combined_cpu and against brute force, exact equality
everywhere and twice -- idle waves, list lengths at the 64-rule step, more consequents than
slots, ties, sums across the dword boundary, bitset widths, the LDS rule's boundaries read from
libfa_host.so, the host fallback, the holdout's own cases and the model on the device."""
import functools

import pytest
import torch

from fastapriori_amd.models.rules import AssociationRules
from fastapriori_amd.ops import primitives as prim
from fastapriori_amd.utils.metrics import Logger
from test_holdout_eval import csr_tensors, mined_case, rules_tensors
from test_recommend_combined import brute_combined, brute_list, brute_places, random_table, weight_tensor

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
LAUNCHERS = ("fa_hip_recommend_combined", "fa_hip_holdout_rank_combined")


def _spy(monkeypatch):
    """Record which launcher runs."""
    calls = []
    for name in LAUNCHERS:
        fn = getattr(prim._native.hip(), name)
        monkeypatch.setattr(prim._native.hip(), name, lambda *a, _fn=fn, _name=name: calls.append(_name) or _fn(*a))
    return calls


def _check(rules, weights, baskets, F1, n, fallbacks=0):
    """Both kernels against the C++ path and brute force; every device result is computed twice
    (once with the index built inside the op, once with a given one) and must repeat itself.
    -> (rule rows, score rows, places) as lists."""
    r_cpu, w_cpu, (boff, bask) = rules_tensors(rules), weight_tensor(weights), csr_tensors(baskets)
    rule, score = prim.recommend_combined(*r_cpu, w_cpu, F1, boff, bask, n)
    place = prim.holdout_rank_combined(*r_cpu, w_cpu, F1, boff, bask, n)
    assert (rule.tolist(), score.tolist()) == brute_combined(rules, weights, baskets, n)
    assert place.tolist() == brute_places(rules, weights, baskets, n)
    a_off, ante, cons = rules_tensors(rules, DEV)
    w_dev, (boff_d, bask_d) = weight_tensor(weights, DEV), csr_tensors(baskets, DEV)
    index = prim.recommend_index(a_off, ante, F1)
    for op, want in ((prim.recommend_combined, (rule, score)), (prim.holdout_rank_combined, (place,))):
        outs = []
        for ix in (None, index):
            prim.reset_fallbacks()
            got = op(a_off, ante, cons, w_dev, F1, boff_d, bask_d, n, index=ix)
            assert len(prim.FALLBACKS) == fallbacks, prim.FALLBACKS
            got = got if isinstance(got, tuple) else (got,)
            assert all(g.device.type == "cuda" and g.dtype == w.dtype and g.shape == w.shape for g, w in zip(got, want))
            outs.append(got)
        for g0, g1, w in zip(outs[0], outs[1], want):
            assert torch.equal(g0, g1)
            assert torch.equal(g0.cpu(), w)
    prim.reset_fallbacks()
    return rule.tolist(), score.tolist(), place.tolist()


# ---------------------------------------------------------------------------
# shapes
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 3, 4, 5])
def test_counts_leave_idle_waves(k):
    # k baskets for the list kernel
    rules, weights, baskets = random_table(64, 33, (3, 2, 4, 3, 2)[:k], seed=k)
    baskets = [sorted(rules[0][0])] + baskets[1:]            # rule 0's antecedent alone: it fires
    rule, _, _ = _check(rules, weights, baskets, 33, 3)
    assert any(r[0] >= 0 for r in rule)
    # k trials for the holdout kernel
    rules, weights, baskets = random_table(64, 33, {1: (1,), 3: (3,), 4: (2, 2), 5: (2, 3)}[k], seed=10 + k)
    _, _, place = _check(rules, weights, baskets, 33, 3)
    assert len(place) == k and (k == 1 or any(place))


@pytest.mark.parametrize("L", [1, 63, 64, 65, 129])
def test_one_list_voting_for_one_consequent(L):
    # all L rules of item 0's list add to item 1: up to 64 lanes, one address
    rules = [((0,), 1)] * L
    weights = [1 + (7 * i) % 5 for i in range(L)]
    rule, score, place = _check(rules, weights, [[0], [0, 1]], 2, 2)
    assert rule == [[0, -1], [-1, -1]] and score == [[sum(weights), 0], [0, 0]] and place == [0, 0, 1]


@pytest.mark.parametrize("L", [1, 63, 64, 65, 129])
def test_one_list_of_distinct_consequents(L):
    # L consequents from one list; three weights, so the order is mostly decided by f
    rules = [((0,), 1 + i) for i in range(L)]
    weights = [1 + (i * 5) % 3 for i in range(L)]
    baskets = [[0], [0, 1], [0, L], [0, (L + 1) // 2]]
    for n in (1, 3, 64):
        rule, score, place = _check(rules, weights, baskets, L + 1, n)
        assert len([r for r in rule[0] if r >= 0]) == min(n, L)
        if n == 64:
            # L > 64: the list is cut at the 64th place; L < 64: it is padded
            assert (-1 in rule[0]) == (L < 64) and (0 in score[0]) == (L < 64)


def test_more_firing_consequents_than_slots():
    # items 0..3 each name every item of 4..89, two pairs add to some: 86 consequents, sums that tie
    rules = [((a,), c) for c in range(4, 90) for a in range(4)] + [((0, 1), c) for c in range(4, 90, 3)]
    rules += [((2, 3), c) for c in range(5, 90, 7)]
    weights = [1 + (3 * i) % 4 for i in range(len(rules))]
    baskets = [[0, 1, 2, 3], [0, 2], [1, 3, 50], [0, 1, 2, 3, 88], [2]]
    assert [len(brute_list(rules, weights, b)) for b in baskets] == [86, 86, 85, 85, 86]
    rule, score, place = _check(rules, weights, baskets, 90, 64)
    assert all(-1 not in r and 0 not in s for r, s in zip(rule, score))
    assert any(place) and 0 in place
    _check(rules, weights, baskets, 90, 7)


def test_ties_are_decided_by_the_first_rule():
    # basket {2, 5}: item 2's list (rules 1, 2) is walked before item 5's (rule 0).  Items 7 and 8 tie at 3;
    # item 7's first rule 0 is met after its rule 2, and still puts it in front of item 8 (f = 1)
    rules = [((5,), 7), ((2,), 8), ((2,), 7)]
    rule, score, place = _check(rules, [1, 3, 2], [[2, 5], [2, 5, 7], [2, 5, 8]], 9, 2)
    assert rule[0] == [0, 1] and score[0] == [3, 3]
    assert place == [0, 0, 0, 0, 1, 0, 0, 2]
    # longer ties: 40 consequents of equal score
    rules = [((0,), 1 + i % 40) for i in range(80)]
    rule, score, _ = _check(rules, [1] * 80, [[0]], 41, 64)
    assert rule[0][:40] == list(range(40)) and score[0][:40] == [2] * 40


def test_sums_carry_across_the_dword_boundary():
    rules = [((0,), 1), ((0,), 1), ((0,), 2)]
    _, score, place = _check(rules, [2 ** 32 - 1, 1, 2 ** 32 - 1], [[0], [0, 2]], 3, 2)
    assert score[0] == [2 ** 32, 2 ** 32 - 1] and place == [0, 0, 2]
    rules = [((0,), 1)] * 129 + [((0,), 2)] * 128
    _, score, _ = _check(rules, [2 ** 32] * 257, [[0]], 3, 2)
    assert score[0] == [129 * 2 ** 32, 128 * 2 ** 32]


@pytest.mark.parametrize("F1", [1, 31, 32, 33, 2049])
def test_bitset_widths(F1):
    if F1 == 1:
        rules, weights, baskets = [((0,), 0)] * 3, [1, 2, 3], [[0]]         # the only table over one item
    else:
        rules, weights, baskets = random_table(65, F1, (2, 3, 4, 5, 2), seed=1)
        # the highest item as consequent and as hidden item: the last entry of every row
        rules, weights, baskets = rules + [((0,), F1 - 1)], weights + [2 ** 32], baskets + [[0, F1 - 1]]
    for n in (2, 64):
        _, _, place = _check(rules, weights, baskets, F1, n)
        if F1 > 1 and n == 64:
            assert place[-1] > 0


@functools.lru_cache(maxsize=None)
def _largest_f1(waves):
    """The largest F1 whose rows fit ``waves`` waves per workgroup, by libfa_host.so's rule."""
    lo, hi = 1, 1 << 20
    assert prim.combine_waves(lo) >= waves > prim.combine_waves(hi)
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if prim.combine_waves(mid) >= waves else (lo, mid)
    return lo


def _wide_case(F1):
    """Rules and baskets over the two ends of the rows; 6 baskets, so more than one workgroup at 4 waves."""
    rules = [((0,), F1 - 1), ((F1 - 1,), 0), ((1,), F1 - 2), ((0, 1), F1 - 1), ((F1 - 2,), F1 - 1), ((F1 - 1,), 1)]
    baskets = [[0, F1 - 1], [0, 1], [1, F1 - 2], [F1 - 2, F1 - 1], [0], [0, 1, F1 - 2]]
    return rules, [3, 2, 2 ** 32, 1, 2, 3], baskets


@pytest.mark.parametrize("waves", [4, 2, 1])
def test_lds_rule_boundaries(waves):
    F1 = _largest_f1(waves)
    lds_max = int(prim._native.host().fa_combine_lds_max())
    assert waves * prim.combine_wave_bytes(F1) <= lds_max < waves * prim.combine_wave_bytes(F1 + 1)
    assert prim.combine_waves(F1) == waves and prim.combine_waves(F1 + 1) == waves // 2
    _, _, place = _check(*_wide_case(F1), F1, 3)
    assert any(place)
    if waves > 1:
        _check(*_wide_case(F1 + 1), F1 + 1, 3)


def test_first_f1_that_fits_no_wave_falls_back_once():
    F1 = _largest_f1(1) + 1
    assert prim.combine_waves(F1) == 0
    _, _, place = _check(*_wide_case(F1), F1, 3, fallbacks=1)      # each op notes exactly one fallback
    assert any(place)
    a_off, ante, cons = rules_tensors(_wide_case(F1)[0], DEV)
    prim.reset_fallbacks()
    prim.recommend_combined(a_off, ante, cons, weight_tensor(_wide_case(F1)[1], DEV), F1,
                            *csr_tensors(_wide_case(F1)[2], DEV), 3)
    assert len(prim.FALLBACKS) == 1 and "combined scoring on the host" in prim.FALLBACKS[0]
    prim.reset_fallbacks()


def test_basket_of_70_items():
    rules, weights, baskets = random_table(129, 200, (70, 2, 70), seed=2)
    assert len(baskets[0]) == 70
    for n in (1, 5, 64):
        _, _, place = _check(rules, weights, baskets, 200, n)
        assert any(place)


# ---------------------------------------------------------------------------
# the holdout's own cases
# ---------------------------------------------------------------------------
def test_rules_listed_under_the_hidden_item():
    # every rule that fires on {2, 9} ends in 9: with 9 hidden nothing fires (and 2 is no consequent)
    assert _check([((9,), 5), ((2, 9), 6)], [4, 4], [[2, 9]], 12, 3)[2] == [0, 0]
    # rule 0 is in the hidden item's list: had it voted, item 5 would stand before item 9
    rules = [((9,), 5), ((2,), 9), ((2, 9), 6)]
    assert _check(rules, [2 ** 32, 1, 2 ** 32], [[2, 9]], 12, 1)[2] == [0, 1]


def test_place_n_and_past_n_and_short_baskets():
    rules = [((0,), c) for c in range(1, 6)]
    baskets = [[0, 3], [0], [], [3]]                 # item 3 is third on {0}; one item; empty; one item
    for n, want in ((3, [0, 3, 0, 0]), (2, [0, 0, 0, 0]), (64, [0, 3, 0, 0])):
        assert _check(rules, [5, 4, 3, 2, 1], baskets, 6, n)[2] == want


def test_no_rules_returns_padding_without_a_launch(monkeypatch):
    calls = _spy(monkeypatch)
    none = (torch.zeros(1, dtype=torch.int64, device=DEV), torch.zeros(0, dtype=torch.int32, device=DEV),
            torch.zeros(0, dtype=torch.int32, device=DEV))
    w0 = torch.zeros(0, dtype=torch.int64, device=DEV)
    boff, bask = csr_tensors([[0, 1], [2]], DEV)
    rule, score = prim.recommend_combined(*none, w0, 3, boff, bask, 2)
    assert rule.device.type == "cuda" and rule.tolist() == [[-1, -1]] * 2 and score.tolist() == [[0, 0]] * 2
    assert prim.holdout_rank_combined(*none, w0, 3, boff, bask, 2).tolist() == [0, 0, 0]
    assert calls == []


@pytest.mark.parametrize("n", [0, 65])
def test_launchers_refuse_n_out_of_range(n):
    # the launchers return before they look at a pointer
    lib = prim._native.hip()
    assert lib.fa_hip_recommend_combined(None, None, None, None, None, None, 1, 33, None, None, 1, n, None, None,
                                         None) != 0
    assert lib.fa_hip_holdout_rank_combined(None, None, None, None, None, None, 1, 33, None, None, None, 1, n, None,
                                            None) != 0


# ---------------------------------------------------------------------------
# the model on the device
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["sum", "votes"])
def test_model_on_device_equals_cpu(monkeypatch, mode):
    res, users, _, _ = mined_case()
    cpu = AssociationRules(res, logger=Logger(enabled=False))
    want_rule, want_score = cpu.recommend_combined_shard(users, 10, mode)
    want_lines = cpu.run_topn(users, 10, scores=True, combine=mode)
    want_ev, want_ranks = cpu.run_evaluate(users, 10, rank_lines=True, combine=mode)
    assert int((want_rule >= 0).sum()) > users.n_lines and sum(want_ev.hits) > 0
    calls = _spy(monkeypatch)
    dev = AssociationRules(res, device=DEV, logger=Logger(enabled=False))        # rules built by the device, too
    udev = users.to(DEV)
    rule, score = dev.recommend_combined_shard(udev, 10, mode)
    assert rule.device.type == "cuda" and score.dtype == torch.int64
    assert torch.equal(rule.cpu(), want_rule) and torch.equal(score.cpu(), want_score)
    assert dev.run_topn(udev, 10, scores=True, combine=mode) == want_lines
    ev, ranks = dev.run_evaluate(udev, 10, rank_lines=True, combine=mode)
    assert ev.as_json() == want_ev.as_json() and ranks == want_ranks and f'"combine": "{mode}"' in ev.as_json()
    assert "fallbacks" not in dev.stats
    assert calls == [LAUNCHERS[0], LAUNCHERS[0], LAUNCHERS[1]]
