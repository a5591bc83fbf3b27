"""The slab rows' layout with a pad shift and the tail rule built on it (csrc/host/fa_slab.h:
slab_row_off / slab_row_col / slab_rows_bytes, slab_pack_width, slab_tail_cut), through the
fa_slab_* exports.  Row u of sw words starts at u * sw * 8 + (u >> s) * 16: one 16-B pad
slot per 2^s rows; s = 0 is the layout the kernels always had, (sw + 2) * 8 bytes per row.
The kernels under each layout are in tests/test_gpu_slab_pack.py."""
import itertools

import numpy as np
import pytest

LDS = 163328          # TUNING.slab_lds_bytes' default


def _map_lds(F1):
    return ((F1 * 2 + 15) & ~15) if F1 <= 8192 else 0


def _rule(n_used, C, lds, accb):
    """(SW, capacity) of the unpacked rule, restated (tests/test_slab_acc8_rule.py)."""
    for sw in (16, 32, 8, 4):
        cap = int((lds - n_used * (sw + 2) * 8) // accb)
        if cap >= min(C, 8192) or (sw == 4 and cap >= 1024):
            return sw, cap
    return 0, 0


def _rows_bytes(sw, s, n):
    return n * sw * 8 + -(-n // (1 << s)) * 16


@pytest.mark.parametrize("s", [0, 1, 2, 3])
@pytest.mark.parametrize("sw", [4, 8, 16, 32])
def test_row_layout(native, sw, s):
    from fastapriori_amd.ops import primitives as Pm
    off = [Pm.slab_row_off(sw, s, u) for u in range(200)]
    assert off[0] == 0
    assert all(o % 16 == 0 for o in off)
    gaps = np.diff(off)
    assert gaps.min() >= sw * 8                       # rows do not overlap: a row is sw * 8 bytes
    assert set(gaps.tolist()) <= {sw * 8, sw * 8 + 16}
    # one pad slot per 2^s rows, after rows 2^s - 1, 2 * 2^s - 1, ...
    assert [int(g > sw * 8) for g in gaps] == [int((u + 1) % (1 << s) == 0) for u in range(199)]
    if s == 0:
        assert off == [(sw + 2) * 8 * u for u in range(200)]
    for u in range(200):
        assert Pm.slab_row_col(sw, s, u) == (off[u] // 16) % 16
    for n in (0, 1, 2, 3, 4, 5, 7, 8, 9, 63, 64, 65, 974):
        fp = Pm.slab_rows_bytes(sw, s, n)
        assert fp == _rows_bytes(sw, s, n), (n,)
        # the footprint ends behind the last row (its data, and its pad where it has one)
        if n:
            assert fp >= Pm.slab_row_off(sw, s, n - 1) + sw * 8
            assert fp <= Pm.slab_row_off(sw, s, n - 1) + sw * 8 + 16
    assert Pm.slab_layout(sw, s) == sw | (s << 8)
    assert Pm.slab_layout_split(Pm.slab_layout(sw, s)) == (sw, s)


def test_width_16_rows_reach_every_column(native):
    from fastapriori_amd.ops import primitives as Pm
    for s in range(4):
        assert {Pm.slab_row_col(16, s, u) for u in range(16 << s)} == set(range(16))


def test_headline_arithmetic(native):
    # T10I4D100M's levels 3-12: 974 used items, 30,122 candidates, 163,328 - 1,952 B of LDS
    from fastapriori_amd.ops import primitives as Pm
    lds = LDS - _map_lds(974)
    assert lds == 161376
    assert Pm.slab_pack_width(974, 30122, lds, 1) == (16, 32800, 2)
    assert Pm.slab_rows_bytes(16, 2, 974) == 974 * 128 + 244 * 16 == 128576
    assert lds - Pm.slab_rows_bytes(16, 1, 974) == 28912 < 30122        # s = 1 does not fit
    assert lds - Pm.slab_rows_bytes(16, 0, 974) == 21120
    # the unpacked rule splits the bundle: u32 at width 8, bytes at width 16, neither holds it
    assert Pm.slab_width(974, 30122, lds, 4)[1] < 30122 and Pm.slab_width(974, 30122, lds, 1)[1] < 30122


def test_pack_rule_edges(native):
    from fastapriori_amd.ops import primitives as Pm
    lds = LDS - _map_lds(974)
    # C at the capacity, and one more (s = 2 -> s = 3)
    assert Pm.slab_pack_width(974, 32800, lds, 1) == (16, 32800, 2)
    assert Pm.slab_pack_width(974, 32801, lds, 1) == (16, lds - _rows_bytes(16, 3, 974), 3)
    cap3 = lds - _rows_bytes(16, 3, 974)
    assert Pm.slab_pack_width(974, cap3, lds, 1) == (16, cap3, 3)
    # one more than the widest capacity: nothing fits, the unpacked rule's own answer
    assert Pm.slab_pack_width(974, cap3 + 1, lds, 1) == (*Pm.slab_width(974, cap3 + 1, lds, 1), 0)
    # what already fits with every row padded keeps s = 0 and the unpacked rule's capacity
    assert Pm.slab_pack_width(974, 21120, lds, 1) == (16, 21120, 0) == (*Pm.slab_width(974, 21120, lds, 1), 0)
    # an n_used where s = 1 suffices, one where s = 3 is needed
    assert Pm.slab_pack_width(950, 30122, lds, 1)[2] == 1
    assert lds - _rows_bytes(16, 0, 950) < 30122 <= lds - _rows_bytes(16, 1, 950)
    assert Pm.slab_pack_width(1000, 30122, lds, 1)[2] == 3
    assert lds - _rows_bytes(16, 2, 1000) < 30122 <= lds - _rows_bytes(16, 3, 1000)
    # wider accumulators divide the capacity
    assert Pm.slab_pack_width(974, 8200, lds, 4) == (16, 32800 // 4, 2)


def test_pack_rule_over_a_grid(native):
    from fastapriori_amd.ops import primitives as Pm
    n_used = (0, 1, 50, 300, 900, 974, 1000, 1020, 1080, 1250, 1300, 2000, 5000)
    cands = (1, 1000, 8192, 8193, 17695, 21120, 21121, 30122, 32800, 32801, 40000, 1 << 20)
    seen = set()
    for n, C, lds, accb in itertools.product(n_used, cands, (48 << 10, LDS, LDS - _map_lds(974)), (1, 2, 4)):
        sw, cap, s = Pm.slab_pack_width(n, C, lds, accb)
        fits = [q for q in range(4) if (lds - _rows_bytes(16, q, n)) // accb >= C and lds >= _rows_bytes(16, q, n)]
        if fits:
            assert (sw, cap, s) == (16, int((lds - _rows_bytes(16, fits[0], n)) // accb), fits[0]), (n, C, lds, accb)
            assert cap >= C
        else:
            # where nothing fits the answer is bit-equal to the unpacked rule's
            assert (sw, cap, s) == (*Pm.slab_width(n, C, lds, accb), 0) == (*_rule(n, C, lds, accb), 0)
        seen.add((sw, s))
    assert {(16, 0), (16, 1), (16, 2), (16, 3), (8, 0), (4, 0), (0, 0)} <= seen


def test_tail_cut_is_a_replay_of_the_unpacked_rule(native):
    from fastapriori_amd.ops import primitives as Pm
    rng = np.random.default_rng(5)
    cuts = set()
    for _ in range(400):
        L = int(rng.integers(1, 12))
        n_used = int(rng.choice([50, 300, 900, 974, 1000, 1100, 2000]))
        lds = int(rng.choice([48 << 10, LDS - _map_lds(974)]))
        accb = int(rng.choice([1, 2, 4]))
        Cs = [int(c) for c in rng.integers(1, int(rng.choice([40, 4000, 20000])), size=L)]
        total, want = Cs[0], 1                        # level 0 stands, level l joins while the total fits
        for c in Cs[1:]:
            if total + c > _rule(n_used, total + c, lds, accb)[1]:
                break
            total += c
            want += 1
        assert Pm.slab_tail_cut(Cs, n_used, lds, accb) == want, (Cs, n_used, lds, accb)
        cuts.add(want == L)
    assert cuts == {True, False}
    assert Pm.slab_tail_cut([], 974, LDS, 4) == 0
    # the headline's chain: levels 3-4 stand (17,695), level 5 does not join at u32
    assert Pm.slab_tail_cut([9000, 8695, 6000, 3000], 974, LDS - _map_lds(974), 4) == 2


def test_host_mirror_of_the_tail_rule(native):
    from fastapriori_amd.ops import primitives as Pm
    lds = LDS - _map_lds(974)
    Cs = [9000, 8695, 6000, 3000, 2000, 1000, 427]          # 30,122 in all
    assert sum(Cs) == 30122
    # the bundle ends the run: one packed pass of all levels
    assert Pm.dl_tail_plan(Cs, 974, lds, 4, 1, ends=True) == (7, 16, 2, 32800)
    # it does not: exactly the unpacked rule's levels, layout and (upgraded) width
    assert Pm.dl_tail_plan(Cs, 974, lds, 4, 1, ends=False) == (2, 16, 0, 21120)
    assert Pm.dl_tail_plan(Cs, 974, lds, 4, 4, ends=False) == (2, 8, 0, 20864)
    # it ends the run but does not fit even at s = 3: cut as without the rule
    big = [9000, 8695, 9000, 9000]
    assert Pm.dl_tail_plan(big, 974, lds, 4, 1, ends=True) == (2, 16, 0, 21120)
    # nothing to remove: the unpacked rule takes every level
    assert Pm.dl_tail_plan([9000, 8695], 974, lds, 4, 1, ends=True) == (2, 16, 0, 21120)


def test_old_exports_are_unchanged(native, tune):
    from fastapriori_amd.ops import primitives as Pm
    n_used = (0, 1, 50, 300, 900, 960, 974, 976, 977, 1000, 1080, 2000, 3000, 5000, 20000)
    cands = (1, 1000, 1023, 1024, 8191, 8192, 8193, 17695, 21120, 21121, 40000, 1 << 20)
    for n, C, lds, accb in itertools.product(n_used, cands, (24 << 10, 48 << 10, LDS, LDS - _map_lds(974)),
                                             (1, 2, 4)):
        assert Pm.slab_width(n, C, lds, accb) == _rule(n, C, lds, accb), (n, C, lds, accb)
    for n, lds, accb in itertools.product(n_used, (48 << 10, LDS), (1, 4)):
        t = Pm.slab_total_limit(n, lds, accb)
        assert t <= _rule(n, t, lds, accb)[1] and t + 1 > _rule(n, t + 1, lds, accb)[1]
    for F1 in (0, 1, 7, 8, 974, 8192, 8193):
        assert Pm.slab_map_lds(F1) == _map_lds(F1)
    # workgroups: a bare width means every row padded, as before the pad shift existed
    tune(slab_lds_bytes=LDS)
    for n, sw, nacc in itertools.product((1, 100, 974, 2000), (4, 8, 16, 32), (1, 1000, 7531, 20000)):
        lds = n * (sw + 2) * 8 + ((nacc + 3) & ~3) * 4 + _map_lds(974)
        per_cu = min(2, max(1, LDS // max(lds, 1)))
        for nslabs in (1, 255, 256, 300, 513, 100000):
            assert Pm._slab_workgroups(nslabs, n, sw, nacc, True, _map_lds(974)) == max(1, min(nslabs, 256 * per_cu))
            assert Pm._slab_workgroups(nslabs, n, Pm.slab_layout(sw, 0), nacc, True, _map_lds(974)) == \
                max(1, min(nslabs, 256 * per_cu))
