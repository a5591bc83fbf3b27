"""The slab rule with one LDS byte per accumulator (csrc/host/fa_slab.h, accb = 1: the
single-writer byte counters of k_count_slab_rec), the accb -> kernel mode mapping
(fa_slab_acc_mode) and the invariant the byte counters rest on: in every pass of a plan
the pieces' candidate ranges [a.x, a.x + n_ext) are pairwise disjoint and cover the pass's
candidates, so a thread -- which owns the same pieces on every slab -- is the only writer
of its counters.  Host plans (plan.cpp, through level_plan_host) are checked here; the
device plan (levels.hip k_dl_pieces_emit) in tests/test_gpu_slab_acc8.py."""
import itertools

import numpy as np
import pytest

LDS = 163328          # TUNING.slab_lds_bytes' default


def _map_lds(F1):
    return ((F1 * 2 + 15) & ~15) if F1 <= 8192 else 0


def _rule(n_used, C, lds, accb):
    """(SW, capacity): the rule restated (widths 16, 32, 8, 4 in the measured order)."""
    for sw in (16, 32, 8, 4):
        cap = int((lds - n_used * (sw + 2) * 8) // accb)
        if cap >= min(C, 8192) or (sw == 4 and cap >= 1024):
            return sw, cap
    return 0, 0


N_USED = (0, 1, 50, 300, 900, 960, 974, 976, 977, 1000, 1080, 2000, 3000, 5000, 20000)
CANDS = (1, 1000, 1023, 1024, 8191, 8192, 8193, 17695, 21120, 21121, 40000, 1 << 20)
BUDGETS = (24 << 10, 48 << 10, LDS, LDS - _map_lds(974), LDS - _map_lds(8192))


def test_slab_width_at_one_byte_matches_the_restated_rule(native):
    from fastapriori_amd.ops import primitives as Pm
    seen = set()
    for n, C, lds in itertools.product(N_USED, CANDS, BUDGETS):
        got = Pm.slab_width(n, C, lds, 1)
        assert got == _rule(n, C, lds, 1), (n, C, lds)
        seen.add(got[0])
    assert seen == {16, 8, 4, 0}


def test_slab_total_limit_at_one_byte(native):
    from fastapriori_amd.ops import primitives as Pm
    for n, lds in itertools.product(N_USED, BUDGETS):
        t = Pm.slab_total_limit(n, lds, 1)
        assert 0 <= t <= _rule(n, t, lds, 1)[1], (n, lds, t)
        assert t + 1 > _rule(n, t + 1, lds, 1)[1], (n, lds, t)


def test_headline_bundle_takes_width_16_in_one_pass(native):
    # T10I4D100M's levels 3-4: 974 used items, 17,695 candidates, 163,328 - 1,952 B of LDS
    from fastapriori_amd.ops import primitives as Pm
    lds = LDS - _map_lds(974)
    assert lds == 161376
    assert Pm.slab_width(974, 17695, lds, 1) == (16, 21120)
    assert Pm.slab_width(974, 17695, lds, 4) == (8, 20864)
    assert Pm.slab_width(974, 17695, lds, 2) == (16, 10560)   # width 16, but not one pass
    # once width 16 holds 8,192 bytes the rule stays there: above ~976 items its one-pass
    # capacity is below u32's at width 8 (496 n > 3 lds)
    assert Pm.slab_total_limit(974, lds, 1) == 21120 > Pm.slab_total_limit(974, lds, 4)
    assert Pm.slab_total_limit(1000, lds, 1) == lds - 144000 < Pm.slab_total_limit(1000, lds, 4)


def test_acc_mode_and_accumulator_words(native):
    from fastapriori_amd.ops import primitives as Pm
    K = Pm.dl()
    modes = {accb: Pm._slab_acc_mode(accb, False, 1)[0] for accb in (4, 2, 1)}
    assert modes[4] == 0 and modes[2] == K.kSlabAcc16
    # a bit of its own, beside the exported ones
    assert modes[1] not in (0, K.kSlabCls, K.kSlabDense, K.kSlabAcc16) and modes[1] & (modes[1] - 1) == 0
    assert modes[1] & (K.kSlabCls | K.kSlabDense | K.kSlabAcc16) == 0
    for C in (1, 2, 3, 4, 5, 8, 9, 17695, 21120):
        assert Pm._slab_acc_mode(4, False, C) == (0, C)
        assert Pm._slab_acc_mode(2, False, C) == (K.kSlabAcc16, (C + 1) // 2)
        assert Pm._slab_acc_mode(1, False, C) == (modes[1], (C + 3) // 4)
        # weighted rows count into u32 whatever is asked
        assert all(Pm._slab_acc_mode(accb, True, C) == (0, C) for accb in (4, 2, 1))


def test_launch_footprint_charges_a_byte_per_candidate(native, tune):
    # the launcher's LDS bytes: slab rows + ceil(C / 4) accumulator words (rounded to 16 B)
    # + rank map.  slab_workgroups gives two workgroups per CU exactly when the budget holds
    # twice that footprint, which pins it to the byte.
    from fastapriori_amd.ops import primitives as Pm
    for n, sw, C, mp in itertools.product((1, 300, 974), (4, 8, 16, 32), (1, 5, 4097, 17695, 21120), (0, 1952)):
        _, nacc = Pm._slab_acc_mode(1, False, C)
        assert nacc == -(-C // 4)
        want = n * (sw + 2) * 8 + ((nacc + 3) & ~3) * 4 + mp
        tune(slab_lds_bytes=2 * want)
        assert Pm._slab_workgroups(5000, n, sw, nacc, True, mp) == 512
        tune(slab_lds_bytes=2 * want - 1)
        assert Pm._slab_workgroups(5000, n, sw, nacc, True, mp) == 256
    # the headline bundle fits the kernel's limit (160 KiB - 256 B) with its map
    _, nacc = Pm._slab_acc_mode(1, False, 17695)
    assert 974 * 144 + ((nacc + 3) & ~3) * 4 + _map_lds(974) <= 160 * 1024 - 256


# ---- single writer: the pieces of a host plan ---------------------------------------

def _groups(rng, F1, m, sizes):
    """Candidates in apriori_gen's form: one prefix of m ids per entry of sizes, in
    lexicographic order, with that many ascending extensions above its last id."""
    top = F1 - max(sizes) - 1
    seen = set()
    while len(seen) < len(sizes):
        seen.add(tuple(sorted(rng.choice(top, m, replace=False).tolist())))
    prefix = np.array(sorted(seen), np.int32).reshape(len(sizes), m)
    ext, ext_off = [], np.zeros(len(sizes) + 1, np.int64)
    for g, s in enumerate(sizes):
        above = np.arange(prefix[g, -1] + 1, F1)
        ext.append(np.sort(rng.choice(above, s, replace=False)))
        ext_off[g + 1] = ext_off[g] + s
    return prefix, ext_off, np.concatenate(ext).astype(np.int32)


def piece_ranges_partition(rec_u32, passes, C):
    """Assert the invariant on 48-B records: per pass (piece begin, piece end, ext base), the
    ranges [a.x, a.x + n_ext) of its pieces tile [0, the pass's candidates)."""
    bounds = [int(e0) for _, _, e0 in passes] + [C]
    assert bounds[0] == 0 and bounds == sorted(bounds)
    for q, (a, b, e0) in enumerate(passes):
        r = rec_u32[a:b]
        n_ext = (r[:, 1] & 0xFF).astype(np.int64)
        live = n_ext > 0                               # class layouts pad wave rows with idle slots
        begin, n_ext = r[live, 0].astype(np.int64), n_ext[live]
        assert n_ext.max(initial=0) <= 8
        order = np.argsort(begin, kind="stable")
        begin, n_ext = begin[order], n_ext[order]
        Cq = bounds[q + 1] - bounds[q]
        # sorted by begin, each range starts where the one before ends: disjoint, no gap
        assert begin.size and begin[0] == 0 and int(begin[-1] + n_ext[-1]) == Cq, (q, Cq)
        assert np.array_equal(begin[1:], (begin + n_ext)[:-1]), q


SIZES = (1, 8, 9, 17, 1, 1, 1, 1, 1, 3, 16, 7, 1, 24, 2)      # pieces: 1, 1, 2, 3, ... per prefix


@pytest.mark.parametrize("accb", [1, 4])
@pytest.mark.parametrize("cls", [0, 2])
@pytest.mark.parametrize("lds_kb", [160, 8])
@pytest.mark.parametrize("m", [2, 4])
def test_host_plan_pieces_partition_every_pass(native, m, lds_kb, cls, accb):
    from fastapriori_amd.ops.primitives import level_plan_host
    rng = np.random.default_rng(10 * m + cls)
    F1 = 64
    prefix, ext_off, ext = _groups(rng, F1, m, SIZES * 24)
    C = int(ext.size)
    rc, info, passes, buf = level_plan_host(prefix, ext_off, ext, F1, 9, lds_bytes=lds_kb * 1024, cls=cls, accb=accb)
    assert rc == 0 and info[23] == (1 if cls else 0)
    assert (info[6] > 1) == (C > info[2])
    if lds_kb == 8:
        assert info[6] > 1 or accb == 1                # the small budget cuts the u32 plan into passes
    rec = buf[info[20]:info[20] + 12 * int(info[4])].view(np.uint32).reshape(-1, 12)
    assert passes[-1][1] == rec.shape[0]
    piece_ranges_partition(rec, passes.tolist(), C)
