"""The regrouping step of one-pass device bundles on the device (csrc/hip/regroup.hip:
k_dl_regroup, k_dl_unpermute; reached by the miner inside the post step, gen.hip dl_post).

* the device's regrouped level tables and permutation equal the host model's
  (ops.host.dl_regroup) on the cases of tests/test_regroup_rule.py: parents, extension
  lists, perm, the statistics;
* the regrouped plan, counted and un-permuted, equals the prefix plan's counts and the
  supports computed in numpy from a dense 0/1 matrix, with byte, u16 and u32 accumulators
  over three 16-word slabs (the last one partial) walked by two workgroups;
* a mined run with the knob on equals the C++ CPU miner and the knob-off run, on one rank and
  on two.
"""
import functools

import numpy as np
import pytest
import torch

from fastapriori_amd.ops import _native, host
from fastapriori_amd.ops import primitives as prim
from test_gen_edges import bundle_case, run_bundle
from test_kernel_edges import _csr
from test_regroup_rule import CASES, model_levels, pieces, regroup_case

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)


@pytest.fixture(scope="module")
def dl_state():
    return prim.DeviceLevelState(DEV)


def _at(buf, ptr, count, dtype):
    """count values of dtype at the device address ptr inside the uint8 tensor buf."""
    o, nb = int(ptr) - buf.data_ptr(), count * np.dtype(dtype).itemsize
    assert 0 <= o and o + nb <= buf.numel()
    return buf[o:o + nb].cpu().numpy().view(dtype)


@pytest.mark.parametrize("case", CASES)
def test_device_equals_model(dl_state, case):
    S, K = dl_state, prim.dl()
    F1, ch, L = regroup_case(case)
    c, P0 = run_bundle(S, F1, ch, L, 8.0)
    assert c[K.kDlLevels] == L
    regrouped, want = host.dl_regroup(model_levels(ch, L))
    got = prim.dl_regroup(S, L, DEV)
    if not regrouped:
        assert got is None and case == "m12_m13"
        return
    stats, perm = got["stats"].cpu().numpy(), got["perm"].cpu().numpy()
    base = 0
    for l, ((rows, cnt, cand), o) in enumerate(zip(ch[:L], want)):
        n, C, d, d0 = len(rows), len(cand), got["desc"][l], S.desc[l]
        assert all(d[f] == d0[f] for f in ("P", "rows", "m", "n", "C", "base")) and d0["base"] == base
        assert stats[l].tolist() == [o["pieces_prefix"], o["pieces_rule"], o["rounds"], o["kept_prefix"]], l
        if n > _native.host().fa_dl_regroup_const(0):
            # more parent rows than a level regroups with: the generator's own table, identity
            assert case == "rows12300" and d["cnt"] == d0["cnt"] and d["off"] == d0["off"]
            assert np.array_equal(perm[base:base + C], base + np.arange(C)) and o["kept_prefix"]
            base += C
            continue
        assert np.array_equal(_at(got["scratch"], d["cnt"], n, np.int32), o["cnt"]), l
        assert np.array_equal(_at(got["scratch"], d["off"], n + 1, np.int64), o["off"]), l
        assert np.array_equal(_at(got["scratch"], d["cnt"] + 4 * n, C, np.int32), o["ex"]), l
        assert np.array_equal(perm[base:base + C] - base, o["perm"]), l
        assert stats[l].tolist() == [o["pieces_prefix"], o["pieces_rule"], o["rounds"], o["kept_prefix"]], l
        base += C
    again = prim.dl_regroup(S, L, DEV)
    assert torch.equal(again["perm"], got["perm"])
    del P0


@functools.lru_cache(maxsize=None)
def _count_case():
    """40 items, 3,000 dense rows: (F1, chain, B, supports of the C(40, 3) candidates)."""
    F1, ch = bundle_case("lat40_F70", 1)
    T = 3000
    rng = np.random.default_rng(40)
    B = (rng.random((T, F1)) < 0.3).astype(np.int64)
    B[np.ix_(np.arange(T) % 8 < 2, np.unique(ch[0][0]))] = 1
    B[B.sum(1) < 2, :2] = 1
    ref = B.astype(bool)[:, ch[0][2]].all(2).sum(0).astype(np.int64)
    return F1, ch, B, ref


@pytest.mark.parametrize("accb", [1.0, 2.0, 4.0], ids=["byte", "u16", "u32"])
def test_regrouped_counts(dl_state, tune, accb):
    S, K = dl_state, prim.dl()
    F1, ch, B, ref = _count_case()
    T, C = B.shape[0], len(ref)
    assert np.unique(ch[0][0]).size == 40 and (T + 63) // 64 == 47 and ref.max() > 255
    tune(lane_deal_min_rows=-1)
    c, P0 = run_bundle(S, F1, ch, 1, 1.0)
    n_used = int(c[K.kDlNUsed])
    roff, ranks = _csr(B)
    roff, ranks = roff.to(DEV), ranks.to(DEV)
    rg = prim.dl_regroup(S, 1, DEV)
    want = host.dl_regroup(model_levels(ch, 1))[1][0]
    assert not want["kept_prefix"] and pieces(want["cnt"]) < want["pieces_prefix"]
    hip = _native.hip()
    hip.fa_hip_debug_slab_max_wg(2)                # two workgroups share the three slabs
    try:
        plan0 = prim.dl_plan(S, 1, F1, n_used, C, prim.dl_lds_budget(F1), DEV, accb=accb)
        assert plan0["sw"] == 16 and plan0["accb"] == accb
        off = prim.dl_count(S, plan0, roff, ranks, None, T, F1, None).cpu().numpy()
        assert int(S.ctl[K.kDlPieces].item()) == want["pieces_prefix"]
        plan = prim.dl_plan(S, 1, F1, n_used, C, prim.dl_lds_budget(F1), DEV, accb=accb, desc=rg["desc"])
        raw = prim.dl_count(S, plan, roff, ranks, None, T, F1, None)
        assert int(S.ctl[K.kDlPieces].item()) == pieces(want["cnt"])
        on = prim.dl_unpermute(raw, rg["perm"]).cpu().numpy()
    finally:
        hip.fa_hip_debug_slab_max_wg(0)
    assert np.array_equal(off.astype(np.int64), ref)
    assert np.array_equal(raw.cpu().numpy().astype(np.int64), ref[want["perm"]])     # the un-permute is exact
    assert np.array_equal(on.astype(np.int64), ref)
    del P0


# ---- mined runs ------------------------------------------------------------------------
MS = 0.002


@functools.lru_cache(maxsize=None)
def _mined_ref():
    from fastapriori_amd.models.apriori import FastApriori, MinerConfig
    from fastapriori_amd.parallel.comm import Comm
    from fastapriori_amd.utils.io import generate_shard
    from fastapriori_amd.utils.metrics import Logger
    cpu = generate_shard(200_000, Comm(), "cpu", 10.0, 4.0, 2000, 1000, 4)
    ref = FastApriori(MS, config=MinerConfig(min_support=MS), logger=Logger(0, enabled=False)).run(cpu)
    return cpu, ref


def _mine(cpu):
    from fastapriori_amd.models.apriori import FastApriori, MinerConfig
    from fastapriori_amd.utils.metrics import Logger
    m = FastApriori(MS, config=MinerConfig(min_support=MS), logger=Logger(0, enabled=False))
    res = m.run(cpu.to(DEV))
    return res, m.stats


def test_mined_run_equals_cpu_miner(tune):
    cpu, ref = _mined_ref()
    tune(dl_regroup=False, dl_regroup_min_rows=0)
    n0, _ = prim.dl_regroup_last()
    off, st0 = _mine(cpu)
    assert prim.dl_regroup_last()[0] == n0                 # knob off: no bundle regroups
    tune(dl_regroup=True)
    on, st = _mine(cpu)
    n1, stats = prim.dl_regroup_last()
    assert n1 > n0 and st["device_bundles"] >= 1 and "fallbacks" not in st, st
    assert stats is not None and (stats[:, 3] == 0).any()   # a level of the last bundle regrouped
    kept = stats[:, 3] == 1
    assert np.all(stats[~kept, 1] < stats[~kept, 0]) and np.all(stats[kept, 1] >= stats[kept, 0])
    assert st["device_bundle_shapes"] == st0["device_bundle_shapes"] and st["level_info"] == st0["level_info"]
    assert len(ref.levels) >= 4 and [len(x) for x in on.levels] == [len(x) for x in ref.levels]
    for a, b, r in zip(on.levels, off.levels, ref.levels):
        assert np.array_equal(a, r) and np.array_equal(b, r)
    for a, b, r in zip(on.counts, off.counts, ref.counts):
        assert np.array_equal(a, r) and np.array_equal(b, r)
    assert on.as_dict() == off.as_dict() == ref.as_dict()


def _rank(n, tune_spec):
    from fastapriori_amd.models.apriori import FastApriori, MinerConfig
    from fastapriori_amd.parallel.comm import init_comm, shutdown_comm
    from fastapriori_amd.tuning import TUNING
    from fastapriori_amd.utils.io import generate_shard
    from fastapriori_amd.utils.metrics import Logger
    TUNING.apply(tune_spec)
    comm = init_comm("cuda")
    try:
        sh = generate_shard(n, comm, comm.device, 10.0, 4.0, 2000, 1000, seed=4)
        m = FastApriori(MS, comm, MinerConfig(min_support=MS), Logger(comm.rank, enabled=False))
        res = m.run(sh)
        return dict(sets=res.as_dict(), world=comm.world_size, regrouped=prim.dl_regroup_last()[0],
                    shapes=m.stats["device_bundle_shapes"])
    finally:
        shutdown_comm(comm)


def test_two_ranks_match_one():
    from fastapriori_amd.parallel.launch import spawn_local
    env = {"FA_DIST_BACKEND": "gloo"}
    one = spawn_local(_rank, 1, 40_000, "dl_regroup=1,dl_regroup_min_rows=0", env=env)[0]
    off = spawn_local(_rank, 2, 40_000, "dl_regroup=0", env=env)
    on = spawn_local(_rank, 2, 40_000, "dl_regroup=1,dl_regroup_min_rows=0", env=env)
    gated = spawn_local(_rank, 2, 40_000, "dl_regroup=1,dl_regroup_min_rows=20001", env=env)
    assert all(g["regrouped"] == 0 and g["sets"] == one["sets"] for g in gated)   # 20,000 lines per rank
    assert one["regrouped"] >= 1
    for o, f in zip(on, off):
        assert o["world"] == 2 and o["regrouped"] >= 1 and f["regrouped"] == 0
        assert o["sets"] == f["sets"] == one["sets"] and o["shapes"] == f["shapes"]
