"""The query counter on the device (csrc/hip/query.hip k_query_slab through
ops.primitives.query_count) against the C++ path on the same plan and against brute
force, at the shapes where the kernel can go wrong: every slab width, row counts around
the word and tile edges, a row longer than the workgroup's stride, several windows of
different widths, one workgroup over every tile and more workgroups than tiles, and the
launcher's limits.  Every comparison is exact integer equality."""
import numpy as np
import pytest
import torch

from fastapriori_amd.parallel.launch import spawn_local

pytestmark = pytest.mark.gpu
WIDTHS = (16, 8, 4, 2, 1)


def _csr(M: np.ndarray, ids: np.ndarray | None = None):
    """CSR (offsets int64, items int32) of a boolean [rows, items] matrix; ids: the raw id
    of every column (default: its index)."""
    r, c = np.nonzero(M)
    off = np.zeros(M.shape[0] + 1, dtype=np.int64)
    np.cumsum(M.sum(axis=1), out=off[1:])
    items = (c if ids is None else ids[c]).astype(np.int32)
    return torch.from_numpy(off), torch.from_numpy(items)


def _plan(rows, n_used, acc=None, lds=None):
    from fastapriori_amd.ops import primitives as prim
    off = np.zeros(len(rows) + 1, dtype=np.int64)
    off[1:] = np.cumsum([len(r) for r in rows])
    idx = np.concatenate([np.sort(np.asarray(r)) for r in rows]).astype(np.int32)
    return prim.query_plan(off, idx, np.arange(len(rows), dtype=np.int64), n_used, len(rows), acc=acc, lds=lds)


def _both(off, items, lut, plan, **kw):
    """(device counts, C++ counts) of one plan."""
    from fastapriori_amd.ops import primitives as prim
    dev = torch.device("cuda", 0)
    got = prim.query_count(off.to(dev), items.to(dev), lut.to(dev), plan, **kw).cpu().numpy()
    return got, prim.query_count(off, items, lut, plan).numpy()


def _brute(M: np.ndarray, rows) -> np.ndarray:
    return np.array([int(M[:, np.asarray(r)].all(axis=1).sum()) for r in rows], dtype=np.int64)


def _queries40(rng):
    rows = [[i] for i in range(40)]
    rows += [rng.choice(40, size=k, replace=False).tolist() for k in (2, 3, 5) for _ in range(60)]
    rows += [list(range(40)), [39, 0], [0, 39]]
    return rows


@pytest.mark.parametrize("sw", WIDTHS)
def test_every_width_at_the_word_and_tile_edges(sw):
    """Dense random rows over 40 items; lines 0, 63 and the tile's last line hold every
    item, so the 40-item query counts exactly the ones present."""
    from fastapriori_amd.ops import primitives as prim
    rng = np.random.default_rng(sw)
    rows = _queries40(rng)
    lds = prim.query_window_lds(40, sw, len(rows))                   # the width's exact footprint
    plan = _plan(rows, 40, lds=lds)
    assert plan["wins"].shape[0] == 1 and int(plan["wins"][0, 2]) == sw
    lut = torch.arange(40, dtype=torch.int32)
    tile = 64 * sw
    for n in sorted({1, 63, 64, 65, tile - 1, tile, tile + 1, 2 * tile + 3}):
        M = rng.random((n, 40)) < 0.6
        full = sorted({r for r in (0, 63, tile - 1, tile, 2 * tile + 2) if r < n})
        M[full] = True
        M[rng.integers(0, n)] |= rng.random(40) < 0.5
        off, items = _csr(M)
        got, cpu = _both(off, items, lut, plan)
        want = _brute(M, rows)
        assert np.array_equal(got, want) and np.array_equal(cpu, want), (sw, n)
        assert want[-3] >= len(full)


def test_a_row_longer_than_the_stride_and_ids_no_query_uses():
    """One line of 3000 distinct ids among short lines: its items are streamed in three
    strides of 1024 positions.  Most ids are in no query (lut -1), some are in the lut but
    in a dead query's place only."""
    rng = np.random.default_rng(7)
    V, n = 3500, 200
    M = np.zeros((n, V), dtype=bool)
    for r in range(n):
        M[r, rng.choice(V, size=int(rng.integers(0, 6)), replace=False)] = True
    M[77] = False
    M[77, rng.choice(V, size=3000, replace=False)] = True
    long_ids = np.flatnonzero(M[77])
    used = np.unique(np.concatenate([long_ids[[0, 1, 1023, 1024, 1025, 2047, 2048, 2999]],
                                     rng.choice(V, size=30, replace=False)]))
    lut = np.full(V, -1, dtype=np.int32)
    lut[used] = np.arange(len(used), dtype=np.int32)
    # two more ids of the long line are in the lut but in no window (a dead query's tokens)
    spare = np.setdiff1d(long_ids, used)[[5, 1500]]
    lut[spare] = len(used) + np.arange(2, dtype=np.int32)
    rows = [[i] for i in range(len(used))]
    rows += [rng.choice(len(used), size=2, replace=False).tolist() for _ in range(50)]
    rows += [np.searchsorted(used, long_ids[[0, 1023, 1024, 2048, 2999]]).tolist()]
    plan = _plan(rows, len(used) + 2)
    off, items = _csr(M)
    got, cpu = _both(off, items, torch.from_numpy(lut), plan)
    want = _brute(M[:, used], rows)
    assert np.array_equal(got, want) and np.array_equal(cpu, want)
    assert want[-1] >= 1 and int(off[78] - off[77]) == 3000


@pytest.mark.parametrize("acc", [1, 3, 1025])
def test_windows_of_forced_sizes(acc):
    """acc = 1025: more queries than threads, so a thread owns two accumulators."""
    rng = np.random.default_rng(acc)
    n_items, n = 60, 700
    rows = [[i] for i in range(n_items)]
    rows += [rng.choice(n_items, size=int(rng.integers(1, 5)), replace=False).tolist()
             for _ in range(1300 if acc == 1025 else 80)]
    plan = _plan(rows, n_items, acc=acc)
    W = plan["wins"].shape[0]
    assert W == -(-len(rows) // acc) and int(plan["wins"][:, 0].max()) == min(acc, len(rows))
    M = rng.random((n, n_items)) < 0.3
    off, items = _csr(M)
    got, cpu = _both(off, items, torch.arange(n_items, dtype=torch.int32), plan)
    want = _brute(M, rows)
    assert np.array_equal(got, want) and np.array_equal(cpu, want)


def test_two_widths_in_one_launch_and_a_window_of_one_single_item_query():
    from fastapriori_amd.ops import primitives as prim
    rng = np.random.default_rng(11)
    a = [rng.choice(10, size=int(rng.integers(1, 4)), replace=False).tolist() for _ in range(30)]
    b = [(10 + rng.choice(400, size=int(rng.integers(1, 4)), replace=False)).tolist() for _ in range(29)]
    b[0] = list(range(10, 410))[::2]                                  # 200 items: b holds all 400 between them
    b[1] = list(range(10, 410))[1::2]
    rows = a + b + [[410]]                                            # sorts last: a window of its own below
    lds = prim.query_window_lds(400, 1, 30)
    plan = _plan(rows, 411, acc=30, lds=lds)
    wins = plan["wins"].numpy()
    assert wins[:, 0].tolist() == [30, 29, 1] and wins[2, 1] == 1    # n_q per window; one query of one item
    assert len(set(wins[:, 2].tolist())) >= 2 and wins[1, 2] == 1    # different widths in the one launch
    n = 1500
    M = rng.random((n, 411)) < 0.2
    M[:, 10:410] |= rng.random((n, 400)) < 0.7
    M[5] = True
    off, items = _csr(M)
    got, cpu = _both(off, items, torch.arange(411, dtype=torch.int32), plan)
    want = _brute(M, rows)
    assert np.array_equal(got, want) and np.array_equal(cpu, want)
    assert want[30] >= 1 and want[-1] > 0


@pytest.mark.parametrize("max_wg", [1, 4096])
def test_one_workgroup_over_every_tile_and_more_workgroups_than_tiles(max_wg):
    from fastapriori_amd.ops import primitives as prim
    rng = np.random.default_rng(3)
    rows = _queries40(rng)
    plan = _plan(rows, 40, lds=prim.query_window_lds(40, 2, len(rows)))
    assert int(plan["wins"][0, 2]) == 2
    n = 128 * 9 + 17                                                  # 10 tiles of 128 rows
    M = rng.random((n, 40)) < 0.5
    off, items = _csr(M)
    got, cpu = _both(off, items, torch.arange(40, dtype=torch.int32), plan, max_wg=max_wg)
    want = _brute(M, rows)
    assert np.array_equal(got, want) and np.array_equal(cpu, want)


def _hand_plan(n_q, n_items, sw, lds, n_used=None):
    """One window whose queries are single items i % n_items, with tensors of the sizes its
    descriptor asks for."""
    n_used = n_items if n_used is None else n_used
    wins = torch.tensor([[n_q, n_items, sw, 0, 0, 0, 0, 0]], dtype=torch.int64)
    tab = torch.arange(n_used, dtype=torch.int32).clamp(max=max(n_items, 1) - 1).to(torch.uint16)
    return {"wins": wins, "tab": tab, "qoff": torch.arange(n_q + 1, dtype=torch.int32),
            "qrow": (torch.arange(n_q, dtype=torch.int32) % max(n_items, 1)).to(torch.uint16),
            "perm": torch.arange(n_q, dtype=torch.int64), "n_queries": n_q, "n_used": n_used, "lds": lds}


def test_launcher_refuses_one_past_each_limit_and_accepts_the_limit():
    from fastapriori_amd.ops import primitives as prim
    L = prim.query_limits()
    dev = torch.device("cuda", 0)
    M = np.zeros((70, 8), dtype=bool)
    M[::2, 0] = M[::3, 1] = M[5, 7] = True
    off, items = _csr(M)
    off, items = off.to(dev), items.to(dev)

    def run(plan, n_lut):
        return prim.query_count(off, items, torch.arange(n_lut, dtype=torch.int32, device=dev) % plan["n_used"],
                                plan).cpu().numpy()

    def want(n_q, n_items):
        col = M.sum(axis=0)
        return np.array([int(col[i % n_items]) if i % n_items < 8 else 0 for i in range(n_q)], dtype=np.int64)

    big = L.kQLdsMax
    # queries per window: kQAcc is taken, one more is refused
    assert np.array_equal(run(_hand_plan(L.kQAcc, 8, 1, big), 8), want(L.kQAcc, 8))
    with pytest.raises(ValueError, match="limits"):
        run(_hand_plan(L.kQAcc + 1, 8, 1, big), 8)
    # LDS: the largest launch, one byte more
    with pytest.raises(ValueError, match="limits"):
        run(_hand_plan(4, 8, 1, big + 1), 8)
    # items: the most that fit kQLdsMax beside one query at width 1, one more, and one past the u16 rows
    top = (big - prim.query_window_lds(0, 1, 1)) // 8
    assert prim.query_window_lds(top, 1, 1) <= big < prim.query_window_lds(top + 1, 1, 1) and top < L.kQMaxItems
    assert np.array_equal(run(_hand_plan(3, top, 1, big), top), want(3, top))
    with pytest.raises(ValueError, match="limits"):
        run(_hand_plan(3, top + 1, 1, big), top + 1)
    with pytest.raises(ValueError, match="limits"):
        run(_hand_plan(3, L.kQMaxItems + 1, 1, big, n_used=L.kQMaxItems + 1), L.kQMaxItems + 1)
    # a window whose footprint exceeds the launch's LDS by one step
    fit = prim.query_window_lds(8, 4, 4)
    assert np.array_equal(run(_hand_plan(4, 8, 4, fit), 8), want(4, 8))
    with pytest.raises(ValueError, match="limits"):
        run(_hand_plan(4, 8, 4, fit - 16), 8)
    # widths: the widest is taken, the next power of two and a non-power are refused; no queries, no items
    assert np.array_equal(run(_hand_plan(4, 8, L.kQMaxWidth, big), 8), want(4, 8))
    for sw in (2 * L.kQMaxWidth, 3, 0):
        with pytest.raises(ValueError, match="limits"):
            run(_hand_plan(4, 8, sw, big), 8)
    for n_q, n_items in ((0, 8), (4, 0)):
        with pytest.raises(ValueError, match="limits"):
            run(_hand_plan(n_q, n_items, 1, big, n_used=8), 8)


def test_mined_itemsets_recount_to_their_counts_on_the_device(tmp_path_factory):
    from test_query_count import _q20k, check_mined_recount
    d, ms = _q20k(tmp_path_factory)
    res = check_mined_recount(d, ms, "cuda")
    assert len(res.levels) >= 14


def test_job_verifies_its_counts_on_the_device(tmp_path, capsys):
    from fastapriori_amd.config import JobConfig
    from fastapriori_amd.parallel.comm import Comm
    from fastapriori_amd.pipeline import run_job
    from fastapriori_amd.utils.io import write_quest_file
    write_quest_file(str(tmp_path / "D.dat"), 5000, 9.0, 4.0, 40, 40, seed=3)
    write_quest_file(str(tmp_path / "U.dat"), 300, 9.0, 4.0, 40, 40, seed=3, users=True)
    (tmp_path / "q.dat").write_text("1 2\n3\n\n1 999999\n")
    s = run_job(JobConfig(input=f"{tmp_path}/", output=f"{tmp_path}/o_", min_support=0.02, device="cuda",
                          verify_counts=True, count_itemsets=str(tmp_path / "q.dat")),
                Comm(device=torch.device("cuda", 0)))
    assert s["n_verified"] > 100 and s["n_counted"] == 4
    assert f"==== verified {s['n_verified']} itemset counts" in capsys.readouterr().out
    got = (tmp_path / "o_itemsetCounts" / "part-00000").read_text().splitlines()
    lines = [set(l.split()) for l in open(tmp_path / "D.dat").read().splitlines()]
    assert got == [f"1 2[{sum(1 for l in lines if {'1', '2'} <= l)}]", f"3[{sum(1 for l in lines if '3' in l)}]",
                   f"[{sum(1 for l in lines if not l)}]", "1 999999[0]"]


@pytest.mark.parametrize("strategy", ["count", "candidate"])
def test_two_ranks_on_the_device(tmp_path, strategy):
    from test_query_count import _rank_counts, ranks_case
    path, qs, want = ranks_case(tmp_path, "dict")
    outs = spawn_local(_rank_counts, 2, path, qs, strategy, "cuda", {"query_acc": 50},
                       env={"FA_DIST_BACKEND": "gloo"}, timeout=300)
    for got, _ in outs:
        assert got == want
