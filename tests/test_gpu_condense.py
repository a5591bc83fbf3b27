"""Closed / maximal marks on the device: k_sup_mark (csrc/hip/condense.hip) against the C++
path on a mined result and against flags derived by hand on an analytic lattice, the shapes
that launch nothing, and MiningResult.condensed on the device."""
import pytest
import torch

from fastapriori_amd.ops import primitives as prim

from test_condense import check_flags, edge_cases, lattice, quest300

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)


@pytest.fixture
def calls(monkeypatch):
    """Every fa_hip_sup_mark call of the test, by name."""
    seen = []
    fn = prim._native.hip().fa_hip_sup_mark
    monkeypatch.setattr(prim._native.hip(), "fa_hip_sup_mark", lambda *a: seen.append("fa_hip_sup_mark") or fn(*a))
    return seen


def test_device_equals_host_on_the_mined_case(calls):
    res, _, _ = quest300()
    ref = prim.condense_flags(res.levels, res.counts, "cpu")
    prim.reset_fallbacks()
    got = prim.condense_flags(res.levels, res.counts, DEV)
    assert len(got) == len(ref) == 10
    for k, ((sup, eq), (rsup, req)) in enumerate(zip(got, ref), 1):
        assert sup.device.type == "cuda" and eq.device.type == "cuda" and sup.dtype == eq.dtype == torch.uint8
        assert torch.equal(sup.cpu(), rsup) and torch.equal(eq.cpu(), req), k
        if k < 10:
            assert 0 < int(req.sum()) < req.numel()                       # both branches, every level
    assert not prim.FALLBACKS
    assert calls == ["fa_hip_sup_mark"]                                   # one launch for ten levels


@pytest.mark.parametrize("with_16_17", [False, True], ids=["full_last_workgroup", "two_threads_in_the_last"])
def test_analytic_lattice(calls, with_16_17):
    # 11264 = 44 x 256 (itemset, position) threads, or 11266: see test_condense.lattice
    levels, counts, want = lattice(with_16_17)
    check_flags(prim.condense_flags(levels, counts, DEV), want)
    assert calls == ["fa_hip_sup_mark"]


@pytest.mark.parametrize("name", ["level1_only", "empty_level2", "trailing_empty"])
def test_shapes_with_little_or_nothing_to_launch(name):
    levels, counts, want = edge_cases()[name]
    got = prim.condense_flags(levels, counts, DEV)
    assert [(s.cpu().tolist(), e.cpu().tolist()) for s, e in got] == want
    assert all(s.device.type == "cuda" for s, _ in got)
    if name != "trailing_empty":
        # no level 2, or an empty one: the launcher returns before any launch (all zeros, no error)
        assert all(not any(s) and not any(e) for s, e in want)


def test_job_on_the_device_writes_both_forms(tmp_path, calls):
    from fastapriori_amd.config import JobConfig
    from fastapriori_amd.parallel.comm import Comm
    from fastapriori_amd.pipeline import run_job
    from test_condense import CLOSED, MAXIMAL, D, U, _read
    (tmp_path / "D.dat").write_text(D)
    (tmp_path / "U.dat").write_text(U)
    s = run_job(JobConfig(input=f"{tmp_path}/", output=f"{tmp_path}/o_", min_support=0.5, device="cuda", closed=True,
                          maximal=True), Comm(device=DEV))
    assert (s["n_itemsets"], s["n_closed"], s["n_maximal"]) == (7, 3, 1)
    assert _read(tmp_path / "o_closedItemset" / "part-00000") == CLOSED
    assert _read(tmp_path / "o_maximalItemset" / "part-00000") == MAXIMAL
    assert calls == ["fa_hip_sup_mark"] * 2                               # one launch per form


@pytest.mark.parametrize("kind", ["closed", "maximal"])
def test_condensed_on_the_device_equals_the_cpu_call(kind):
    res, closed, maximal = quest300()
    ref = closed if kind == "closed" else maximal
    got = res.condensed(kind, device=DEV)
    assert got.digest() == ref.digest() and got.n_itemsets == ref.n_itemsets
    assert got.stats == ref.stats and [l.shape for l in got.levels] == [l.shape for l in ref.levels]
