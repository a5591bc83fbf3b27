"""The rule export with multi-item consequents on the device (csrc/hip/rules.hip k_rs_count /
k_rm_scan / k_rs_emit) against the C++ path, bit for bit: the mined case under every sort and
threshold set, workgroup edges, compaction across many workgroups and scan chunks, the
measures' corner cases, both errors through the error word, the shapes that launch nothing,
and a job on the device."""
import numpy as np
import pytest
import torch

from fastapriori_amd.ops import host
from fastapriori_amd.ops import primitives as prim

from test_condense import D, U, _mine, quest300
from test_rule_measures import HAND_BYTES, SORTS, THRESHOLDS, all_rules, little_to_do, small_lattice
from test_rule_splits import (CUBE_SPLIT_CONF, HAND_MULTI_BYTES, MFIELDS, as_multi, check_cube_threshold, check_errors,
                              check_hand_splits, check_repeated_token, cube_splits, edge_lattice, elements, msame,
                              splits, tie_pos)

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
NEW = ("fa_hip_rule_splits", "fa_hip_rule_splits_emit")


def on_device(res, **kw) -> host.MultiRuleMeasures:
    """ops.primitives.rule_splits_device, max_consequent = 1 included."""
    d = prim.rule_splits_device(res.levels, res.counts, res.n_lines, tie_pos(res), DEV, **kw)
    return host.MultiRuleMeasures(*[d[f].cpu().numpy() for f in MFIELDS])


@pytest.fixture
def calls(monkeypatch):
    """Every call of the export's launchers in the test, by name."""
    seen = []
    lib = prim._native.hip()
    for name in NEW + ("fa_hip_rule_measures", "fa_hip_rule_measures_emit", "fa_hip_rule_measures_fin"):
        fn = getattr(lib, name)
        monkeypatch.setattr(lib, name, lambda *a, _fn=fn, _n=name: seen.append(_n) or _fn(*a))
    return seen


@pytest.mark.parametrize("M", [1, 2, 3, 9])
def test_device_equals_cpp_on_the_mined_case(M, calls):
    res = quest300()[0]
    assert len(res.levels) == 10
    prim.reset_fallbacks()
    sizes = set()
    for sort in SORTS:
        for th in THRESHOLDS:
            del calls[:]
            got = on_device(res, max_consequent=M, sort=sort, **th)
            msame(got, splits(res, max_consequent=M, sort=sort, **th))
            assert calls.count("fa_hip_rule_splits") == 1, (M, sort, th)           # one selection pass for ten levels
            assert calls.count("fa_hip_rule_splits_emit") <= 1 and calls.count("fa_hip_rule_measures_fin") <= 1
            assert "fa_hip_rule_measures" not in calls
            sizes.add(got.n_rules)
    assert elements(res, M) in sizes and len(sizes) >= 4
    assert not prim.FALLBACKS


def test_limits_and_the_public_interface(calls):
    res = quest300()[0]
    prim.reset_fallbacks()
    R = splits(res, max_consequent=2, min_confidence=0.5, sort="lift").n_rules
    for limit in (0, 1, R - 1, R, R + 1):
        kw = dict(max_consequent=2, min_confidence=0.5, sort="lift", limit=limit)
        msame(on_device(res, **kw), splits(res, **kw))
    assert not prim.FALLBACKS
    # through AssociationRules: the new launchers at M >= 2 only
    del calls[:]
    msame(all_rules(res, device=DEV, max_consequent=2), splits(res, max_consequent=2))
    assert calls[:2] == list(NEW)
    del calls[:]
    all_rules(res, device=DEV)
    assert calls and not set(calls) & set(NEW)


def test_device_tensors_and_the_hand_example():
    res = _mine(D, 0.5)
    rm = prim.rule_splits_device(res.levels, res.counts, res.n_lines, np.arange(3), DEV, max_consequent=2)
    assert sorted(rm) == sorted(MFIELDS) and all(v.device.type == "cuda" for v in rm.values())
    assert rm["cnt_s"].numel() == 12 and rm["cons_off"].tolist()[-1] == rm["cons"].numel() == 15
    check_hand_splits(on_device(res, max_consequent=2), res)
    msame(on_device(res, max_consequent=1), as_multi(all_rules(res)))


@pytest.mark.parametrize("one_more_pair", [False, True], ids=["full_last_workgroup", "two_threads_in_the_last"])
def test_workgroup_edges(one_more_pair):
    res = edge_lattice(one_more_pair)             # 6144 = 24 x 256 (itemset, split) threads, or 6146
    for kw in (dict(), dict(min_confidence=0.75, sort="leverage")):
        want = splits(res, max_consequent=7, **kw)
        msame(on_device(res, max_consequent=7, **kw), want)
    assert 0 < want.n_rules < 6144 and splits(res, max_consequent=7).n_rules == (6146 if one_more_pair else 6144)


def test_compaction_across_workgroups_and_scan_chunks():
    res, _ = cube_splits()
    per_wg = check_cube_threshold()               # some workgroups select nothing, some all 256, most a part
    kw = dict(max_consequent=11, min_confidence=CUBE_SPLIT_CONF, sort="lift")
    want = splits(res, **kw)
    assert want.n_rules == int(per_wg.sum())
    msame(on_device(res, **kw), want)
    # the compacted enumeration order itself: two runs place alike (no atomics in the placement)
    kw = dict(max_consequent=11, min_confidence=CUBE_SPLIT_CONF, sort="support", limit=100000)
    a, b = (prim.rule_splits_device(res.levels, res.counts, res.n_lines, tie_pos(res), DEV, **kw) for _ in range(2))
    assert all(torch.equal(a[f], b[f]) for f in MFIELDS)


def test_measures_on_the_device():
    res = small_lattice()                         # N = 2^31 - 1, products near 2^61, at all splits
    for sort in ("leverage", "conviction", "lift"):
        msame(on_device(res, max_consequent=10, sort=sort), splits(res, max_consequent=10, sort=sort))
    check_repeated_token(on_device)


def test_errors_arrive_through_the_error_word(calls):
    check_errors(on_device)
    assert calls == ["fa_hip_rule_splits"] * 4                             # read before anything is emitted
    res = _mine(D, 0.5)
    check_hand_splits(on_device(res, max_consequent=2), res)               # the next call starts from a zero word


@pytest.mark.parametrize("name", sorted(little_to_do()))
def test_shapes_that_launch_little_or_nothing(name, calls):
    res, n = little_to_do()[name]
    rm = prim.rule_splits_device(res.levels, res.counts, res.n_lines, np.arange(3), DEV, max_consequent=2)
    assert all(v.device.type == "cuda" for v in rm.values()) and rm["cnt_s"].numel() == n
    msame(on_device(res, max_consequent=2), as_multi(all_rules(res)))
    if n == 0:
        # no level 2, or an empty one: the launcher returns before any launch, nothing is emitted
        assert set(calls) == {"fa_hip_rule_splits"} and rm["cons_off"].tolist() == [0] == rm["ante_off"].tolist()


def test_job_on_the_device(tmp_path, calls):
    from fastapriori_amd.config import JobConfig
    from fastapriori_amd.parallel.comm import Comm
    from fastapriori_amd.pipeline import run_job
    (tmp_path / "D.dat").write_text(D)
    (tmp_path / "U.dat").write_text(U)
    job = dict(input=f"{tmp_path}/", min_support=0.5, device="cuda", rules=True)
    s = run_job(JobConfig(**job, output=f"{tmp_path}/o_", rules_max_consequent=2), Comm(device=DEV))
    assert s["n_rules_exported"] == 12 and s["rules_max_consequent"] == 2
    assert (tmp_path / "o_rules" / "part-00000").read_bytes() == HAND_MULTI_BYTES
    assert calls == ["fa_hip_rule_splits", "fa_hip_rule_splits_emit", "fa_hip_rule_measures_fin"]
    del calls[:]
    s0 = run_job(JobConfig(**job, output=f"{tmp_path}/p_"), Comm(device=DEV))
    assert s0["n_rules_exported"] == 9 and (tmp_path / "p_rules" / "part-00000").read_bytes() == HAND_BYTES
    assert calls == ["fa_hip_rule_measures", "fa_hip_rule_measures_emit", "fa_hip_rule_measures_fin"]
    assert (tmp_path / "o_recommends" / "part-00000").read_bytes() == \
        (tmp_path / "p_recommends" / "part-00000").read_bytes()
