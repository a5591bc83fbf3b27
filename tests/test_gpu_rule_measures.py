"""The rule export on the device (csrc/hip/rules.hip k_rm_count / k_rm_scan / k_rm_emit /
k_rm_fin) against the C++ path, bit for bit: the mined case under every sort and threshold
set, workgroup edges, compaction across many workgroups and scan chunks, the measures'
corner cases, the shapes that launch nothing, and a job on the device."""
import numpy as np
import pytest
import torch

from fastapriori_amd.ops import primitives as prim

from test_condense import D, U, _mine, quest300
from test_rule_measures import (CUBE_CONF, FIELDS, HAND_BYTES, SORTS, THRESHOLDS, all_rules, check_hand,
                                check_large_counts, check_repeated_token, check_thresholds, cube, little_to_do,
                                missing_subset, same, small_lattice)

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)


def on_device(res, **kw):
    return all_rules(res, device=DEV, **kw)


@pytest.fixture
def calls(monkeypatch):
    """Every fa_hip_rule_measures* call of the test, by name."""
    seen = []
    lib = prim._native.hip()
    for name in ("fa_hip_rule_measures", "fa_hip_rule_measures_emit", "fa_hip_rule_measures_fin"):
        fn = getattr(lib, name)
        monkeypatch.setattr(lib, name, lambda *a, _fn=fn, _n=name: seen.append(_n) or _fn(*a))
    return seen


def test_device_equals_cpp_on_the_mined_case(calls):
    res = quest300()[0]
    assert len(res.levels) == 10
    prim.reset_fallbacks()
    cases = [dict(th, sort=sort) for sort in SORTS for th in THRESHOLDS]
    R = all_rules(res, min_confidence=0.5, sort="lift").n_rules
    cases += [dict(min_confidence=0.5, sort="lift", limit=limit) for limit in (0, 1, R - 1, R, R + 1)]
    sizes = set()
    for kw in cases:
        del calls[:]
        got = on_device(res, **kw)
        same(got, all_rules(res, **kw))
        assert calls.count("fa_hip_rule_measures") == 1, kw           # one selection pass for ten levels
        assert calls.count("fa_hip_rule_measures_emit") <= 1 and calls.count("fa_hip_rule_measures_fin") <= 1
        sizes.add(got.n_rules)
    assert 0 in sizes and len(sizes) > 6
    assert not prim.FALLBACKS


def test_device_tensors():
    res = _mine(D, 0.5)
    rm = prim.rule_measures_device(res.levels, res.counts, res.n_lines, np.arange(3), DEV)
    assert sorted(rm) == sorted(FIELDS)
    assert all(v.device.type == "cuda" for v in rm.values())
    assert rm["cons"].numel() == 9 and rm["ante_off"].tolist()[-1] == rm["ante"].numel() == 12
    check_hand(on_device(res), res)


@pytest.mark.parametrize("with_16_17", [False, True], ids=["full_last_workgroup", "two_threads_in_the_last"])
def test_workgroup_edges(with_16_17):
    res = small_lattice(with_16_17)               # 11264 = 44 x 256 (itemset, position) threads, or 11266
    for kw in (dict(), dict(min_confidence=0.75, sort="leverage"), dict(min_lift=1.0, sort="conviction")):
        want = all_rules(res, **kw)
        same(on_device(res, **kw), want)
    assert 0 < want.n_rules < (11266 if with_16_17 else 11264)


def test_compaction_across_workgroups_and_scan_chunks():
    res, per_wg = cube()
    # chosen on the CPU: 381 workgroups select nothing, 92 all 256, the other 8743 a mix
    assert per_wg.size == 9216 and (per_wg == 0).sum() > 50 and (per_wg == 256).sum() > 50
    assert ((per_wg > 0) & (per_wg < 256)).sum() > per_wg.size // 2
    want = all_rules(res, min_confidence=CUBE_CONF, sort="lift")
    assert want.n_rules == int(per_wg.sum())
    got = on_device(res, min_confidence=CUBE_CONF, sort="lift")
    same(got, want)
    same(on_device(res, min_confidence=CUBE_CONF, sort="lift"), got)           # no atomics in the placement
    # the compacted (level, itemset, position) order itself: two runs place alike
    tie = np.arange(len(res.items))
    kw = dict(min_confidence=CUBE_CONF, sort="support", limit=100000)
    a = prim.rule_measures_device(res.levels, res.counts, res.n_lines, tie, DEV, **kw)
    b = prim.rule_measures_device(res.levels, res.counts, res.n_lines, tie, DEV, **kw)
    assert all(torch.equal(a[f], b[f]) for f in FIELDS)


def test_measures_on_the_device():
    check_large_counts(on_device)
    check_repeated_token(on_device)
    check_thresholds(on_device)


@pytest.mark.parametrize("name", sorted(little_to_do()))
def test_shapes_that_launch_little_or_nothing(name, calls):
    res, n = little_to_do()[name]
    rm = prim.rule_measures_device(res.levels, res.counts, res.n_lines, np.arange(3), DEV)
    assert all(v.device.type == "cuda" for v in rm.values()) and rm["cons"].numel() == n
    same(on_device(res), all_rules(res))
    if n == 0:
        # no level 2, or an empty one: the launcher returns before any launch, nothing is emitted
        assert set(calls) == {"fa_hip_rule_measures"} and rm["ante_off"].tolist() == [0]


def test_missing_subset_raises_through_the_error_word(calls):
    with pytest.raises(RuntimeError, match="size 4 has a subset that is not in level 3"):
        on_device(missing_subset())
    assert calls == ["fa_hip_rule_measures"]                              # read before anything is emitted
    with pytest.raises(RuntimeError, match=r"size \d+ has a subset that is not in level \d+"):
        on_device(quest300()[1])
    res = _mine(D, 0.5)
    check_hand(on_device(res), res)                                        # the next call starts from a zero word


def test_job_on_the_device(tmp_path, calls):
    from fastapriori_amd.config import JobConfig
    from fastapriori_amd.parallel.comm import Comm
    from fastapriori_amd.pipeline import run_job
    (tmp_path / "D.dat").write_text(D)
    (tmp_path / "U.dat").write_text(U)
    job = dict(input=f"{tmp_path}/", min_support=0.5, device="cuda")
    s = run_job(JobConfig(**job, output=f"{tmp_path}/o_", rules=True, min_confidence=0.6), Comm(device=DEV))
    assert s["n_rules_exported"] == 9 and s["n_itemsets"] == 7
    assert (tmp_path / "o_rules" / "part-00000").read_bytes() == HAND_BYTES
    assert calls == ["fa_hip_rule_measures", "fa_hip_rule_measures_emit", "fa_hip_rule_measures_fin"]
    s0 = run_job(JobConfig(**job, output=f"{tmp_path}/p_"), Comm(device=DEV))
    assert "n_rules_exported" not in s0 and not (tmp_path / "p_rules").exists()
    assert (tmp_path / "o_recommends" / "part-00000").read_bytes() == \
        (tmp_path / "p_recommends" / "part-00000").read_bytes()
