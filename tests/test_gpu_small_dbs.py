"""The device miner against the brute-force oracle on the corpus of tests/small_dbs.py.

One test per configuration of FastApriori._mine_device_loop (``CONFIGS``), the entries looped
inside.  The reference is always models.oracle.mine on the same text (test_small_dbs.oracle,
computed once per entry), never a device result and never the CPU miner.  The comparison is
test_small_dbs.compare: exact, and it names the entry, the configuration and the first itemset
that differs with both counts.  Every run is made twice on one FastApriori object (workspace,
control block and F sizes are reused) and must repeat itself.

Coverage is a condition: each configuration ends by asserting, from ``stats`` and
``log.records``, that the path it is there for was taken -- on every entry with a level 3 where
the path is a property of the run, on at least one entry where it depends on the entry.  A
configuration that never reaches its path on this corpus fails; no entry is skipped.

Every entry runs under ``default``, ``dedup_on``, ``dedup_off`` and ``gates_open_acc8_1``; every
configuration runs the core subset (small_dbs.CORE).
"""
import functools

import numpy as np
import pytest
import torch

from fastapriori_amd.models.apriori import FastApriori, MinerConfig
from fastapriori_amd.ops import primitives as prim
from fastapriori_amd.ops.host import apriori_gen
from fastapriori_amd.tuning import TUNING
from fastapriori_amd.utils.io import parse_bytes
from fastapriori_amd.utils.metrics import Logger
from small_dbs import BY_NAME, CORE, ENTRIES
from test_small_dbs import compare, oracle

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
ALL = [e.name for e in ENTRIES]
CFG_FIELDS = set(MinerConfig.__dataclass_fields__)

GATES = dict(dl_acc8_min_rows=0, dl_regroup_min_rows=0, lane_deal_min_rows=0, window_trim_min_rows=0,
             trim_min_rows=0)
# id -> (knobs: MinerConfig fields and TUNING knobs together, entries, per-entry LDS budget)
CONFIGS = {
    "default": (dict(), ALL, None),
    "dedup_on": (dict(dedup="on"), ALL, None),
    "dedup_off": (dict(dedup="off"), ALL, None),
    "gram": (dict(pair_strategy="gram"), CORE, None),
    "horizontal": (dict(pair_strategy="horizontal"), CORE, None),
    "gates_open_acc8_1": (dict(GATES, dl_acc8_bundles=1, dedup="off"), ALL, None),
    "gates_open_acc8_2": (dict(GATES, dl_acc8_bundles=2, dedup="off"), CORE, "width16_minus_one"),
    "acc16_bundles": (dict(dl_acc16_bundles=True, dl_acc8_bundles=0, dedup="off"), CORE, None),
    "tail_on": (dict(dl_tail_bundle=True, dl_acc8_min_rows=0, dedup="off"), CORE, "tail_pad"),
    "tail_off": (dict(dl_tail_bundle=False, dl_acc8_min_rows=0, dedup="off"), CORE, "tail_pad"),
    "max_level_3": (dict(max_level=3), CORE, None),
    "max_level_4": (dict(max_level=4), CORE, None),
    "max_level_5": (dict(max_level=5), CORE, None),
    "no_regroup": (dict(dl_regroup=False, dl_regroup_min_rows=0), CORE, None),
    "regroup": (dict(dl_regroup=True, dl_regroup_min_rows=0), CORE, None),
    "one_level_bundles": (dict(bundle_levels=False), CORE, None),
    "growth_1": (dict(bundle_growth=1.0), CORE, None),
    "growth_100": (dict(bundle_growth=100.0), CORE, None),
    "no_post": (dict(dl_post=False), CORE, None),
    "multipass_acc16_winitems": (dict(dl_acc16=True, mp_window_items=True, dedup="off"), CORE, "multipass"),
    "multipass_acc16": (dict(dl_acc16=True, mp_window_items=False, dedup="off"), CORE, "multipass"),
    "multipass_u32_winitems": (dict(dl_acc16=False, mp_window_items=True, dedup="off"), CORE, "multipass"),
    "multipass_u32": (dict(dl_acc16=False, mp_window_items=False, dedup="off"), CORE, "multipass"),
    "multipass_weighted": (dict(dedup="on"), CORE, "multipass"),
    "multipass_window_trim": (dict(window_trim_min_rows=0, window_trim_cost=0.0, trim_min_rows=0, dedup="off"),
                              CORE, "multipass"),
    "multi_to_host": (dict(dl_multi=False, dedup="off"), CORE, "multipass"),
    "host_loop_devgen_chain": (dict(device_levels=False, gen_device_min_rows=0, gen_chain=True), CORE, None),
    "host_loop_devgen": (dict(device_levels=False, gen_device_min_rows=0, gen_chain=False), CORE, None),
    "bitmap_kernel": (dict(level_kernel="bitmap"), CORE, None),
    "trim_forced": (dict(trim_min_rows=0, trim_rows_frac=2.0, trim_nnz_frac=2.0), CORE, None),
}
FALLBACKS_ALLOWED = ("multi_to_host", "host_loop_devgen_chain", "host_loop_devgen", "bitmap_kernel")


@functools.lru_cache(maxsize=None)
def _shard(name: str):
    return parse_bytes(BY_NAME[name].text, device=DEV)


@functools.lru_cache(maxsize=None)
def _level3(name: str):
    """(F1, items that level 3's candidates use, level 3's candidates) from the oracle's F_2."""
    exp = oracle(name)[0]
    f2 = np.array(sorted(sorted(s) for s in exp.itemsets if len(s) == 2), dtype=np.int32).reshape(-1, 2)
    if len(f2) < 3:
        return len(exp.items), 0, 0
    pi, _, ex = apriori_gen(f2)
    return len(exp.items), int(np.union1d(f2[pi].ravel(), ex).size) if ex.size else 0, int(ex.size)


def _lds_budget(name: str, rule: str, accb: int):
    """TUNING.slab_lds_bytes for entry ``name``, chosen on the host with the slab rule alone
    (prim.slab_width), or None for the default budget.

    multipass: the smallest budget at which the rule still returns a width for level 3's U
    used items and C3 candidates.  With more than 1024 candidates that is width 4 with a
    capacity of 1024 < C3, so level 3 itself is counted window by window; with fewer the
    level fits and only later, wider levels do.  -> (budget, whether level 3 must be multi-pass)
    width16_minus_one: width 16 holds one u32 accumulator too few for level 3, so the rule
    leaves width 16 and byte accumulators bring the bundle back to it.  -> (budget, whether
    that is so)
    tail_pad: for an entry that states its last bundle (expectations["tail_bundle"]: used items
    and candidates), the smallest budget at which the packed pass of the tail rule holds it:
    only the thinnest row padding fits, so the bundle's pad shift is > 0.  -> (budget, True)"""
    F1, U, C3 = _level3(name)
    if rule == "tail_pad":
        t = BY_NAME[name].expectations.get("tail_bundle")
        if t is None:
            return None, False
        fits = lambda b: prim.slab_pack_width(t["used"], t["candidates"], b, 1)       # noqa: E731
        b = next(b for b in range(0, _default_lds(), 32) if fits(b)[0] == 16 and fits(b)[1] >= t["candidates"])
        assert fits(b)[2] > 0 and prim.slab_width(t["used"], t["candidates"], b, 4)[1] < t["candidates"]
        return b + prim.slab_map_lds(F1), True
    if C3 == 0:
        return None, False
    if rule == "width16_minus_one":
        b = U * 144 + 4 * (min(C3, 8192) - 1)
        ok = (C3 >= 2 and prim.slab_width(U, C3, b, 4)[0] in (8, 4) and prim.slab_width(U, C3, b, 1)[0] == 16
              and prim.slab_width(U, C3, b, 1)[1] >= C3)
    else:
        b = next((b for b in range(0, 1 << 18, 16) if prim.slab_width(U, C3, b, accb)[0]), None)
        ok = b is not None and prim.slab_width(U, C3, b, accb)[1] < C3
    if b is None or b + prim.slab_map_lds(F1) >= _default_lds():
        return None, False
    return b + prim.slab_map_lds(F1), ok


def _default_lds() -> int:
    from fastapriori_amd.tuning import Tuning
    return Tuning().slab_lds_bytes


DEDUP_CALLS = []


@pytest.fixture(autouse=True)
def _note_dedup(monkeypatch):
    """DEDUP_CALLS grows whenever a run merges its rows into weight classes."""
    real = FastApriori._dedup
    monkeypatch.setattr(FastApriori, "_dedup", lambda self, db: (DEDUP_CALLS.append(1), real(self, db))[1])


class Run:
    """What one entry's run under one configuration left behind."""

    def __init__(self, name, m, res, forced, weighted):
        self.name, self.stats, self.records, self.res, self.forced = name, dict(m.stats), list(m.log.records), res, forced
        self.T0 = int(m.stats.get("T", 0))                            # rows kept by the compression
        self.weighted = weighted if len(res.items) >= 2 else None     # FastApriori._dedup laid the rows out
        self.has3 = any(len(s) >= 3 for s in oracle(name)[1])
        # ... and every level of it counted in one pass of the slab kernel
        self.onepass = self.has3 and not ({"device_multipass", "device_bitmap_levels", "host_levels"} & set(m.stats))
        self.shapes = self.stats.get("device_bundle_shapes", [])      # (k0, levels, C, used, sw, accumulator bytes)


def _mine(name: str, cid: str, tune) -> Run:
    knobs, _, rule = CONFIGS[cid]
    e = BY_NAME[name]
    cfg = {k: v for k, v in knobs.items() if k in CFG_FIELDS}
    tune(**{k: v for k, v in knobs.items() if k not in CFG_FIELDS})
    forced = False
    if rule is not None:
        unit = cfg.get("dedup") == "off"
        budget, forced = _lds_budget(name, rule, 2 if rule == "multipass" and unit and TUNING.dl_acc16 else 4)
        tune(slab_lds_bytes=_default_lds() if budget is None else budget)
    m = FastApriori(e.min_support, config=MinerConfig(min_support=e.min_support, **cfg), logger=Logger(0, enabled=False))
    DEDUP_CALLS.clear()
    first = m.run(_shard(name))
    compare(first, name, cid, max_level=cfg.get("max_level", 0))
    st1 = dict(m.stats)
    run = Run(name, m, first, forced, bool(DEDUP_CALLS))
    m.log.records.clear()
    again = m.run(_shard(name))
    compare(again, name, cid + ", second run", max_level=cfg.get("max_level", 0))
    assert len(first.levels) == len(again.levels), (name, cid)
    for a, b, ca, cb in zip(first.levels, again.levels, first.counts, again.counts):
        assert np.array_equal(a, b) and np.array_equal(ca, cb), (name, cid, "the second run differs")
    for key in ("device_bundle_shapes", "device_bundle_pads", "device_multipass", "host_levels", "pair_strategy"):
        assert st1.get(key) == m.stats.get(key), (name, cid, key, st1.get(key), m.stats.get(key))
    if cid in FALLBACKS_ALLOWED:
        pass
    else:
        assert "fallbacks" not in run.stats, (name, cid, run.stats["fallbacks"])
    return run


@functools.lru_cache(maxsize=None)
def _default_shapes(name: str):
    e = BY_NAME[name]
    m = FastApriori(e.min_support, config=MinerConfig(min_support=e.min_support), logger=Logger(0, enabled=False))
    m.run(_shard(name))
    return tuple(m.stats.get("device_bundle_shapes", ()))


def _some(runs, pred, what):
    hit = [r.name for r in runs if pred(r)]
    assert hit, f"no entry reached: {what}"
    return hit


def _every(runs, pred, what, only=lambda r: r.has3):
    miss = [(r.name, r.shapes) for r in runs if only(r) and not pred(r)]
    assert not miss, f"{what}: not on {miss}"
    assert any(only(r) for r in runs), what


@pytest.mark.parametrize("cid", list(CONFIGS))
def test_config_equals_oracle(tune, cid, monkeypatch):
    knobs, names, rule = CONFIGS[cid]
    calls = {"dl_plan": 0}
    if cid == "no_post":
        real = prim.dl_plan
        monkeypatch.setattr(prim, "dl_plan", lambda *a, **k: (calls.__setitem__("dl_plan", calls["dl_plan"] + 1),
                                                              real(*a, **k))[1])
    if cid in ("growth_1", "growth_100"):
        base = {n: _default_shapes(n) for n in names}            # before any knob is set
    rg0 = prim.dl_regroup_last()[0]
    runs = [_mine(n, cid, tune) for n in names]
    rg1 = prim.dl_regroup_last()[0]
    print(cid, {r.name: (r.shapes, r.stats.get("device_bundle_pads"), r.stats.get("device_multipass"),
                         r.stats.get("host_levels"), r.stats.get("window_trims")) for r in runs if r.has3})

    on_device = cid not in ("host_loop_devgen_chain", "host_loop_devgen", "bitmap_kernel")
    if on_device and cid != "multi_to_host":
        _every(runs, lambda r: r.stats.get("device_bundles", 0) >= 1, "a device bundle")
    if cid == "dedup_on" or cid == "multipass_weighted":
        # (fewer than two kept rows are never merged: FastApriori._want_dedup)
        _every(runs, lambda r: r.weighted is True, "the weighted layout", only=lambda r: r.T0 >= 2)
    if knobs.get("dedup") == "off":
        _every(runs, lambda r: r.weighted is False, "the unit layout", only=lambda r: r.weighted is not None)
    if cid in ("gram", "horizontal"):
        _every(runs, lambda r: r.stats.get("pair_strategy") == cid, "the pair strategy",
               only=lambda r: len(r.res.items) >= 2)
    if cid == "gates_open_acc8_1":
        _every(runs, lambda r: r.shapes and all(s[5] == 1 for s in r.shapes), "every bundle in bytes",
               only=lambda r: r.onepass)
        assert rg1 > rg0, "no bundle was regrouped"
    if cid == "gates_open_acc8_2":
        _every(runs, lambda r: r.shapes[0][4] == 16 and r.shapes[0][5] == 1, "level 3 in bytes at width 16",
               only=lambda r: r.forced)
        assert rg1 > rg0, "no bundle was regrouped"
    if cid == "acc16_bundles":
        _every(runs, lambda r: r.shapes and all(s[5] == 2 for s in r.shapes), "every bundle in u16",
               only=lambda r: r.onepass)
    if cid == "tail_on":
        _every(runs, lambda r: any(p > 0 for p in r.stats.get("device_bundle_pads", ())), "a packed tail bundle",
               only=lambda r: r.forced)
    if cid == "tail_off":
        _every(runs, lambda r: not any(r.stats.get("device_bundle_pads", ())), "no packed bundle")
    if cid.startswith("max_level"):
        m = knobs["max_level"]
        assert all(len(r.res.levels) <= m for r in runs)
        _every(runs, lambda r: r.stats.get("device_bundles", 0) >= 1 and all(s[0] + s[1] - 1 <= m for s in r.shapes),
               "bundles end at the limit")
        _some(runs, lambda r: max((len(s) for s in oracle(r.name)[1]), default=0) > m, "an entry deeper than the limit")
    if cid == "no_regroup":
        assert rg1 == rg0, "a bundle was regrouped with the knob off"
    if cid == "regroup":
        assert rg1 > rg0, "no bundle was regrouped"
    if cid == "one_level_bundles":
        _every(runs, lambda r: r.shapes and all(s[1] == 1 for s in r.shapes), "one level per bundle")
    if cid in ("growth_1", "growth_100"):
        _some(runs, lambda r: [s[:2] for s in r.shapes] != [s[:2] for s in base[r.name]],
              "bundles cut differently from the default's")
    if cid == "no_post":
        assert calls["dl_plan"] >= 2 * sum(r.onepass for r in runs) > 0, "the plan was not driven from Python"
    if cid.startswith("multipass"):
        _every(runs, lambda r: r.stats.get("device_multipass", 0) >= 1, "a window-by-window level",
               only=lambda r: r.forced)
        assert all(r.stats.get("host_levels", 0) == 0 for r in runs)
    if cid == "multipass_window_trim":
        _some(runs, lambda r: r.stats.get("window_trims", 0) >= 1, "a trimmed window")
    if cid == "multi_to_host":
        _every(runs, lambda r: r.stats.get("host_levels", 0) >= 1 and "device_multipass" not in r.stats,
               "the host loop took over", only=lambda r: r.forced)
    if cid.startswith("host_loop_devgen"):
        assert all("device_bundles" not in r.stats for r in runs)
        _every(runs, lambda r: r.stats.get("host_levels", 0) >= 1, "the host loop")
    if cid == "bitmap_kernel":
        assert all("device_bundles" not in r.stats for r in runs)
    if cid == "trim_forced":
        _every(runs, lambda r: any(rec.get("phase") == "trim" for rec in r.records), "a trim",
               only=lambda r: "trim_loses" in BY_NAME[r.name].expectations)
