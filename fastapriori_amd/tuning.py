"""Internal tuning knobs: one dataclass, read at call time.

Product settings (what a user of the reference changes: support, device, strategy,
outputs) live in ``config.JobConfig`` (CLI > FA_* env > defaults) and
``models.apriori.MinerConfig``.  Everything here is a lab setting: the defaults are the
measured choices (docs/PERF.md, docs/PERF_HISTORY.md), code reads them through the
module-level ``TUNING`` instance when it runs (not at import), and tests change them
with ``override(...)``.  A/B experiments set ``FA_TUNE="name=value,name=value"`` --
the one environment variable this module reads -- e.g.
``FA_TUNE=bundle_growth=2.0,device_levels=0 python bench.py``.

The full table of knobs with their defaults is in docs/ARCHITECTURE.md
("Configuration").
"""
from __future__ import annotations

import os
from contextlib import contextmanager
from dataclasses import dataclass, fields


@dataclass
class Tuning:
    # ---- level loop (models/apriori.py) -------------------------------------------
    bundle_levels: bool = True          # count speculative later levels in level k's launch
    bundle_growth: float = 1.5          # a bundled level may have <= this x the previous level's candidates
    bundle_max_prefix: int = 9          # no bundling past prefixes of this many items
    device_levels: bool = True          # level bundles generated / counted / thresholded on the GPU
    dl_post: bool = True                # the bundle's plan + count queued by the generator's native call
    dl_multi: bool = True               # multi-pass levels stay on the device (window by window)
    gen_device: bool = True             # apriori-gen on the GPU for big levels (host loop)
    gen_chain: bool = True              # speculative levels in one native call (host loop)
    gen_device_min_rows: int = 512      # smaller F_{k-1}: the C++ host generator
    # k = 2 across ranks: triangles of at least this many pairs are reduce-scattered and
    # thresholded per slice (Comm.reduce_scatter_select) instead of all-reduced; below it
    # the triangle is all-reduced and F_2 compacted on the device with no host round trip.
    # For the T10I4 triangle (474K pairs, 1.9 MB) one ring all-reduce over xGMI costs less
    # than the reduce-scatter's three collectives and two host syncs; 4M pairs (F1 ~ 2900,
    # 16 MB) is where the all-reduce's 2(W-1)/W volume starts to dominate.
    pair_rs_min: int = 1 << 22
    # ---- compression (ops/primitives.py) ------------------------------------------
    fused_compress: bool = True         # two-pass fused compression for short rows
    early_compress: bool = True         # compression queued before the F1 bookkeeping (host overlap)
    f1_rank_device: bool = True         # narrow numeric vocabularies ranked on the device (no F1 host round trip)
    fused_compress_mean_len: float = 12.0
    fused_layout: bool = True           # the emit pass writes the pair kernel's blocked layout
    compress_wave_mean_len: float = 48.0
    # ---- counting kernels (ops/primitives.py) -------------------------------------
    slab_lds_bytes: int = 160 * 1024 - 512   # LDS of the slab kernel (minus its static scratch)
    slab_cls: int = 1                   # class layout of host-planned slab passes: 0 off, 1 model, 2 always
    dense_min_rows: float = 4.0         # skip the all-zero-prefix test above this many rows per slab
    dl_acc16: bool = True               # packed u16 accumulators in window-by-window levels (unit weights)
    dl_acc16_bundles: bool = False      # ... and in one-pass device bundles
    # single-writer byte accumulators in one-pass device bundles (unit weights; before
    # dl_acc16_bundles): four candidates per accumulator word, so a bundle of ~1000 used
    # items and ~20K candidates counts on 16-word slabs instead of 8-word ones.  0: off;
    # 1: every bundle is accepted by the slab rule at one byte per candidate and counted in
    # bytes (the bundling shifts: T10I4D100M 3-5 | 6-12 plus a trim, 40.9 ms against 39.8);
    # 2: bundled as without the knob, counted in bytes where that moves the bundle's slab
    # up to width 16 (T10I4D100M levels 3-4: 11.9 -> 9.5 ms, the run 39.95 -> 38.06 ms)
    dl_acc8_bundles: int = 2
    # ... from this many rows to count: measured to gain on the 12.5M-row shard (6.21 ->
    # 6.03 ms) and above, no measurable difference at 100K rows (1.08-1.19 ms either way),
    # where the bundles stay on the accumulators the rule gave them
    dl_acc8_min_rows: int = 1 << 20
    # the tail rule (csrc/host/fa_slab.h, gen.hip dl_tail): a device bundle that holds every
    # remaining level of the run -- the chain ran out of candidates, or --max-level ends the
    # mining inside it -- is counted in ONE pass of 16-word slabs whose rows are padded one
    # in 2, 4 or 8 instead of each (the pad shift; the smallest that leaves the accumulators
    # room), where the slab rule would split it and build every slab twice.  Unit weights, the
    # rank map in LDS, bundles planned by the post step (dl_post), and at least
    # dl_acc8_min_rows lines per counting rank (the database's lines / ranks, or all of them
    # when every rank counts the whole database): the rule decides which levels share a
    # bundle and its all-reduce, so it never looks at a rank's own shard.  Every other bundle
    # is cut exactly as without the knob.
    dl_tail_bundle: bool = True
    # one-pass device bundles the post step plans and counts: every candidate grouped under
    # its best parent -- any (k-1)-subset that is a parent row -- instead of its lexicographic
    # prefix (csrc/host/fa_regroup.h, csrc/hip/regroup.hip), the counts put back in the
    # generator's order before the all-reduce.  Off: the prefix plan, byte for byte.  It
    # decides the piece records, so every rank sets the same value.
    dl_regroup: bool = True
    # ... from this many lines per counting rank (the database's lines / ranks, as the tail
    # rule's: the same on every rank).  The step's cost is fixed per bundle -- one workgroup
    # per level, 0.87 ms on T10I4's levels 3-12 -- while the slab time it saves grows with
    # the rows counted (1.78 ms per 100 M rows there): T10I4D100M 36.65 -> 35.81 ms, but
    # the 12.5M-row shard 5.80 -> 6.32 ms and T10I4D100K 1.09 -> 1.20 ms without the
    # threshold, which sits above the ~50 M rows where the two meet
    dl_regroup_min_rows: int = 1 << 26
    mp_window_items: bool = True        # window-by-window levels: each window's slab holds only its own used items
    # window-by-window levels: a window counts only the rows holding >= k of its own items
    # (its items' bitmap compacted to them, count.hip k_win_compact) when the binomial
    # estimate keeps fewer than window_trim_est_frac of the level's rows and the count
    # (a sample, then exact) fewer than min(window_trim_rows_frac,
    # 1 - window_trim_cost * items / (candidates * (k + 1))) (FastApriori._window_rows)
    window_trim: bool = True
    window_trim_est_frac: float = 0.95
    window_trim_rows_frac: float = 0.97
    window_trim_cost: float = 100.0
    # ... when the rank's shard had at least this many rows after compression (T40I10D10M,
    # 10M rows: windows of a tenth of the work, where the compaction's fixed costs ate the
    # gain: 70.6 -> 73.6 ms; the shard's size, not the level's: T40I10D100M's level 11
    # keeps ~20M rows and still gains, 21.8 -> 16.5 ms)
    window_trim_min_rows: int = 1 << 25
    # bank-aware lane deal of device slab plans (levels.hip k_dl_lane_assign) from this many
    # rows (-1: off): ~0.18 ms per bundle against ~5 % of the slab counts (T10I4D100M
    # 42.1 -> 41.2 ms; the 12.5M-row shard 6.50 -> 6.85 ms, hence the threshold)
    lane_deal_min_rows: int = 1 << 25
    pair_wg: int = 0                    # k_pair_queue16 workgroups (0: one per CU)
    gram_mfma_min_class_words: int = 512   # shorter weight classes: the popcount Gram
    bitmap_blocked: bool = True         # the Gram's bitmap in 8-word blocks (count.hip BmView)
    # transaction trimming before a level (models/apriori.py _trim_worth_it, gen.hip dl_post):
    # when the binomial estimate keeps fewer than this share of the rows, or of the items
    trim_rows_frac: float = 0.75
    trim_nnz_frac: float = 0.6
    # ---- the query counter (ops/primitives.py query_plan / query_count) -------------
    query_lds_bytes: int = 160 * 1024 - 512   # LDS of a window: slab, accumulators, tile offsets (fa_query.h)
    query_acc: int = 0                  # queries per window (0: fa_query.h kQAcc; smaller makes more windows)
    query_max_wg: int = 0               # workgroups of the one launch (0: the launcher's rule)
    # ---- I/O (utils/io.py) -------------------------------------------------------
    gpu_parse: bool = True              # D.dat parsed on the GPU behind the H2D copies
    gpu_parse_dict: bool = True         # dictionary-mode tokens too
    stream_parse: bool = True           # parse each chunk as it lands
    ring_slots: int = 16                # pinned read-ring slots (pread threads)
    # ---- collectives (parallel/comm.py) --------------------------------------------
    bucket_mb: float = 64.0             # largest single all-reduce; longer vectors go in buckets

    @classmethod
    def from_env(cls, spec: str | None = None) -> "Tuning":
        t = cls()
        t.apply(os.environ.get("FA_TUNE", "") if spec is None else spec)
        return t

    def apply(self, spec: str) -> None:
        """'name=value,name=value' (bools as 0/1/true/false)."""
        types = {f.name: f.type for f in fields(self)}
        for part in filter(None, (p.strip() for p in spec.split(","))):
            name, _, val = part.partition("=")
            name = name.strip()
            if name not in types:
                raise ValueError(f"FA_TUNE: unknown knob {name!r} (known: {', '.join(sorted(types))})")
            cur = getattr(self, name)
            if isinstance(cur, bool):
                v = val.strip().lower() in ("1", "true", "yes", "on")
            else:
                v = type(cur)(float(val) if isinstance(cur, int) else val)
            setattr(self, name, v)


TUNING = Tuning.from_env()


@contextmanager
def override(**kw):
    """Temporarily change knobs of TUNING (tests, experiments)."""
    old = {k: getattr(TUNING, k) for k in kw}
    for k in kw:
        if not hasattr(TUNING, k):
            raise AttributeError(f"unknown tuning knob {k}")
    try:
        for k, v in kw.items():
            setattr(TUNING, k, v)
        yield TUNING
    finally:
        for k, v in old.items():
            setattr(TUNING, k, v)


__all__ = ["Tuning", "TUNING", "override"]
