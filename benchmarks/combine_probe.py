"""Top-N lists and leave-one-out ranks in the three --combine modes, on the device.

    python benchmarks/combine_probe.py [--config T10I4D100M] [--n 10] [--reps 3] [--warmup 1]

The headline's rules with a 1 M-line generated U.dat.  ``first`` (k_recommend_topn_indexed,
k_holdout_rank_indexed) is the yardstick from the same build; ``sum`` and ``votes`` run
k_recommend_combined / k_holdout_rank_combined, which walk every firing rule of a basket by
design.  Whole calls (LUT, canonical sort, basket de-duplication, the kernel, the fan-out),
host clock around work that ends in a device synchronise; warm runs, the modes alternating;
min / median / max over the repetitions.  One JSON line.
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

MODES = ("first", "sum", "votes")


def _stats(ms: list) -> dict:
    return {"median_ms": round(statistics.median(ms), 3), "min_ms": round(min(ms), 3), "max_ms": round(max(ms), 3),
            "reps": len(ms)}


def main():
    import torch
    import bench
    from fastapriori_amd.models.apriori import FastApriori, MinerConfig
    from fastapriori_amd.models.rules import AssociationRules
    from fastapriori_amd.ops import primitives as prim
    from fastapriori_amd.parallel.comm import Comm
    from fastapriori_amd.utils.io import generate_shard
    from fastapriori_amd.utils.metrics import Logger

    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default=bench.HEADLINE)
    ap.add_argument("--n", type=int, default=10)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("combine_probe needs a GPU: its figures are device times")
    dev = torch.device("cuda", 0)
    comm, quiet = Comm(device=dev), Logger(enabled=False)
    rows, L, I, P, N, ms = bench.CONFIGS[a.config]
    sh = generate_shard(rows, comm, dev, L, I, P, N, seed=1)
    res = FastApriori(ms, config=MinerConfig(min_support=ms), logger=quiet).run(sh)
    del sh
    users = generate_shard(bench.U_LINES, comm, dev, L, I, P, N, seed=2, users=True)
    ar = AssociationRules(res, device=dev, logger=quiet)

    def timed(fn):
        torch.cuda.synchronize()
        t = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t) * 1e3, out

    def topn(mode):
        if mode == "first":
            return ar.recommend_topn_shard(users, a.n)
        return ar.recommend_combined_shard(users, a.n, mode)[0]

    paths = {f"topn_{m}": (lambda m=m: topn(m)) for m in MODES}
    paths.update({f"holdout_{m}": (lambda m=m: ar.holdout_ranks_shard(users, a.n, combine=m)[1]) for m in MODES})
    prim.reset_fallbacks()
    for _ in range(max(a.warmup, 1)):
        outs = {k: timed(f)[1] for k, f in paths.items()}
    times = {k: [] for k in paths}
    for _ in range(a.reps):
        for k, f in paths.items():                              # alternating
            times[k].append(timed(f)[0])
    if prim.FALLBACKS:
        raise SystemExit(f"combine_probe: host fallbacks {prim.FALLBACKS}")
    out = {"config": a.config, "n": a.n, "n_rules": ar.rules().n_rules, "n_items": len(res.items),
           "lines": users.n_lines, "distinct_baskets": int(ar.stats["distinct_baskets"])}
    for k in paths:
        out[k] = _stats(times[k])
        if k.startswith("topn"):
            out[k]["entries"] = int((outs[k] >= 0).sum())
        else:
            out[k]["hits"] = int((outs[k] > 0).sum())
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
