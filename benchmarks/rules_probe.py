"""Rule building on the host (C++) vs the device (HIP) for a mined result, then the
recommendation kernels on its rule table (--top-n N: the ranked top-N kernels, too).

    python benchmarks/rules_probe.py [--config T10I4D10M] [--top-n 10] [--export]

--export: also the rule export (AssociationRules.all_rules: every rule, no cut, five measures)
on the host and on the device at min_confidence 0 and 0.5, with the rule counts and a signature.
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    import numpy as np
    import torch
    import bench
    from fastapriori_amd.models.apriori import FastApriori, MinerConfig
    from fastapriori_amd.models.rules import AssociationRules
    from fastapriori_amd.parallel.comm import Comm
    from fastapriori_amd.utils.io import generate_shard
    from fastapriori_amd.utils.metrics import Logger

    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="T10I4D10M")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--top-n", type=int, default=0, help="also time recommend_topn_shard for N = 1 and this N")
    ap.add_argument("--export", action="store_true", help="also time all_rules() on host and device")
    a = ap.parse_args()
    n, L, I, P, N, ms = bench.CONFIGS[a.config]
    dev = torch.device("cuda", 0)
    sh = generate_shard(n, Comm(device=dev), dev, L, I, P, N, 1)
    res = FastApriori(ms, config=MinerConfig(min_support=ms), logger=Logger(enabled=False)).run(sh)
    del sh
    out = {"config": a.config, "n_itemsets": res.n_itemsets}
    for name, d in (("host", None), ("device", dev)):
        best = 1e9
        for _ in range(a.reps):
            torch.cuda.synchronize()
            t = time.perf_counter()
            rt = AssociationRules(res, logger=Logger(enabled=False), device=d).rules()
            torch.cuda.synchronize()
            best = min(best, time.perf_counter() - t)
        out[name + "_ms"] = round(best * 1e3, 2)
        out[name + "_rules"] = rt.n_rules
        out[name + "_sig"] = int(np.asarray(rt.cons, dtype=np.int64).sum() + rt.ante.astype(np.int64).sum())
    if a.export:
        # the one-pass export next to the cut builder above (device_ms): the same subset searches
        # without the per-level launches and readbacks; wall time around the call, device drained
        for mc in (0.0, 0.5):
            for name, d in (("host", None), ("device", dev)):
                ar = AssociationRules(res, logger=Logger(enabled=False), device=d)
                best = 1e9
                for rep in range(a.reps + 1):
                    torch.cuda.synchronize()
                    t = time.perf_counter()
                    rm = ar.all_rules(min_confidence=mc)
                    torch.cuda.synchronize()
                    if rep:                                 # the first call is the warm-up
                        best = min(best, time.perf_counter() - t)
                key = f"export_{name}_c{mc:g}"
                out[key + "_ms"] = round(best * 1e3, 2)
                out[key + "_rules"] = rm.n_rules
                out[key + "_sig"] = int(rm.cons.astype(np.int64).sum() + rm.ante.astype(np.int64).sum()
                                        + rm.cnt_s.sum() + rm.lift.view(np.int64).sum() % (1 << 40))
        # the same two builders with the results left on the device: what the calls above
        # spend outside the copy of their result arrays to numpy
        from fastapriori_amd.ops import primitives as prim
        tie = AssociationRules(res, logger=Logger(enabled=False))._tie_pos()
        for key, fn in (("export_device_c0_resident_ms",
                         lambda: prim.rule_measures_device(res.levels, res.counts, res.n_lines, tie, dev)),
                        ("device_resident_ms", lambda: prim.rules_build_device(res.levels, res.counts, tie, dev))):
            best = 1e9
            for rep in range(a.reps + 1):
                torch.cuda.synchronize()
                t = time.perf_counter()
                r = fn()
                torch.cuda.synchronize()
                if rep:
                    best = min(best, time.perf_counter() - t)
            out[key] = round(best * 1e3, 2)
            out[key.replace("_ms", "_mbytes")] = round(sum(v.numel() * v.element_size() for v in r.values()
                                                           if isinstance(v, torch.Tensor)) / 1e6, 1)
            del r
    users = generate_shard(max(n // 100, 1000), Comm(device=dev), dev, L, I, P, N, 1, users=True)
    ar = AssociationRules(res, logger=Logger(enabled=False), device=dev)
    ar.rules()
    recs = {}
    for name, idx in (("recommend_indexed", True), ("recommend_scan", False)):
        ar.use_index = idx
        best = 1e9
        for _ in range(a.reps):
            torch.cuda.synchronize()
            t = time.perf_counter()
            r = ar.recommend_shard(users)
            torch.cuda.synchronize()
            best = min(best, time.perf_counter() - t)
        out[name + "_ms"] = round(best * 1e3, 2)
        recs[name] = r.cpu()
    out["users"] = users.n_lines
    out["recommend_agree"] = bool(torch.equal(recs["recommend_indexed"], recs["recommend_scan"]))
    out["users_with_rec"] = int((recs["recommend_indexed"] >= 0).sum())
    out["distinct_baskets"] = ar.stats.get("distinct_baskets")
    if a.top_n:
        # ranked lists on the same rule table and users: N = 1 (the first-match walk with a
        # one-entry buffer) and N = --top-n, both kernels
        cons = torch.from_numpy(np.asarray(ar.rules().cons))
        tops = {}
        for N in dict.fromkeys((1, a.top_n)):
            for name, idx in (("indexed", True), ("scan", False)):
                ar.use_index = idx
                best = 1e9
                for _ in range(a.reps):
                    torch.cuda.synchronize()
                    t = time.perf_counter()
                    r = ar.recommend_topn_shard(users, N)
                    torch.cuda.synchronize()
                    best = min(best, time.perf_counter() - t)
                out[f"topn{N}_{name}_ms"] = round(best * 1e3, 2)
                tops[N, name] = r.cpu()
            out[f"topn{N}_agree"] = bool(torch.equal(tops[N, "indexed"], tops[N, "scan"]))
            out[f"topn{N}_entries"] = int((tops[N, "indexed"] >= 0).sum())
        col0 = tops[1, "indexed"][:, 0].to(torch.int64)
        first = torch.where(col0 >= 0, cons[col0.clamp(min=0)], torch.full_like(cons[:1], -1))
        out["topn1_is_first_match"] = bool(torch.equal(first, recs["recommend_indexed"]))
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
