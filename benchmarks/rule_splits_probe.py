"""The rule export with multi-item consequents (all_rules(max_consequent = M)) on the device
(HIP) and on the C++ path for a mined Quest result, at M = 1, 2 and every split.

    python benchmarks/rule_splits_probe.py [--config T10I4D10M] [--min-confidence 0.0]

Per M: the (itemset, split) elements, the rules kept, device ms with the results left on the
device (ops.primitives.rule_splits_device, one warm-up call, best of --reps, host clock around
the call ending in a device synchronise), device ms end to end through AssociationRules (with
the copy of the twelve result arrays to numpy), C++ ms (ops.host.rule_splits) and whether
the two paths agree bit for bit.  M = 1 also times today's export for comparison.
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
    from fastapriori_amd.ops import host
    from fastapriori_amd.ops import primitives as prim
    from fastapriori_amd.parallel.comm import Comm
    from fastapriori_amd.utils.io import generate_shard
    from fastapriori_amd.utils.metrics import Logger

    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="T10I4D10M")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--min-confidence", type=float, default=0.0)
    a = ap.parse_args()
    n, L, I, P, N, ms = bench.CONFIGS[a.config]
    dev = torch.device("cuda", 0)
    sh = generate_shard(n, Comm(device=dev), dev, L, I, P, N, 1)
    res = FastApriori(ms, config=MinerConfig(min_support=ms), logger=Logger(enabled=False)).run(sh)
    del sh
    K = len([c for c in res.counts if len(c)])
    tie = AssociationRules(res, logger=Logger(enabled=False))._tie_pos()
    args = (res.levels, res.counts, res.n_lines, tie)
    kw = dict(min_confidence=a.min_confidence)
    out = {"config": a.config, "n_itemsets": res.n_itemsets, "levels": K, "min_confidence": a.min_confidence}

    def best_ms(fn):
        best, r = 1e9, None
        for rep in range(a.reps + 1):
            del r
            torch.cuda.synchronize()
            t = time.perf_counter()
            r = fn()
            torch.cuda.synchronize()
            if rep:                                     # the first call is the warm-up
                best = min(best, time.perf_counter() - t)
        return round(best * 1e3, 2), r

    ar = AssociationRules(res, logger=Logger(enabled=False), device=dev)
    out["today_device_resident_ms"], _ = best_ms(lambda: prim.rule_measures_device(*args, dev, **kw))
    out["today_cpp_ms"], _ = best_ms(lambda: host.rule_measures(*args, **kw))
    for name, M in (("m1", 1), ("m2", 2), ("all", max(K - 1, 1))):
        plan = host.rule_splits_plan(*args[:3], a.min_confidence, None, "confidence", None, M)
        out[name + "_elements"] = int(plan["eoff"][-1])
        out[name + "_device_resident_ms"], d = best_ms(lambda: prim.rule_splits_device(*args, dev, max_consequent=M, **kw))
        out[name + "_rules"] = int(d["cnt_s"].numel())
        out[name + "_result_mbytes"] = round(sum(v.numel() * v.element_size() for v in d.values()) / 1e6, 1)
        if M >= 2:
            out[name + "_device_end_to_end_ms"], _ = best_ms(lambda: ar.all_rules(max_consequent=M, **kw))
        out[name + "_cpp_ms"], h = best_ms(lambda: host.rule_splits(*args, max_consequent=M, **kw))
        out[name + "_agree"] = all(np.array_equal(d[f].cpu().numpy().view(np.int64) if d[f].dtype == torch.float64
                                                  else d[f].cpu().numpy(),
                                                  getattr(h, f).view(np.int64) if getattr(h, f).dtype == np.float64
                                                  else getattr(h, f)) for f in d)
        del d, h
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
