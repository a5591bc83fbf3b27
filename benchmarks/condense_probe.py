"""Closed itemsets of a mined result: MiningResult.condensed("closed") on the device (the
upload and the kept rows' readback included), k_sup_mark alone (device events), and the same
call on the C++ path at the host's thread count.

    python benchmarks/condense_probe.py [--config T40I10D10M] [--reps 7] [--warmup 2]

Mines the config once on cuda:0, then times; one JSON line with the median and the spread
(min, max) of every figure, the kept counts of both forms and whether device and host agree.
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _stats(ms: list) -> dict:
    return {"median_ms": round(statistics.median(ms), 3), "min_ms": round(min(ms), 3), "max_ms": round(max(ms), 3),
            "reps": len(ms)}


def main():
    import torch
    import bench
    from fastapriori_amd.models.apriori import FastApriori, MinerConfig
    from fastapriori_amd.ops import primitives as prim
    from fastapriori_amd.parallel.comm import Comm
    from fastapriori_amd.utils.env import num_threads
    from fastapriori_amd.utils.io import generate_shard
    from fastapriori_amd.utils.metrics import Logger

    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="T40I10D10M")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("condense_probe needs a GPU: its figures are device times")
    n, L, I, P, N, ms = bench.CONFIGS[a.config]
    dev = torch.device("cuda", 0)
    sh = generate_shard(n, Comm(device=dev), dev, L, I, P, N, 1)
    res = FastApriori(ms, config=MinerConfig(min_support=ms), logger=Logger(enabled=False)).run(sh)
    del sh
    out = {"config": a.config, "n_itemsets": res.n_itemsets, "levels": len(res.levels),
           "elements": int(sum(len(l) * k for k, l in enumerate(res.levels, 1) if k >= 2)),
           "host_threads": num_threads()}

    def timed(device):
        torch.cuda.synchronize()
        t = time.perf_counter()
        r = res.condensed("closed", device=device)
        torch.cuda.synchronize()
        return (time.perf_counter() - t) * 1e3, r

    runs = {}
    for name, d in (("device", dev), ("host", None)):
        for _ in range(a.warmup):
            timed(d)
        got = [timed(d) for _ in range(a.reps)]
        out[name + "_closed"] = _stats([g[0] for g in got])
        runs[name] = got[-1][1]
    out["n_closed"] = runs["device"].n_itemsets
    out["n_maximal"] = res.condensed("maximal", device=dev).n_itemsets
    out["device_equals_host"] = runs["device"].digest() == runs["host"].digest()

    # the kernel alone: the uploaded state once, then the launch between two events
    m = prim.condense_marks(res.levels, res.counts, dev)
    for _ in range(a.warmup):
        prim._condense_launch(m)
    kern = []
    for _ in range(a.reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        prim._condense_launch(m)
        e1.record()
        e1.synchronize()
        kern.append(e0.elapsed_time(e1))
    prim.condense_check(m)
    out["kernel"] = _stats(kern)
    out["device_faster_than_host"] = out["device_closed"]["median_ms"] < out["host_closed"]["median_ms"]
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
