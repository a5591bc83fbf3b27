"""Leave-one-out ranks: the one-kernel path (AssociationRules.holdout_ranks_shard) against the
composition from the parts that existed before it, on the device.

    python benchmarks/evaluate_probe.py [--config T10I4D100M] [--n 10] [--reps 3] [--warmup 1]

The composition is timed end to end like the kernel path: the same basket preparation
(_prepare_baskets, de-duplicated), then one explicit basket B - {h} per trial built with torch
ops, recommend_topn over all of them, the lookup of h in every list and the fan-out to the
lines.  Two data sets -- the headline's rules with a 1 M-line generated U.dat, and the mined
case of tests/test_gpu_recommend_topn.py -- each with the scan and the indexed kernels.  Host
clock around work that ends in a device synchronise; warm runs, the two paths alternating;
min / median / max over the repetitions.  The two results are compared bit for bit before any
time is reported, and the probe fails when they differ.  One JSON line.
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


def composed_ranks(ar, users, n):
    """(boff, ranks) as holdout_ranks_shard returns them, from recommend_topn."""
    import torch
    from fastapriori_amd import ops
    (a_off, ante, cons), index, F1, boff, bask, inv = ar._prepare_baskets(users)
    dev = bask.device
    M, nnz = boff.numel() - 1, bask.numel()
    cnt = boff[1:] - boff[:-1]
    trow = torch.repeat_interleave(torch.arange(M, device=dev), cnt)
    tsz = cnt[trow] - 1                                         # trial t: its row without element t
    toff = torch.zeros(nnz + 1, dtype=torch.int64, device=dev)
    torch.cumsum(tsz, 0, out=toff[1:])
    total = int(toff[-1])
    tt = torch.repeat_interleave(torch.arange(nnz, device=dev), tsz)
    k = torch.arange(total, device=dev) - toff[tt]
    j = torch.arange(nnz, device=dev) - boff[trow]              # the hidden element's place in its row
    tbask = bask[boff[trow[tt]] + k + (k >= j[tt]).to(torch.int64)].contiguous()
    top = ops.recommend_topn(a_off, ante, cons, F1, toff, tbask, n, index=index)
    item = torch.where(top >= 0, cons[top.clamp(min=0).to(torch.int64)], torch.full_like(top, -1))
    at = item == bask[:, None]
    ranks = torch.where(at.any(1), at.to(torch.int32).argmax(1).to(torch.int32) + 1,
                        torch.zeros((), dtype=torch.int32, device=dev))
    if inv is None:
        return boff, ranks
    lcnt = cnt[inv]
    loff = torch.zeros(inv.numel() + 1, dtype=torch.int64, device=dev)
    torch.cumsum(lcnt, 0, out=loff[1:])
    pos = torch.repeat_interleave(boff[inv] - loff[:-1], lcnt) + torch.arange(int(loff[-1]), device=dev)
    return loff, ranks[pos].contiguous()


def compare(ar, users, n, reps, warmup) -> dict:
    import torch

    def timed(fn):
        torch.cuda.synchronize()
        t = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t) * 1e3, out

    paths = {"kernel": lambda: ar.holdout_ranks_shard(users, n), "composition": lambda: composed_ranks(ar, users, n)}
    for _ in range(warmup):
        outs = {k: timed(f)[1] for k, f in paths.items()}
    equal = all(torch.equal(a, b) for a, b in zip(outs["kernel"], outs["composition"]))
    if not equal:
        raise SystemExit("evaluate_probe: the kernel's ranks differ from the composition's")
    ms = {k: [] for k in paths}
    for _ in range(reps):
        for k, f in paths.items():                              # alternating
            ms[k].append(timed(f)[0])
    boff, ranks = outs["kernel"]
    cnt = boff[1:] - boff[:-1]
    out = {"lines": int(boff.numel() - 1), "distinct_baskets": int(ar.stats["distinct_baskets"]),
           "elements": int(ranks.numel()), "trials": int(cnt[cnt >= 2].sum()), "hits": int((ranks > 0).sum()),
           "bit_equal": equal, "kernel": _stats(ms["kernel"]), "composition": _stats(ms["composition"])}
    out["composition_over_kernel"] = round(out["composition"]["median_ms"] / out["kernel"]["median_ms"], 2)
    return out


def main():
    import torch
    import bench
    from fastapriori_amd.models.apriori import FastApriori, MinerConfig
    from fastapriori_amd.models.rules import AssociationRules
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
        raise SystemExit("evaluate_probe needs a GPU: its figures are device times")
    dev = torch.device("cuda", 0)
    comm, quiet = Comm(device=dev), Logger(enabled=False)
    rows, L, I, P, N, ms = bench.CONFIGS[a.config]
    cases = {a.config: ((rows, L, I, P, N, 1), ms, (bench.U_LINES, L, I, P, N, 2)),
             "mined test case": ((20000, 8.0, 3.0, 80, 100, 9), 0.01, (3000, 8.0, 3.0, 80, 100, 9))}
    out = {"n": a.n, "cases": {}}
    for name, (d, sup, u) in cases.items():
        sh = generate_shard(d[0], comm, dev, *d[1:5], seed=d[5])
        res = FastApriori(sup, config=MinerConfig(min_support=sup), logger=quiet).run(sh)
        del sh
        users = generate_shard(u[0], comm, dev, *u[1:5], seed=u[5], users=True)
        case = {"n_rules": None}
        for kernel in ("indexed", "scan"):
            ar = AssociationRules(res, device=dev, logger=quiet)
            ar.use_index = kernel == "indexed"
            case["n_rules"] = ar.rules().n_rules
            case[kernel] = compare(ar, users, a.n, a.reps, max(a.warmup, 1))
        out["cases"][name] = case
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
