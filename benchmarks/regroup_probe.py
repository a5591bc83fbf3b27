"""Grouping figures of the regrouping step (csrc/hip/regroup.hip) on a config's last device
bundle: per level the prefix plan's pieces against the regrouped plan's, and the prefix rows
they read (pieces x m), as the post step of a mining run left them; and where the rounds
kernel's time goes per level (its phase timers: setup, rounds, numbering, in microseconds).

    python benchmarks/regroup_probe.py [--config T10I4D100M] [--n-txn N]
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    import torch
    import bench
    from fastapriori_amd.models.apriori import FastApriori, MinerConfig
    from fastapriori_amd.ops import primitives as prim
    from fastapriori_amd.parallel.comm import Comm
    from fastapriori_amd.utils.io import generate_shard
    from fastapriori_amd.utils.metrics import Logger

    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default=bench.HEADLINE)
    ap.add_argument("--n-txn", type=int, default=0)
    a = ap.parse_args()
    n_txn, avg_len, avg_pat, n_pat, n_items, ms = bench.CONFIGS[a.config]
    comm = Comm(device=torch.device("cuda", 0))
    shard = generate_shard(a.n_txn or n_txn, comm, comm.device, avg_len, avg_pat, n_pat, n_items, 1)
    m = FastApriori(ms, comm, MinerConfig(min_support=ms), Logger(0, enabled=False))
    from fastapriori_amd.ops import _native
    phases = torch.zeros((prim.dl().kDlMaxL, 4), dtype=torch.int64, device=comm.device)
    _native.hip().fa_hip_debug_dl_regroup_phases(phases.data_ptr())
    try:
        m.run(shard)
        torch.cuda.synchronize()
    finally:
        _native.hip().fa_hip_debug_dl_regroup_phases(None)
    ph = phases.cpu().numpy()
    n, stats = prim.dl_regroup_last()
    shapes = m.stats.get("device_bundle_shapes")
    out = dict(config=a.config, bundles_regrouped=n, bundle_shapes=shapes, levels=[])
    if stats is not None:
        k0, L = shapes[-1][0], shapes[-1][1]
        assert L == len(stats)
        for l, (pp, pr, rounds, kept) in enumerate(stats.tolist()):
            mm = k0 - 1 + l
            used = pp if kept else pr
            out["levels"].append(dict(k=k0 + l, m=mm, pieces_prefix=pp, pieces_rule=pr, rounds=rounds,
                                      kept_prefix=kept, pieces=used,
                                      us=[round(float(x) / 100.0, 2) for x in ph[l, 1:] - ph[l, :-1]]))
        out["rounds_kernel_us"] = round(float(ph[:L, 3].max() - ph[:L, 0].min()) / 100.0, 2)
        out["pieces_prefix"] = sum(v["pieces_prefix"] for v in out["levels"])
        out["pieces"] = sum(v["pieces"] for v in out["levels"])
        out["prefix_rows_prefix"] = sum(v["pieces_prefix"] * v["m"] for v in out["levels"])
        out["prefix_rows"] = sum(v["pieces"] * v["m"] for v in out["levels"])
    print(json.dumps(out))


if __name__ == "__main__":
    main()
