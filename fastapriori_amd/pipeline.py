"""The end-to-end job: Main.main of the reference (Main.scala:16-38).

    read D.dat/U.dat shards -> mine -> write freqItemset -> rules -> recommend
    -> write recommends

One process per GPU (torchrun); rank 0 writes the outputs.  Phase timings are
printed as the reference does ("==== Total time for get freqItemsets ..."); the
mining window includes reading and parsing D.dat, like the reference's lazy
RDD read makes it do.
"""
from __future__ import annotations

import json
import os
import time

from .config import JobConfig
from .models.apriori import FastApriori, MinerConfig
from .models.rules import AssociationRules
from .parallel.comm import Comm, init_comm, shutdown_comm
from .utils import io
from .utils.checkpoint import Checkpointer, input_fingerprint
from .utils.metrics import Logger


def _load_checkpoint(ckpt: Checkpointer, comm, require_complete: bool = False):
    """Rank 0 reads the checkpoint and sends it to every rank, so all ranks resume
    from the same level (a per-rank read could race rank 0's rewrite of meta.json,
    or miss a temp dir that is not shared, and then the ranks' collectives diverge)."""
    res, err = None, None
    if comm.is_root:
        try:
            res = ckpt.load(require_complete=require_complete)
        except (OSError, ValueError, KeyError) as e:
            err = f"{type(e).__name__}: {e}"
    res, err = comm.broadcast_object((res, err))
    if err:
        raise ValueError(f"checkpoint load failed on rank 0: {err}")
    return res


def _load_saved(cfg: JobConfig, comm):
    """Rank 0 rebuilds the mined result from the saved ``freqItems`` / ``ItemsToRank``
    files (io.load_saved_results, the reference's Utils.getAll) and sends it to every
    rank; None when the files are missing."""
    freq, rank = cfg.output + "freqItems", cfg.output + "ItemsToRank"
    res, err = None, None
    if comm.is_root and os.path.exists(rank) and os.path.exists(freq):
        try:
            res = io.load_saved_results(freq, rank)
        except (OSError, ValueError, KeyError) as e:
            err = f"{type(e).__name__}: {e}"
    res, err = comm.broadcast_object((res, err))
    if err:
        raise ValueError(f"loading {freq} failed on rank 0: {err}")
    return res


def mine_window(cfg: JobConfig, comm, log: Logger, ckpt: Checkpointer | None, summary: dict):
    """The reference's timed mining window (Main.scala:28-32): read + parse D.dat,
    mine, write freqItemset (and, with a temp path, the per-level checkpoint).
    bench.py times this same function for its e2e record."""
    d_path, out_freq = cfg.input + "D.dat", cfg.output + "freqItemset"
    resume = _load_checkpoint(ckpt, comm) if (ckpt is not None and cfg.resume) else None
    # candidate distribution: every rank holds the whole DB
    t_read = time.time()
    shard = io.read_shard(d_path, comm if cfg.strategy == "count" else Comm(device=comm.device))
    summary["read_ms"] = round((time.time() - t_read) * 1000, 1)
    # --profile: hipEvent phase times per level and a Chrome trace of the phases
    mcfg = MinerConfig(min_support=cfg.min_support, dedup=cfg.dedup, pair_strategy=cfg.pair_strategy,
                       max_level=cfg.max_level, parallelism=cfg.strategy, tiebreak=cfg.tiebreak,
                       timing="events" if cfg.profile else "off", trace=cfg.profile)
    miner = FastApriori(cfg.min_support, comm, mcfg, log, ckpt)
    result = miner.run(shard, resume=resume)
    summary["miner"] = dict(miner.stats)
    summary["device_bundles"] = int(miner.stats.get("device_bundles", 0))
    trace = summary["miner"].pop("trace", None)
    if cfg.profile and trace is not None and comm.is_root:
        # Chrome trace of the mining phases (host spans + hipEvent device spans)
        tpath = os.path.join(cfg.temp or ".", "fastapriori_trace.json")
        with open(tpath, "w") as f:
            json.dump({"traceEvents": trace, "displayTimeUnit": "ms"}, f)
        summary["trace_path"] = tpath
    del shard
    t_write = time.time()
    if comm.is_root:
        io.write_freq_itemsets(result, out_freq, overwrite=cfg.overwrite)
        if cfg.with_counts:
            io.write_freq_itemsets(result, cfg.output + "freqItems", with_counts=True, overwrite=cfg.overwrite)
            io.write_items_to_rank(result, cfg.output + "ItemsToRank")
            io.write_freq_items(result, cfg.output + "FreqItems")
    if ckpt is not None:
        # the completion follows the level files the device loop queued on the checkpoint
        # thread; the job joins it at its end (run_job), not inside this window
        ckpt.mark_complete(result, background=True)
    comm.barrier()
    summary["write_ms"] = round((time.time() - t_write) * 1000, 1)
    return result


def recommend_window(cfg: JobConfig, comm, log: Logger, result, summary: dict) -> list:
    """The reference's second timed window (Main.scala:34-37): read + parse U.dat,
    rules (generation, cut, sort), one recommendation per user line, write
    recommends.  bench.py times this same function for its e2e record."""
    t0 = time.perf_counter()
    users = io.read_shard(cfg.input + "U.dat", comm)
    t1 = time.perf_counter()
    ar = AssociationRules(result, comm, log)
    ar.rules()
    t2 = time.perf_counter()
    recs = ar.run(users)
    t3 = time.perf_counter()
    if comm.is_root:
        io.write_lines(recs, cfg.output + "recommends", overwrite=cfg.overwrite)
    comm.barrier()
    t4 = time.perf_counter()
    # host wall time of each step (a step's device work ends inside the next host readback)
    summary["recommend_steps_ms"] = {k: round(v * 1e3, 1) for k, v in
                                     (("read_U", t1 - t0), ("rules", t2 - t1), ("recommend", t3 - t2),
                                      ("write", t4 - t3))}
    if cfg.top_n > 0:
        # ranked lists next to the first-match file (no counterpart in the reference)
        # (--combine sum | votes: listed by the summed weights of all firing rules)
        top = ar.run_topn(users, cfg.top_n, scores=cfg.top_n_scores, combine=cfg.combine)
        if comm.is_root:
            io.write_lines(top, cfg.output + "recommendsTopN", overwrite=cfg.overwrite)
            summary.update(top_n=cfg.top_n, n_topn_entries=sum(0 if l == "0" else l.count(" ") + 1 for l in top))
        if cfg.combine != "first":
            summary["combine"] = cfg.combine
        comm.barrier()
        summary["recommend_steps_ms"]["topn"] = round((time.perf_counter() - t4) * 1e3, 1)
    summary["n_rules"] = ar.rules().n_rules
    if recs is not None:                   # rank 0 holds every user's recommendation
        summary.update(n_users=len(recs), n_recommended=sum(1 for r in recs if r != "0"))
    return recs


def evaluate_window(cfg: JobConfig, comm, log: Logger, result, summary: dict) -> None:
    """--evaluate N / --evaluate-ranks (no counterpart in the reference): after the
    recommendation window, so neither of the reference's timed windows gets slower.  It reads
    U.dat itself, as count_window reads D.dat, and builds the rules again without their log
    lines.  Every rank ranks the trials of its own lines (AssociationRules.run_evaluate); the
    integers are all-reduced, so every rank holds the same Evaluation; rank 0 writes
    ``<output>evaluation`` (one JSON line) and, with --evaluate-ranks, ``<output>evaluationRanks``
    (one line per U.dat line), and the others meet it where it reports how that went."""
    t0 = time.perf_counter()
    users = io.read_shard(cfg.input + "U.dat", comm)
    ar = AssociationRules(result, comm, Logger(comm.rank, enabled=False))
    ev, lines = ar.run_evaluate(users, cfg.evaluate, rank_lines=cfg.evaluate_ranks, combine=cfg.combine)
    for f in ar.stats.get("fallbacks", ()):
        log.metric(phase="fallback", what=f, stage="evaluate")
    err = None
    if comm.is_root:
        try:
            io.write_lines([ev.as_json()], cfg.output + "evaluation", overwrite=cfg.overwrite)
            if cfg.evaluate_ranks:
                io.write_lines(lines, cfg.output + "evaluationRanks", overwrite=cfg.overwrite)
        except (OSError, RuntimeError, ValueError) as e:
            err = f"{type(e).__name__}: {e}"
    err = comm.broadcast_object(err)                           # the ranks' meeting point
    if err:
        raise RuntimeError(f"--evaluate failed on rank 0: {err}")
    ms = int((time.perf_counter() - t0) * 1000)
    log.line(f"Total time for get evaluation {ms}")
    mode = {"combine": ev.combine} if ev.combine != "first" else {}
    log.metric(phase="evaluate", n=ev.n, n_lines=ev.n_lines, n_lines_skipped=ev.n_lines_skipped,
               n_trials=ev.n_trials, n_infrequent_tokens=ev.n_infrequent_tokens, hits=ev.hits, ms=ms, **mode)
    summary.update(evaluate_n=ev.n, n_trials=ev.n_trials, hit_rate_at_n=ev.hit_rate[-1], mrr=ev.mrr, **mode)


def count_window(cfg: JobConfig, comm, log: Logger, result, summary: dict) -> None:
    """--count-itemsets / --verify-counts (no counterpart in the reference): after the
    mining window and before condense_window, so neither of the reference's timed windows
    gets slower.  It reads D.dat itself, as mine_window does and with the same --strategy
    (mine_window keeps nothing of its shard), and counts with models.query.count_itemsets,
    which shares nothing with the miner.

    --count-itemsets PATH: rank 0 reads the query file and sends the queries to every
    rank, all ranks count, rank 0 writes ``<output>itemsetCounts`` -- line i: query line
    i's distinct tokens in first-occurrence order, one space apart, then ``[count]`` -- and
    the others meet it where it reports how that went.  --verify-counts: every mined
    itemset of two or more items is recounted and compared with the mined count (level 1
    counts occurrences, the query counter lines: docs/PARITY.md); the vectors are identical
    on every rank, so a difference raises on every rank."""
    from .models.query import ItemsetQueries, count_itemsets, result_counts
    t0 = time.perf_counter()
    whole = Comm(device=comm.device)
    shard = io.read_shard(cfg.input + "D.dat", comm if cfg.strategy == "count" else whole)
    if cfg.count_itemsets:
        queries, err = None, None
        if comm.is_root:
            try:
                queries = ItemsetQueries.from_file(cfg.count_itemsets)
            except (OSError, RuntimeError, ValueError) as e:
                err = f"{type(e).__name__}: {e}"
        queries, err = comm.broadcast_object((queries, err))
        if err:
            raise RuntimeError(f"--count-itemsets: reading {cfg.count_itemsets} failed on rank 0: {err}")
        counts = count_itemsets(shard, queries, comm, cfg.strategy)
        n, err = None, None
        if comm.is_root:
            try:
                lines = [" ".join(queries.query_tokens(i)) + f"[{c}]" for i, c in enumerate(counts.tolist())]
                io.write_lines(lines, cfg.output + "itemsetCounts", overwrite=cfg.overwrite)
                n = len(lines)
            except (OSError, RuntimeError, ValueError) as e:
                err = f"{type(e).__name__}: {e}"
        n, err = comm.broadcast_object((n, err))                   # the ranks' meeting point
        if err:
            raise RuntimeError(f"--count-itemsets failed on rank 0: {err}")
        ms = int((time.perf_counter() - t0) * 1000)
        log.line(f"Total time for get itemsetCounts {ms}")
        log.metric(phase="count_itemsets", n_queries=n, ms=ms)
        summary["n_counted"] = n
    if cfg.verify_counts:
        t1 = time.perf_counter()
        queries = ItemsetQueries.from_result(result, min_size=2)
        got = count_itemsets(shard, queries, comm, cfg.strategy)
        want = result_counts(result, min_size=2)
        bad = (got != want).nonzero()[0]
        if len(bad):
            i = int(bad[0])
            raise RuntimeError(f"--verify-counts: itemset {{{' '.join(queries.query_tokens(i))}}} was mined with count "
                               f"{int(want[i])} but {int(got[i])} lines of D.dat contain it "
                               f"({len(bad)} of {len(want)} itemsets differ)")
        log.line(f"verified {len(want)} itemset counts")
        log.metric(phase="verify_counts", n_verified=len(want), ms=int((time.perf_counter() - t1) * 1000))
        summary["n_verified"] = len(want)


CONDENSED_DIRS = {"closed": "closedItemset", "maximal": "maximalItemset"}


def condense_window(cfg: JobConfig, comm, log: Logger, result, summary: dict) -> None:
    """--closed / --maximal (no counterpart in the reference): between its two timed
    windows, so neither gets slower.  Every rank holds the identical result: rank 0
    alone computes on its device and writes ``<output>closedItemset`` /
    ``<output>maximalItemset`` ("a b c[cnt]" lines, the format io.load_saved_results
    reads back); the others meet it where it reports how that went."""
    for kind in [k for k in ("closed", "maximal") if getattr(cfg, k)]:
        t0 = time.perf_counter()
        n_kept, err = None, None
        if comm.is_root:
            try:
                kept = result.condensed(kind, device=comm.device)
                io.write_freq_itemsets(kept, cfg.output + CONDENSED_DIRS[kind], with_counts=True,
                                       overwrite=cfg.overwrite)
                n_kept = kept.n_itemsets
            except (OSError, RuntimeError, ValueError) as e:
                err = f"{type(e).__name__}: {e}"
        n_kept, err = comm.broadcast_object((n_kept, err))     # the ranks' meeting point
        if err:
            raise RuntimeError(f"--{kind} failed on rank 0: {err}")
        ms = int((time.perf_counter() - t0) * 1000)
        log.line(f"Total time for get {kind}Itemsets {ms}")
        log.metric(phase="condense", kind=kind, n_all=result.n_itemsets, n_kept=n_kept, ms=ms)
        summary[f"n_{kind}"] = n_kept


def rules_window(cfg: JobConfig, comm, log: Logger, result, summary: dict) -> None:
    """--rules (no counterpart in the reference): after condense_window and before the
    recommendation window, so neither of the reference's timed windows gets slower.  Every
    rank holds the identical result: rank 0 alone computes AssociationRules.all_rules on its
    device (with --rules-max-consequent M: consequents of up to M items) and writes
    ``<output>rules`` (io.write_rules); the others meet it where it
    reports how that went, and a failure raises on every rank."""
    t0 = time.perf_counter()
    n, err = None, None
    if comm.is_root:
        try:
            ar = AssociationRules(result, comm, Logger(enabled=False))
            rm = ar.all_rules(cfg.min_confidence, cfg.min_lift, cfg.rules_sort, cfg.rules_limit,
                              cfg.rules_max_consequent)
            io.write_rules(rm, result.items, cfg.output + "rules", overwrite=cfg.overwrite)
            n = rm.n_rules
        except (OSError, RuntimeError, ValueError) as e:
            err = f"{type(e).__name__}: {e}"
    n, err = comm.broadcast_object((n, err))                   # the ranks' meeting point
    if err:
        raise RuntimeError(f"--rules failed on rank 0: {err}")
    ms = int((time.perf_counter() - t0) * 1000)
    log.line(f"Total time for get rules {ms}")
    log.metric(phase="rules_export", n_rules=n, min_confidence=cfg.min_confidence, min_lift=cfg.min_lift,
               sort=cfg.rules_sort, limit=cfg.rules_limit, max_consequent=cfg.rules_max_consequent, ms=ms)
    summary["n_rules_exported"] = n
    summary["rules_max_consequent"] = cfg.rules_max_consequent


def make_checkpointer(cfg: JobConfig, comm) -> Checkpointer | None:
    if cfg.temp and (cfg.checkpoint or cfg.rules_only) and not cfg.count_only:
        # rules-only needs no D.dat: it reloads the mined itemsets (Utils.getAll's use case)
        fp = None if cfg.rules_only else input_fingerprint(cfg.input + "D.dat", cfg.min_support)
        return Checkpointer(cfg.temp, comm.rank, fp)
    return None


def run_job(cfg: JobConfig, comm=None) -> dict:
    own_comm = comm is None
    if comm is None:
        dev = None if cfg.device == "auto" else cfg.device
        comm = init_comm(dev)
    if cfg.world_size and comm.world_size != cfg.world_size:
        if own_comm:
            shutdown_comm(comm)
        raise RuntimeError(f"--world-size {cfg.world_size} but the process group has {comm.world_size} ranks")
    log = Logger(comm.rank, metrics_path=cfg.metrics_path)
    summary: dict = {}
    ckpt = None
    try:
        ckpt = make_checkpointer(cfg, comm)
        comm.barrier()

        if cfg.count_only:
            # --count-itemsets PATH --count-only: D.dat is read, counted and written; nothing is mined
            count_window(cfg, comm, log, None, summary)
            summary.update(world_size=comm.world_size)
            log.metric(phase="job", **{k: v for k, v in summary.items() if not isinstance(v, dict)})
            return summary

        t1 = time.time()
        if cfg.rules_only:
            # the complete checkpoint under temp, else the saved result files of a
            # --with-counts run (freqItems + ItemsToRank: Utils.getAll, Utils.scala:65-81)
            result = _load_checkpoint(ckpt, comm, require_complete=True) if ckpt is not None else None
            if result is None:
                result = _load_saved(cfg, comm)
            if result is None:
                where = f"under {ckpt.dir} " if ckpt is not None else ""
                raise FileNotFoundError(f"--rules-only: no complete checkpoint {where}and no "
                                        f"{cfg.output}freqItems + {cfg.output}ItemsToRank (written by --with-counts)")
            comm.barrier()
        else:
            result = mine_window(cfg, comm, log, ckpt, summary)
        t_mine = int((time.time() - t1) * 1000)
        log.line(f"Total time for get freqItemsets {t_mine}")

        if cfg.count_itemsets or cfg.verify_counts:
            count_window(cfg, comm, log, result, summary)
        if cfg.closed or cfg.maximal:
            condense_window(cfg, comm, log, result, summary)
        if cfg.rules:
            rules_window(cfg, comm, log, result, summary)

        t2 = time.time()
        recommend_window(cfg, comm, log, result, summary)
        t_rec = int((time.time() - t2) * 1000)
        log.line(f"Total time for get recommends {t_rec}")
        if cfg.evaluate > 0:
            evaluate_window(cfg, comm, log, result, summary)
        summary.update(mine_ms=t_mine, recommend_ms=t_rec, n_itemsets=result.n_itemsets,
                       world_size=comm.world_size)
        log.metric(phase="job", **{k: v for k, v in summary.items() if not isinstance(v, dict)})
        return summary
    except BaseException as e:
        # the job's own failure wins: a background checkpoint error is only attached to it
        if ckpt is not None:
            try:
                ckpt.wait()
            except BaseException as ck_err:   # noqa: BLE001 (logged; the original error propagates)
                import sys
                print(f"fastapriori: checkpoint thread also failed: {type(ck_err).__name__}: {ck_err}",
                      file=sys.stderr)
                log.metric(phase="checkpoint_error", error=f"{type(ck_err).__name__}: {ck_err}")
            ckpt = None
        raise e
    finally:
        if ckpt is not None:
            ckpt.wait()                  # the checkpoint is complete before the job returns
        if own_comm:
            shutdown_comm(comm)


def _relaunch(cfg: JobConfig, argv) -> int:
    """``--world-size N`` from a plain ``python -m fastapriori_amd``: start N ranks (one per
    GPU) under torch.distributed.run.  This parent process never touches the GPU."""
    import subprocess
    import sys

    from .parallel.launch import free_port
    argv = list(sys.argv[1:] if argv is None else argv)
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={cfg.world_size}",
           "--master-addr", "127.0.0.1", f"--master-port={free_port()}", "-m", "fastapriori_amd", *argv]
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    return subprocess.call(cmd, env=env)


def main(argv=None) -> int:
    from .config import parse_args
    cfg = parse_args(argv)
    if cfg.world_size > 1 and "WORLD_SIZE" not in os.environ:
        return _relaunch(cfg, argv)
    if cfg.profile and not cfg.metrics_path:
        # --profile: JSON-lines metrics (per-level device times, bytes reduced, HBM bytes
        # estimates) and a Chrome trace of the phases (mine_window), both under the temp path
        cfg.metrics_path = os.path.join(cfg.temp or ".", "fastapriori_metrics.jsonl")
    run_job(cfg)
    return 0
