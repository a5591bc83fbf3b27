"""Support counts of GIVEN itemsets over a transaction shard (no counterpart in the
reference, which counts only what it mines): ``count_itemsets``.

A *query* is a set of tokens -- one line of a query file, tokenised exactly as a D.dat
line (a blank line is the empty token, repeated tokens collapse) -- and its *count* the
number of D.dat lines that contain every one of them: a LINE count over the shard's
distinct ids per line (``TransactionShard.items``; ``extras`` are ignored), so a one-item
query can be smaller than the item's mined level-1 count, which counts occurrences
(docs/PARITY.md).  A query with a token the database does not hold counts 0; query i
answers at position i, duplicates each.

The counter goes back to the raw parsed rows and shares nothing with the miner: the plan
and the kernel are ops.primitives.query_plan / query_count (csrc/host/query.cpp,
csrc/hip/query.hip), so a mined result can be checked against it (--verify-counts).
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np
import torch

from ..ops import primitives as prim
from ..parallel.comm import Comm
from .data import MiningResult, TransactionShard, Vocabulary, hash_tokens


@dataclass
class ItemsetQueries:
    """Q queries over T distinct tokens: ``off`` int64 [Q + 1] and ``idx`` int32 index a
    query's tokens in ``tokens`` (first-occurrence order; a token may repeat inside a
    query, it collapses when counted).  ``hashes``: the parser's 64-bit hash of every token
    when they come from a dictionary-mode file (the raw bytes' identity; a token with
    invalid UTF-8 would hash differently once decoded), else None."""
    tokens: list[str]
    off: np.ndarray
    idx: np.ndarray
    hashes: np.ndarray | None = None

    @property
    def n_queries(self) -> int:
        return len(self.off) - 1

    def query_tokens(self, i: int) -> list[str]:
        """Query i's distinct tokens in first-occurrence order."""
        seen, out = set(), []
        for j in self.idx[int(self.off[i]):int(self.off[i + 1])].tolist():
            if j not in seen:
                seen.add(j)
                out.append(self.tokens[j])
        return out

    @classmethod
    def from_lists(cls, queries) -> "ItemsetQueries":
        """From token lists.  A blank query line is the list [""]; an empty list is refused
        (it would be contained in every line, which no file line can say)."""
        tok_id: dict[str, int] = {}
        off, idx = [0], []
        for i, q in enumerate(queries):
            q = list(q)
            if not q:
                raise ValueError(f"query {i} has no token (a blank line is the token '')")
            for t in q:
                idx.append(tok_id.setdefault(str(t), len(tok_id)))
            off.append(len(idx))
        return cls(list(tok_id), np.asarray(off, dtype=np.int64), np.asarray(idx, dtype=np.int32))

    @classmethod
    def from_shard(cls, shard: TransactionShard) -> "ItemsetQueries":
        """From a parsed query file (every line, in file order)."""
        v = shard.vocab
        ids = shard.items.cpu().numpy()
        off = shard.offsets.cpu().numpy().astype(np.int64)
        used, inv = np.unique(ids, return_inverse=True)
        tokens = [v.token(int(i)) for i in used] if v.numeric else v.decode(used)
        hashes = None if v.numeric else np.asarray(v.hashes, dtype=np.uint64)[used]
        return cls(tokens, off, inv.astype(np.int32).reshape(-1), hashes)

    @classmethod
    def from_file(cls, path: str) -> "ItemsetQueries":
        """From a query file, parsed by the D.dat parser on the host (the host parser keeps
        a line's tokens in first-occurrence order).  Every caller reads the whole file."""
        from ..utils import io
        return cls.from_shard(io.read_shard(path, Comm(), "cpu"))

    @classmethod
    def from_result(cls, result: MiningResult, min_size: int = 1) -> "ItemsetQueries":
        """Every mined itemset of at least ``min_size`` items, level by level in row order
        (the order of ``result_counts``)."""
        off, idx = [np.zeros(1, dtype=np.int64)], []
        base = 0
        for k, rows in enumerate(result.levels, 1):
            rows = np.asarray(rows, dtype=np.int32).reshape(-1, k)
            if k < min_size or not len(rows):
                continue
            off.append(base + k * np.arange(1, len(rows) + 1, dtype=np.int64))
            idx.append(rows.reshape(-1))
            base += rows.size
        hashes = result.item_hashes
        if hashes is not None and len(hashes) != len(result.items):
            hashes = None
        return cls(list(result.items), np.concatenate(off), np.concatenate(idx) if idx else np.zeros(0, np.int32),
                   None if hashes is None else np.asarray(hashes, dtype=np.uint64))


def result_counts(result: MiningResult, min_size: int = 1) -> np.ndarray:
    """The mined counts in ItemsetQueries.from_result's order."""
    parts = [np.asarray(c, dtype=np.int64).ravel() for k, c in enumerate(result.counts, 1) if k >= min_size]
    return np.concatenate(parts) if parts else np.zeros(0, dtype=np.int64)


def _token_ids(queries: ItemsetQueries, vocab: Vocabulary) -> np.ndarray:
    """Database id of every query token, -1 when the database does not hold it (as
    AssociationRules._rank_lut: numeric ids by value, dictionary ids through the hashes)."""
    T = len(queries.tokens)
    ids = np.full(T, -1, dtype=np.int64)
    if not T or not vocab.size:
        return ids
    if vocab.numeric:
        for j, t in enumerate(queries.tokens):
            i = Vocabulary.numeric_id(t)
            if 0 <= i < vocab.size:
                ids[j] = i
        return ids
    qh = queries.hashes if queries.hashes is not None else hash_tokens(queries.tokens)
    qh = np.asarray(qh, dtype=np.uint64)
    vh = np.asarray(vocab.hashes, dtype=np.uint64)
    vo = np.argsort(vh)
    pos = np.minimum(np.searchsorted(vh[vo], qh), vh.size - 1)
    hit = vh[vo][pos] == qh
    ids[hit] = vo[pos[hit]]
    return ids


def plan_queries(queries: ItemsetQueries, vocab: Vocabulary) -> tuple[np.ndarray, dict]:
    """(lut int32 [vocab.size]: database id -> used index or -1, the window plan) of the
    queries against a database vocabulary.  Dead queries (an absent token) never reach the
    plan; repeated tokens of a query collapse."""
    Q = queries.n_queries
    tid = _token_ids(queries, vocab)
    # used index = a present token's place among the queries' present tokens: it does not
    # depend on the database's id assignment, so ranks that hold the same database cut the
    # same windows whatever ids their parsers gave
    present = tid >= 0
    tu = np.where(present, np.cumsum(present) - 1, -1).astype(np.int64)
    off = np.asarray(queries.off, dtype=np.int64)
    qu = tu[np.asarray(queries.idx, dtype=np.int64)]              # used index per query entry
    qof = np.repeat(np.arange(Q, dtype=np.int64), np.diff(off))   # query per entry
    dead = np.zeros(Q, dtype=bool)
    dead[qof[qu < 0]] = True
    keep = ~dead[qof]
    # distinct (query, used index) pairs, ascending inside a query
    pairs = np.unique(np.stack([qof[keep], qu[keep]], axis=1), axis=0) if keep.any() else np.zeros((0, 2), np.int64)
    live = np.flatnonzero(~dead & (np.diff(off) > 0))
    cnt = np.bincount(pairs[:, 0], minlength=Q)[live] if len(pairs) else np.zeros(len(live), np.int64)
    loff = np.zeros(len(live) + 1, dtype=np.int64)
    np.cumsum(cnt, out=loff[1:])
    lut = np.full(max(vocab.size, 1), -1, dtype=np.int32)
    lut[tid[present]] = tu[present].astype(np.int32)
    plan = prim.query_plan(loff, pairs[:, 1].astype(np.int32), live, int(present.sum()), Q)
    return lut, plan


def count_itemsets(shard: TransactionShard, queries: ItemsetQueries, comm: Comm | None = None,
                   strategy: str = "count") -> np.ndarray:
    """Lines of the database that contain every token of each query -> int64 [Q], query
    order, identical on every rank.

    ``strategy="count"``: ``shard`` is this rank's part of the database; every rank counts
    its own rows and one all-reduce of the vector assembles the result (a rank with an
    empty shard still takes part).  ``"candidate"``: every rank holds the whole database
    and counts the windows w with w % world_size == rank; the same all-reduce follows.
    In dictionary mode the vocabulary is the shard's own, so each rank plans against its
    shard (a token the shard does not hold is in none of its lines).  A shard on a GPU is
    counted by the HIP kernel, a CPU shard by the C++ path."""
    if strategy not in ("count", "candidate"):
        raise ValueError(f"count_itemsets: strategy must be 'count' or 'candidate', not {strategy!r}")
    comm = comm or Comm()
    err = None
    try:
        lut, plan = plan_queries(queries, shard.vocab)
    except ValueError as e:
        err = e
    # a dictionary shard plans against its own vocabulary, so a plan can fail on one rank
    # alone: the ranks agree on that before the counts' collective
    if comm.allreduce_int(0 if err is None else 1, "max"):
        raise err if err is not None else ValueError("count_itemsets: the query plan failed on another rank")
    dev = shard.items.device
    windows = (comm.rank, comm.world_size) if (strategy == "candidate" and comm.world_size > 1) else None
    cnt = prim.query_count(shard.offsets, shard.items, torch.from_numpy(lut).to(dev), plan, windows=windows)
    if comm.world_size > 1:
        full = torch.zeros(max(queries.n_queries, 1), dtype=torch.int64, device=dev)
        full[:queries.n_queries] = cnt
        cnt = comm.all_reduce_(full)[:queries.n_queries]
    return cnt.cpu().numpy()
