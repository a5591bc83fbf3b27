"""Edge shapes of the rule kernels (csrc/hip/rules.hip) on the device.

Whole builder: every case of test_rule_edges.py through ops.primitives.rules_build_device,
against the same expected tables (the frozenset reference there, the oracle for the mined
cases), exactly; the inputs that must raise; and a --rules-only job over a cut file.

Single kernels: fa_hip_rule_gen, fa_hip_rule_cut and fa_hip_rule_emit called on tensors
built for one thing each -- thread totals around the workgroup size, one-row and one-column
levels, the ends of the binary search, counts that differ above bit 32, every (rule,
child) position of the cut, the strictness of its comparison -- against loops in numpy
and Python.  Every output buffer lies between guard words that must not change.
"""
import numpy as np
import pytest
import torch

from fastapriori_amd.ops import primitives as prim

from test_rule_edges import WHOLE, bad_cases, case, check_table, message, rules_only_job_on_a_cut_file

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
G = 64                                   # guard words on each side of an output


# ---------------------------------------------------------------------------
# the whole builder
# ---------------------------------------------------------------------------
@pytest.fixture
def argsorts(monkeypatch):
    """The keyword arguments of every torch.argsort call of the test."""
    seen = []
    fn = torch.argsort
    monkeypatch.setattr(torch, "argsort", lambda *a, **kw: seen.append(kw) or fn(*a, **kw))
    return seen


@pytest.mark.parametrize("name", WHOLE)
def test_device_builder(name, argsorts):
    levels, counts, tie, want = case(name)
    got = prim.rules_build_device(levels, counts, tie.copy(), DEV)      # the cases are read-only
    assert all(got[f].device.type == "cuda" for f in ("ante_off", "ante", "cons", "conf"))
    check_table(got, want)
    if len(want["cons"]):
        # the packed key below 128 levels, the two-pass ordering (a stable argsort) from there on
        assert [kw for kw in argsorts if kw.get("stable")] == ([dict(stable=True)] if len(levels) >= 128 else [])


def test_padded_lattice_equals_the_unpadded_one():
    a, b = case("lattice_live"), case("lattice_live_k128")
    assert len(a[0]) == 11 and len(b[0]) == 128 and a[3] is b[3]
    check_table(prim.rules_build_device(b[0], b[1], b[2].copy(), DEV), a[3])


@pytest.mark.parametrize("name", sorted(bad_cases()))
def test_device_builder_rejects(name):
    levels, counts, tie, k = bad_cases()[name]
    with pytest.raises(RuntimeError, match=message(k)):
        prim.rules_build_device(levels, counts, tie.copy(), DEV)


def test_rules_only_job_on_a_cut_file(tmp_path):
    from fastapriori_amd.parallel.comm import Comm
    rules_only_job_on_a_cut_file(tmp_path, "cuda", Comm(device=DEV))


# ---------------------------------------------------------------------------
# single kernels: buffers
# ---------------------------------------------------------------------------
FILL = {torch.int32: -0x5A5A5A5B, torch.float64: -12345.678, torch.uint8: 0xAB}


class Out:
    """An output of n elements with G guard elements before and after it."""

    def __init__(self, n, dtype):
        self.n, self.buf = n, torch.full((n + 2 * G,), FILL[dtype], dtype=dtype, device=DEV)
        self.ptr = self.buf.data_ptr() + G * self.buf.element_size()

    def get(self):
        """The n elements, after checking the guards."""
        h = self.buf.cpu()
        assert bool((h[:G] == FILL[h.dtype]).all()) and bool((h[G + self.n:] == FILL[h.dtype]).all())
        return h[G:G + self.n].numpy()


def _dev(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(DEV)


def _st():
    return torch.cuda.current_stream(DEV).cuda_stream


# ---------------------------------------------------------------------------
# fa_hip_rule_gen
# ---------------------------------------------------------------------------
def run_gen(S, A, cS, cA):
    """(sub, conf, err) of the kernel for level-k rows S over level-(k-1) rows A."""
    S, A = np.asarray(S, dtype=np.int32), np.asarray(A, dtype=np.int32)
    nS, k = S.shape
    assert A.shape == (len(cA), k - 1) and len(cS) == nS
    sub, conf, err = Out(nS * k, torch.int32), Out(nS * k, torch.float64), Out(1, torch.int32)
    err.buf[G] = 0
    d = [_dev(S, np.int32), _dev(A, np.int32), _dev(cS, np.int64), _dev(cA, np.int64)]
    rc = prim._native.hip().fa_hip_rule_gen(d[0].data_ptr(), nS, k, d[1].data_ptr(), len(cA), d[2].data_ptr(),
                                            d[3].data_ptr(), sub.ptr, conf.ptr, err.ptr, _st())
    assert rc == 0
    torch.cuda.synchronize(DEV)
    return sub.get(), conf.get(), int(err.get()[0])


def ref_gen(S, A, cS, cA):
    """The kernel's contract: the row of A equal to S[s] without position p, or -1; conf =
    cS[s] / cA[row] as correctly rounded int / int, 0.0 for a miss; err = k on any miss."""
    k = len(S[0])
    where = {tuple(r): i for i, r in enumerate(np.asarray(A).tolist())}
    assert len(where) == len(A)
    sub, conf = [], []
    for s, row in enumerate(np.asarray(S).tolist()):
        for p in range(k):
            i = where.get(tuple(row[:p] + row[p + 1:]), -1)
            sub.append(i)
            conf.append(int(cS[s]) / int(cA[i]) if i >= 0 else 0.0)
    return np.array(sub, dtype=np.int32), np.array(conf, dtype=np.float64), (k if -1 in sub else 0)


def check_gen(S, A, cS, cA):
    got, want = run_gen(S, A, cS, cA), ref_gen(S, A, cS, cA)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and got[2] == want[2]
    return want


def _rows(rng, n, k, top):
    """n distinct ascending k-rows of ranks below top, sorted."""
    rows = set()
    while len(rows) < n:
        rows.add(tuple(sorted(rng.choice(top, size=k, replace=False).tolist())))
    return sorted(rows)


@pytest.mark.parametrize("k,nS", [(3, 85), (2, 128), (2, 129), (3, 171)])
def test_gen_thread_totals(k, nS):
    # 255, 256, 258 and 513 threads; ranks up to 2^30; every tenth subset row left out of A
    rng = np.random.default_rng(k * 1000 + nS)
    pool = sorted(set(rng.choice(1 << 30, size=18, replace=False).tolist()) | {(1 << 30) - 1, 0})
    S = [tuple(pool[i] for i in r) for r in _rows(rng, nS, k, len(pool))]
    allsub = sorted({r[:p] + r[p + 1:] for r in S for p in range(k)})
    A = [r for i, r in enumerate(allsub) if i % 10 != 3]
    cA = rng.integers(1 << 33, 1 << 34, size=len(A))
    cS = rng.integers(1, 1 << 33, size=nS)
    sub, _, err = check_gen(S, A, cS, cA)
    assert nS * k in (255, 256, 258, 513) and err == k and (sub >= 0).sum() > nS


def test_gen_one_row_below():
    # nA = 1: a hit and a miss per row
    sub, conf, err = check_gen([[5, 9], [5, 10]], [[5]], [3, 1], [4])
    assert sub.tolist() == [-1, 0, -1, 0] and conf.tolist() == [0.0, 0.75, 0.0, 0.25] and err == 2
    assert check_gen([[5, 9]], [[9]], [3], [4])[0].tolist() == [0, -1]


def test_gen_twelve_columns():
    # one row of 12 ranks over its twelve subsets: leaving out p finds row 11 - p
    row = [3, 17, 1 << 10, 1 << 15, 1 << 20, (1 << 20) + 1, 1 << 25, 1 << 28, 1 << 29, (1 << 30) - 2, (1 << 30) - 1,
           1 << 30]
    A = sorted(tuple(row[:p] + row[p + 1:]) for p in range(12))
    sub, _, err = check_gen([row], A, [1 << 40], [(1 << 41) + i for i in range(12)])
    assert sub.tolist() == list(range(11, -1, -1)) and err == 0


def test_gen_search_ends():
    # 1000 rows [7, x], x = 10, 12, .., 2008: only the last column differs
    A = [[7, 10 + 2 * i] for i in range(1000)]
    S = [[3, 7, 10], [3, 7, 2008], [7, 10, 1010], [7, 11, 13], [7, 1010, 1011], [7, 2008, 2009]]
    sub, _, err = check_gen(S, A, [1, 2, 3, 4, 5, 6], np.arange(1000) + 7)
    assert sub.reshape(6, 3).tolist() == [
        [0, -1, -1],           # [7, 10] first row; [3, 10], [3, 7] sort before it
        [999, -1, -1],         # [7, 2008] last row
        [-1, 500, 0],          # [10, 1010] after the last row; [7, 1010] the middle row
        [-1, -1, -1],          # [11, 13] after; [7, 13], [7, 11] between two neighbours
        [-1, -1, 500],         # [7, 1011] between two neighbours
        [-1, -1, 999],         # [7, 2009] after the last row, same first column
    ] and err == 3


def test_gen_counts_are_64_bit_and_the_division_is_exact():
    cA = [3, (1 << 32) + 3, (1 << 33) + 7, (1 << 33) + (1 << 32) + 7]
    _, conf, err = check_gen([[0, 1], [2, 3]], [[0], [1], [2], [3]], [1, (1 << 33) + 7], cA)
    # conf: 1 / cA[1], 1 / cA[0], cS / cA[3], cS / cA[2]
    assert conf[1] == 1 / 3 and conf[0] == 1 / ((1 << 32) + 3) != conf[1]        # differ above bit 32 only
    assert conf[3] == 1.0 and conf[2] == ((1 << 33) + 7) / ((1 << 33) + (1 << 32) + 7) and err == 0


# ---------------------------------------------------------------------------
# fa_hip_rule_cut
# ---------------------------------------------------------------------------
def run_cut(sub, conf, k, kept_prev, conf_prev):
    nS = len(conf) // k
    kept = Out(nS * k, torch.uint8)
    d = [_dev(sub, np.int32), _dev(conf, np.float64), _dev(kept_prev, np.uint8), _dev(conf_prev, np.float64)]
    rc = prim._native.hip().fa_hip_rule_cut(d[0].data_ptr(), d[1].data_ptr(), nS, k, d[2].data_ptr(),
                                            d[3].data_ptr(), kept.ptr, _st())
    assert rc == 0
    torch.cuda.synchronize(DEV)
    return kept.get()


def ref_cut(sub, conf, k, kept_prev, conf_prev):
    """Rule (s, p) survives iff for every other position q the child itemset sub[s][q]
    exists and its rule with the same consequent -- the item at position p of s, which is
    at [j for j != q].index(p) in the child -- was kept with a strictly smaller confidence."""
    nS = len(conf) // k
    kept = np.zeros(nS * k, dtype=np.uint8)
    for s in range(nS):
        for p in range(k):
            ok = True
            for q in range(k):
                if q == p:
                    continue
                child = int(sub[s * k + q])
                if child < 0:
                    ok = False
                    continue
                ci = child * (k - 1) + [j for j in range(k) if j != q].index(p)
                ok = ok and bool(kept_prev[ci]) and bool(conf_prev[ci] < conf[s * k + p])
            kept[s * k + p] = ok
    return kept


@pytest.mark.parametrize("k,nS", [(3, 85), (3, 86), (4, 64), (4, 65), (7, 46), (7, 74)])
def test_cut_positions_and_strictness(k, nS):
    """Every itemset has k children of its own (child s * k + q for position q), so a
    conf_prev entry belongs to one (s, q, position).  Rules have confidence 0.5 over children
    of 0.25: all kept, but for
      * one itemset per ordered pair (p, q): the single entry that rule p reads in child q
        is 0.75, which cuts rule p and no other rule of the itemset;
      * four more: that entry equal to 0.5 (cut), the next double below 0.5 (kept), not
        kept one level down (cut), and child q missing (every rule but q cut);
      * the rest: random values of {0.25, 0.5, 0.75}, random kept flags, a few -1."""
    rng = np.random.default_rng(k * 100 + nS)
    pairs = [(p, q) for p in range(k) for q in range(k) if q != p]
    assert nS >= len(pairs) + 4 and nS * k in (255, 258, 256, 260, 322, 518)
    sub = np.arange(nS * k, dtype=np.int32)
    conf = np.full(nS * k, 0.5)
    conf_prev = np.full(nS * k * (k - 1), 0.25)
    kept_prev = np.ones(nS * k * (k - 1), dtype=np.uint8)

    def entry(s, p, q):
        return (s * k + q) * (k - 1) + p - (q < p)

    want_cut = set()
    for s, (p, q) in enumerate(pairs):
        conf_prev[entry(s, p, q)] = 0.75
        want_cut.add(s * k + p)
    s0 = len(pairs)
    p, q = k - 1, 0
    conf_prev[entry(s0, p, q)] = 0.5
    conf_prev[entry(s0 + 1, p, q)] = np.nextafter(0.5, 0)
    kept_prev[entry(s0 + 2, p, q)] = 0
    sub[(s0 + 3) * k + q] = -1
    want_cut |= {s0 * k + p, (s0 + 2) * k + p} | {(s0 + 3) * k + j for j in range(k) if j != q}
    lo = (s0 + 4) * k
    fill = slice(lo * (k - 1), None)
    conf[lo:] = rng.choice([0.25, 0.5, 0.75], size=nS * k - lo)
    conf_prev[fill] = rng.choice([0.25, 0.5, 0.75], size=conf_prev[fill].size, p=[0.8, 0.1, 0.1])
    kept_prev[fill] = rng.random(kept_prev[fill].size) < 0.95
    sub[lo:][rng.random(nS * k - lo) < 0.03] = -1
    got, want = run_cut(sub, conf, k, kept_prev, conf_prev), ref_cut(sub, conf, k, kept_prev, conf_prev)
    assert set(np.flatnonzero(want[:lo] == 0).tolist()) == want_cut          # the case is what it says
    assert set(np.flatnonzero(got[:lo] == 0).tolist()) == want_cut
    assert np.array_equal(got, want)
    if nS * k > lo + 50:
        assert 0 < int(want[lo:].sum()) < nS * k - lo


# ---------------------------------------------------------------------------
# fa_hip_rule_emit
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("R", [1, 255, 256, 257])
def test_emit(R):
    rng = np.random.default_rng(R)
    n = [0, 5, 1, 7, 3, 9, 4]                                   # rows of the levels of sizes 1..6
    levels = {m: rng.integers(0, 1 << 30, size=(n[m], m), dtype=np.int32) for m in range(1, 7)}
    base = np.zeros(8, dtype=np.int64)                          # base[m]: element offset of the size-m level
    np.cumsum([levels[m].size for m in range(1, 7)], out=base[2:])
    rows_all = np.concatenate([levels[m].reshape(-1) for m in range(1, 7)])
    # the first and the last row of every level, then random rows; sizes in shuffled order
    rules = [(m, i) for m in range(1, 7) for i in (0, n[m] - 1)]
    rules += [(m, int(rng.integers(n[m]))) for m in rng.integers(1, 7, size=max(R - len(rules), 0)).tolist()]
    rules = [rules[i] for i in rng.permutation(len(rules))][:R]
    msz = np.array([m for m, _ in rules], dtype=np.int32)
    idx = np.array([i for _, i in rules], dtype=np.int32)
    ante_off = np.zeros(R + 1, dtype=np.int64)
    np.cumsum(msz, out=ante_off[1:])
    want = np.concatenate([levels[m][i] for m, i in rules])
    ante = Out(int(ante_off[-1]), torch.int32)
    d = [_dev(rows_all, np.int32), _dev(base, np.int64), _dev(msz, np.int32), _dev(idx, np.int32),
         _dev(ante_off, np.int64)]
    rc = prim._native.hip().fa_hip_rule_emit(*[t.data_ptr() for t in d], R, ante.ptr, _st())
    assert rc == 0
    torch.cuda.synchronize(DEV)
    assert np.array_equal(ante.get(), want)
    assert R == 1 or len(set(msz.tolist())) == 6
