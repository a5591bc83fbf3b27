"""The device piece plan, counted (csrc/hip/levels.hip: k_dl_map, k_dl_pieces_count / scan /
emit, k_dl_lane_assign; counted by k_count_slab_rec).

The plan is otherwise reached only through whole mining runs compared with the host loop.
Here a device bundle is generated from rows built on purpose (tests/test_gen_edges.py,
section 3), planned with ops.primitives.dl_plan and counted with dl_count over a small dense
0/1 matrix B[T, F1]; every candidate's count must equal the number of rows of B that hold it,
computed from B in numpy.  The cases reach pieces of 8 extensions and every remainder, parent
rows cut into two and three pieces, the 256-parent-row planner blocks, prefixes past the 12
ids a piece record holds (written to gpre) up to the longest the loop takes (40), the rank
map over all 512 bitset words, and the lane deal.
"""
import functools

import numpy as np
import pytest

from fastapriori_amd.ops import _native
from fastapriori_amd.ops import primitives as prim
from test_gen_edges import DEV, bundle_case, accepted, check_bundle, run_bundle, _placed
from test_kernel_edges import _csr

# id: (bundle case, max_levels, growth, T of B, parent rows R of the accepted levels)
PLAN_CASES = {
    "lat20_T1":       ("lat20_F70", 2, 5.0, 1, 190 + 1140),
    "lat20_T64":      ("lat20_F70", 2, 5.0, 64, 190 + 1140),
    "lat20_T65":      ("lat20_F70", 2, 5.0, 65, 190 + 1140),
    "lat20_T200":     ("lat20_F70", 2, 5.0, 200, 190 + 1140),
    "R255":           ("lat24_F70_del21", 1, 1.0, 65, 255),
    "R256":           ("lat24_F70_del20", 1, 1.0, 65, 256),
    "R257":           ("lat24_F70_del19", 1, 1.0, 65, 257),
    "R528":           ("lat33_F70", 1, 1.0, 64, 528),
    "m11_gpre":       ("lat15_F70_m11", 4, 3.0, 65, 1365 + 455 + 105 + 15),
    "m39_m40":        ("lat42_F70_m39", 2, 3.0, 200, 11480 + 861),
    "lat13_deep":     ("lat13_F70", 31, 3.0, 200, 8177),
    "cliques":        ("cliques_s3", 31, 8.0, 200, None),
    "F32768":         ("lat12_F32768", 2, 3.0, 65, 66 + 220),
    "lane_deal":      ("lat40_F70", 1, 1.0, 200, 780),
}


@functools.lru_cache(maxsize=None)
def _plan_case(case):
    """-> (F1, chain, accepted levels L, B int8 [T, F1], supports: per level int64 [C_l])."""
    name, max_levels, growth, T, R = PLAN_CASES[case]
    F1, ch = bundle_case(name, max_levels if max_levels < 31 else 64)
    L, empty = accepted(ch, max_levels, growth)
    assert L == (max_levels if max_levels < 31 else len(ch) - 1) and empty == (max_levels == 31)
    if R is not None:
        assert sum(len(r) for r, _, _ in ch[:L]) == R
    # B as test_kernel_edges._slab_rows makes it: random rows, a planted share of rows that
    # hold every item of the bundle (deep candidates have support), >= 2 items in every row
    rng = np.random.default_rng(1000 + sorted(PLAN_CASES).index(case))
    B = (rng.random((T, F1)) < 0.3).astype(np.int8)
    B[np.ix_(np.arange(T) % 10 < 3, np.unique(ch[0][0]))] = 1
    B[B.sum(1) < 2, :2] = 1
    has = B.astype(bool)
    sup = [has[:, cand].all(2).sum(0).astype(np.int64) for _, _, cand in ch[:L]]
    assert all(s.shape == (len(c),) for s, (_, _, c) in zip(sup, ch)) and sup[L - 1].max() >= min(T, 3) // 3
    per = np.concatenate([cnt for _, cnt, _ in ch[:L]])          # extensions per parent row
    if name == "lat20_F70":
        # every piece size, and rows of one, two and three pieces
        assert set(per.tolist()) == set(range(19)) and {0, 1, 2} == set((per // 8).tolist())
    if case == "m11_gpre":
        assert [r.shape[1] for r, _, _ in ch[:L]] == [11, 12, 13, 14] and prim.dl().kDlInline == 12
    if case == "m39_m40":
        assert [r.shape[1] for r, _, _ in ch[:L]] == [39, 40] and prim.dl().kDlMaxM == 40
    if case == "F32768":
        assert set(_placed(F1, 12)) == set(np.unique(ch[0][0]).tolist()) and F1 == 64 * prim.dl().kDlBitsW
    if case == "lane_deal":
        # the pieces of 8 come first, level 0's first: its first 256 records share n_ext = 8
        # and m = 2, one whole window of k_dl_lane_assign (by the reference's counts)
        assert int((ch[0][1] // 8).sum()) >= 3 * 256
    return F1, ch, L, B, sup


def test_plan_references(native):
    for case in PLAN_CASES:
        _plan_case(case)
    Rs = [PLAN_CASES[c][4] for c in ("R255", "R256", "R257", "R528")]
    assert Rs == [255, 256, 257, 528]             # around one planner block (kDlPB = 256), and past two


@pytest.fixture(scope="module")
def dl_state():
    return prim.DeviceLevelState(DEV)


@pytest.mark.gpu
@pytest.mark.parametrize("case", list(PLAN_CASES))
def test_plan_counts(dl_state, tune, case):
    name, max_levels, growth, T, _ = PLAN_CASES[case]
    F1, ch, L, B, sup = _plan_case(case)
    S, K = dl_state, prim.dl()
    c, P0 = run_bundle(S, F1, ch, max_levels, growth)
    check_bundle(S, c, F1, ch, L, empty=max_levels == 31)
    C = int(sum(len(cand) for _, _, cand in ch[:L]))
    gneed = int(_native.hip().fa_hip_dl_gpre_need(S.desc.ctypes.data, L))
    assert gneed == sum(r.size for r, _, _ in ch[:L] if r.shape[1] > K.kDlInline)
    assert (gneed > 0) == (case in ("m11_gpre", "m39_m40"))
    roff, ranks = _csr(B.astype(np.int64))
    roff, ranks = roff.to(DEV), ranks.to(DEV)
    if case == "lane_deal":
        tune(lane_deal_min_rows=0)
    S.rows_hint = T if case == "lane_deal" else 0
    try:
        plan = prim.dl_plan(S, L, F1, int(c[K.kDlNUsed]), C, prim.dl_lds_budget(F1), DEV)
        got = prim.dl_count(S, plan, roff, ranks, None, T, F1, None)
        got = got.cpu().numpy()
        pieces = int(S.ctl[K.kDlPieces].item())
    finally:
        S.rows_hint = 0
    per = np.concatenate([cnt for _, cnt, _ in ch[:L]])
    assert pieces == int(((per + 7) // 8).sum())
    assert got.dtype == np.int32 and got.shape == (C,)
    base = 0
    for l in range(L):
        assert np.array_equal(got[base:base + len(sup[l])], sup[l]), l
        base += len(sup[l])
    del P0
