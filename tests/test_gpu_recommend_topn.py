"""Ranked top-N on the device: recommend_topn_shard with both kernels (k_recommend_topn and
k_recommend_topn_indexed) against the C++ path, on a mined rule table."""
import functools

import pytest
import torch

from fastapriori_amd.models.apriori import FastApriori, MinerConfig
from fastapriori_amd.models.rules import AssociationRules
from fastapriori_amd.ops import primitives as prim
from fastapriori_amd.parallel.comm import Comm
from fastapriori_amd.utils.io import generate_shard

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)


@functools.lru_cache(maxsize=None)
def _case():
    """The data of test_gpu_kernels.test_recommend_kernel: (mined result, users, CPU rules)."""
    sh = generate_shard(20000, Comm(), "cpu", 8.0, 3.0, 80, 100, seed=9)
    res = FastApriori(0.01, config=MinerConfig(min_support=0.01)).run(sh)
    users = generate_shard(3000, Comm(), "cpu", 8.0, 3.0, 80, 100, seed=9, users=True)
    return res, users, AssociationRules(res)


@functools.lru_cache(maxsize=None)
def _ref(n):
    _, users, ar = _case()
    return ar.recommend_topn_shard(users, n)


@pytest.mark.parametrize("indexed", [False, True], ids=["scan", "indexed"])
@pytest.mark.parametrize("n", [1, 3, 10])
def test_topn_shard_matches_cpu(monkeypatch, n, indexed):
    res, users, ar = _case()
    ref = _ref(n)
    assert tuple(ref.shape) == (users.n_lines, n) and (ref[:, 0] >= 0).any() and (ref[:, n - 1] < 0).any()
    if n > 1:
        assert (ref[:, n - 1] >= 0).any()            # full lists, too
    monkeypatch.setattr(prim, "RECOMMEND_INDEX_MIN_RULES", 1)
    calls = []
    for name in ("fa_hip_recommend_topn", "fa_hip_recommend_topn_indexed"):
        fn = getattr(prim._native.hip(), name)
        monkeypatch.setattr(prim._native.hip(), name,
                            lambda *a, _fn=fn, _name=name: calls.append(_name) or _fn(*a))
    dev = AssociationRules(res, device="cpu")            # the same (host-built) rule table
    dev.use_index = indexed
    prim.reset_fallbacks()
    got = dev.recommend_topn_shard(users.to(DEV), n)
    assert got.device.type == "cuda" and got.dtype == torch.int32
    assert torch.equal(got.cpu(), ref)
    assert not prim.FALLBACKS
    assert calls == ["fa_hip_recommend_topn_indexed" if indexed else "fa_hip_recommend_topn"]
    # column 0 is the rule behind the first-match recommendation
    first = dev.recommend_shard(users.to(DEV)).cpu()
    cons = torch.from_numpy(ar.rules().cons)
    col0 = ref[:, 0].to(torch.int64)
    assert torch.equal(torch.where(col0 >= 0, cons[col0.clamp(min=0)], torch.full_like(cons[:1], -1)), first)


def test_run_topn_on_device_equals_cpu_lines():
    res, users, ar = _case()
    dev = AssociationRules(res, device=DEV)              # rules built by the device, too
    got = dev.run_topn(users.to(DEV), 5, scores=True)
    assert got == ar.run_topn(users, 5, scores=True)
    assert "fallbacks" not in dev.stats
