"""hgibbs_cs_select (hg_csselect.cpp, host only) against the walk of tests/cs_restate.py on random candidates: overlapping member
lists, ties in the leads' counts, the three statuses, PEP counts on both sides of the bound and on it; the walk's two properties; the
refusals.  No GPU needed."""
import ctypes as C

import numpy as np
import pytest

import cs_restate as cr
from hydra_amd import capi

M = 400


def random_candidates(nlead, max_size, seed, min_pep):
    """leads from a narrow range of markers (so the member lists overlap), counts from a handful of values (so they tie)"""
    rng = np.random.default_rng(seed)
    leads = rng.choice(M, size=nlead, replace=False).astype(np.uint32)
    lead_cnt = rng.integers(1, 6, nlead).astype(np.uint32)
    status = rng.choice([0, 0, 0, 1, 2], nlead).astype(np.uint32)
    size = np.where(status == 0, rng.integers(1, max_size + 1, nlead), 0).astype(np.uint32)
    pep = np.where(status == 0, min_pep + rng.integers(-2, 3, nlead), 0).astype(np.uint32)
    members = np.full((nlead, max_size), cr.NONE, dtype=np.uint32)
    for i in range(nlead):
        if size[i]:
            near = np.arange(max(0, int(leads[i]) - 80), min(M, int(leads[i]) + 81))
            near = near[near != leads[i]]
            members[i, 0] = leads[i]
            members[i, 1:size[i]] = rng.choice(near, size=int(size[i]) - 1, replace=False)
    return leads, lead_cnt, status, size, pep, members


@pytest.mark.parametrize("max_size", [1, 3, 64])
@pytest.mark.parametrize("nlead", [0, 1, 2, 65, 300])
def test_against_the_restatement(nlead, max_size):
    min_pep = 10
    seen = set()
    for seed in range(4):
        leads, lead_cnt, status, size, pep, members = random_candidates(nlead, max_size, 1000 * nlead + 10 * max_size + seed, min_pep)
        got = capi.cs_select(M, leads, lead_cnt, status, size, pep, members, max_size, min_pep)
        want = cr.walk(leads, lead_cnt, status, size, pep, members, min_pep)
        assert got.tolist() == want
        # the properties: accepted sets are disjoint; a rejected candidate that reached its sum and the PEP bound shares a member with
        # an accepted one that comes earlier in the walk
        rank = {i: k for k, i in enumerate(sorted(range(nlead), key=lambda i: (-int(lead_cnt[i]), int(leads[i]))))}
        sets = {i: set(members[i, :size[i]].tolist()) for i in range(nlead)}
        owned = set()
        for i in got.tolist():
            assert status[i] == 0 and pep[i] >= min_pep and not (sets[i] & owned)
            owned |= sets[i]
        for i in range(nlead):
            if i in got.tolist():
                continue
            if status[i] == 0 and pep[i] >= min_pep:
                assert any(rank[a] < rank[i] and sets[a] & sets[i] for a in got.tolist()), i
                seen.add("overlap")
            elif status[i] == 0:
                seen.add("low" if pep[i] < min_pep - 1 else "just below")
        seen |= {"on the bound"} if np.any((status == 0) & (pep == min_pep)) else set()
        seen |= {"ties"} if len(set(lead_cnt.tolist())) < nlead else set()
    if nlead >= 65:
        assert seen >= {"low", "just below", "on the bound", "ties"} and (max_size == 1 or "overlap" in seen), seen


def test_the_order_is_count_then_index():
    leads = np.array([9, 3, 7, 1], dtype=np.uint32)
    lead_cnt = np.array([2, 5, 5, 2], dtype=np.uint32)
    one = np.ones(4, dtype=np.uint32)
    got = capi.cs_select(10, leads, lead_cnt, 0 * one, one, 3 * one, leads.reshape(4, 1), 1, 3)
    assert got.tolist() == [1, 2, 3, 0]


def test_refusals():
    L = capi.lib()
    u32 = lambda *v: (C.c_uint32 * max(len(v), 1))(*v)  # noqa: E731
    nt = C.c_uint32(7)

    def refused(msg, M=10, nlead=1, leads=u32(1), cnt=u32(1), status=u32(0), size=u32(1), pep=u32(1), members=u32(1, 2), max_size=2, taken=u32(0), ntaken=C.byref(nt)):
        assert L.hgibbs_cs_select(M, nlead, leads, cnt, status, size, pep, members, max_size, 1, taken, ntaken) != 0
        assert msg in L.hgibbs_last_error().decode(), L.hgibbs_last_error().decode()

    refused("hgibbs_cs_select: null output (ntaken)", ntaken=None)
    for name in ("leads", "cnt", "status", "size", "pep", "members"):
        refused("hgibbs_cs_select: null input with nlead = 1", **{name: None})
    refused("hgibbs_cs_select: null output (taken)", taken=None)
    refused("hgibbs_cs_select: max_size = 0, must be in [1, 256]", max_size=0)
    refused("hgibbs_cs_select: max_size = 257, must be in [1, 256]", max_size=257)
    refused("hgibbs_cs_select: candidate 0 has size 3, above max_size = 2", size=u32(3))
    refused("hgibbs_cs_select: candidate 0: member 1 is marker 10, not below M = 10", size=u32(2), members=u32(1, 10))
    assert nt.value == 0
    # a member outside a size is not looked at; no candidate at all needs no array
    assert L.hgibbs_cs_select(10, 1, u32(1), u32(1), u32(0), u32(1), u32(1), u32(1, 0xFFFFFFFF), 2, 1, u32(0), C.byref(nt)) == 0 and nt.value == 1
    assert L.hgibbs_cs_select(10, 0, None, None, None, None, None, None, 2, 1, None, C.byref(nt)) == 0 and nt.value == 0
