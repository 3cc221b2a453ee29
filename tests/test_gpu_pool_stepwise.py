"""The step-wise pool protocol of include/spring_reorder.h (mg_begin -> rounds of mg_search, the caller's own all-gather,
mg_apply -> mg_end), driven the way a caller outside the library drives it: G virtual ranks on one device, each its own
context, the exchange done HERE from what mg_slices reports (never spring_reorder_mg_exchange_virtual, which knows both
chain groups of every rank), the streams merged HERE by the rule the header states from spring_reorder_tid_split's mid[].
Each case runs with the library's proposal buffer (d_prop = NULL) and with one the caller owns; the merged output must equal
one context's run_chains with num_chains = total_chains and the oracle of the schedule that ran (stats.phases), whoever owns
the buffer and whatever G is.  Every 7 rounds the seed-pick invariants of every group's view are checked on every rank.

Device memory for the exchange and the caller-owned buffers comes from the HIP runtime the library itself is bound to
(ctypes), so that no second copy of the runtime enters the process (see spring_amd/pool.py, OneRankComm)."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

from helpers import KEYS, check_invariants
from oracle import pyoracle as po

pytestmark = pytest.mark.gpu

STREAMS = ("order", "rc", "flag", "pos", "rlen")
CHECK_EVERY = 7
HIP_MEMCPY_D2D = 3

# name: (n, L, genome, K, num_thr, options, chain groups that must run)
CASES = {
    # the library's choice at 16 384 chains: two groups, on one GPU as over 2 or 4 ranks
    "k16384_auto_mc": (200_000, 100, 200_000 * 100 // 25, 16384, 3, dict(phases=-1, fused=3, deep_bins=-1), 2),
    "k8192_ph2": (120_000, 150, 120_000 * 150 // 25, 8192, 2, dict(phases=2, fused=0, deep_bins=-1), 2),
    # unequal groups: 4096 + 2048
    "k6144_ph2_mc": (150_000, 100, 150_000 * 100 // 25, 6144, 5, dict(phases=2, fused=3, deep_bins=-1), 2),
    "k20480_auto": (200_000, 150, 200_000 * 150 // 25, 20480, 4, dict(phases=-1, fused=0, deep_bins=-1), 2),
    # not a multiple of 2048: one group on one GPU, and in a pool (its slices would not be whole mark-step blocks)
    "k20000_auto_mc": (200_000, 100, 200_000 * 100 // 25, 20000, 3, dict(phases=-1, fused=3, deep_bins=-1), 1),
    # contended: two candidates per proposal, resolved after the caller's exchange
    "contended_alt2": (40_000, 150, 2_000, 512, 2, dict(phases=1, deep_bins=1, alternatives=2), 1),
}


def _sa():
    import spring_amd
    return spring_amd


@functools.lru_cache(maxsize=1)
def _hip():
    """The HIP runtime the library is bound to (already loaded: RTLD_NOLOAD never maps a second copy)."""
    from spring_amd import _lib
    _lib.lib()
    H = C.CDLL("libamdhip64.so.7", mode=os.RTLD_NOLOAD | os.RTLD_NOW)
    H.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    H.hipFree.argtypes = [C.c_void_p]
    H.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    for f in (H.hipMalloc, H.hipFree, H.hipMemcpy, H.hipDeviceSynchronize):
        f.restype = C.c_int
    return H


def _hchk(rc, what):
    assert rc == 0, "%s failed: hipError %d" % (what, rc)


@functools.lru_cache(maxsize=None)
def _reference(name):
    """One context's run_chains with num_chains = K, and the oracle of the schedule it ran."""
    sa = _sa()
    n, L, gen, K, T, kw, groups = CASES[name]
    with sa.ReorderStage(sa.ReorderOpts(num_chains=K, num_thr=T, **kw)) as st:
        st.load_synth(n, L, gen, 23, 10000)
        single = st.run().streams()
        dna = st.download_dna()
    assert int(single["stats"]["phases"]) == groups and int(single["stats"]["chains"]) == K, (name, single["stats"]["phases"])
    read, ln = po.load_dna(dna, n, L)
    A = kw.get("alternatives", 1)
    oracle = po.reorder_rounds_ph if groups == 2 else po.reorder_rounds
    want = oracle(read, ln, L, K, T, alternatives=A)
    return single, want, read, ln


def _expected_slices(K, G, r, groups):
    """Chain ownership as the header states it, in bytes of the proposal buffer."""
    if groups == 1:
        return [(r * (K // G) * 8, (K // G) * 8)]
    H = max((K // 2 + 1024) // 2048 * 2048, 2048)
    return [(r * (H // G) * 8, (H // G) * 8), ((H + r * ((K - H) // G)) * 8, ((K - H) // G) * 8)]


def _stepwise(name, G, caller_buffer):
    """The protocol over G ranks -> (each rank's streams, chain groups, rounds)."""
    from spring_amd.pool import _MgStage
    from spring_amd.reorder import ReorderError, ReorderOpts
    H = _hip()
    n, L, gen, K, T, kw, groups = CASES[name]
    stages = [_MgStage(ReorderOpts(num_chains=K, num_thr=T, **kw)) for _ in range(G)]
    bufs = []
    try:
        for s in stages:
            s.load_synth(n, L, gen, 23, 10000)
            s.build_dict()
        for r, s in enumerate(stages):
            d = None
            if caller_buffer:
                p = C.c_void_p()
                _hchk(H.hipMalloc(C.byref(p), K * 8), "hipMalloc")
                bufs.append(p.value)
                d = p.value
            s.mg_begin(r, G, K, d)
        ran = [int(s.stats()["phases"]) for s in stages]
        assert ran == [groups] * G, (name, G, caller_buffer, ran)
        layout = [s.mg_slices() for s in stages]
        covered = []
        for r, (ptr, sl, tot) in enumerate(layout):
            assert tot == K * 8
            if caller_buffer:
                assert ptr == bufs[r], "mg_slices must report the caller's buffer"
            assert sl == _expected_slices(K, G, r, groups), (r, sl)
            covered += sl
        covered.sort()
        assert covered[0][0] == 0 and sum(b for _, b in covered) == K * 8
        assert all(a + b == c for (a, b), (c, _) in zip(covered, covered[1:])), "the slices of all ranks must tile the buffer"
        # the one-slice query: the same answer with one group, a refusal that names mg_slices with two
        if groups == 1:
            ptr, off, nb, tot = stages[0].mg_slice()
            assert (ptr, [(off, nb)], tot) == layout[0]
        else:
            with pytest.raises(ReorderError, match="mg_slices"):
                stages[0].mg_slice()
        with pytest.raises(ReorderError):
            stages[0].check_seed_state(groups)
        rounds = 0
        while True:
            for s in stages:
                s.mg_search()
            for d, (dst, _, _) in enumerate(layout):
                for r, (src, sl, _) in enumerate(layout):
                    if r == d:
                        continue
                    for off, nb in sl:
                        _hchk(H.hipMemcpy(dst + off, src + off, nb, HIP_MEMCPY_D2D), "hipMemcpy")
            _hchk(H.hipDeviceSynchronize(), "hipDeviceSynchronize")  # the exchange is complete before any mg_apply
            alive = [s.mg_apply(True) for s in stages]
            rounds += 1
            assert len(set(alive)) == 1, "ranks disagree on the number of running chains after round %d: %r" % (rounds, alive)
            if rounds % CHECK_EVERY == 0:
                for r, s in enumerate(stages):
                    for g in range(groups):
                        assert s.check_seed_state(g) == (0, 0), (name, G, caller_buffer, "rank", r, "group", g, "round", rounds)
            if alive[0] == 0:
                break
        per_rank = []
        for s in stages:
            s.mg_end()
            s.finalize()
            per_rank.append(s.streams())
    finally:
        for s in stages:
            s.close()
        for b in bufs:
            H.hipFree(b)
    return per_rank, groups, rounds


def _merge_by_header_rule(per_rank, T, groups):
    """include/spring_reorder.h (mg_begin): the tid-t stream of the job is every rank's records [tid_off[t], mid[t]), ranks
    ascending, then every rank's records [mid[t], tid_off[t+1]), ranks ascending; likewise the singletons with mid_s."""
    out = {}
    for stream_keys, off_k, mid_k, tid_k in ((STREAMS, "tid_off", "tid_mid", "tid_off"),
                                             (("order_s",), "tid_off_s", "tid_mid_s", "tid_off_s")):
        pieces = {k: [] for k in stream_keys}
        tid_off = [0]
        for r in per_rank:
            off, mid = [int(x) for x in r[off_k]], [int(x) for x in r[mid_k]]
            assert len(off) == T + 1 and len(mid) == T and all(off[t] <= mid[t] <= off[t + 1] for t in range(T))
            if groups == 1:
                assert mid == off[1:], "with one group mid[t] = tid_off[t + 1]"
        for t in range(T):
            size = 0
            for first_part in (True, False):
                for r in per_rank:
                    lo = int(r[off_k][t]) if first_part else int(r[mid_k][t])
                    hi = int(r[mid_k][t]) if first_part else int(r[off_k][t + 1])
                    for k in stream_keys:
                        pieces[k].append(r[k][lo:hi])
                    size += hi - lo
            tid_off.append(tid_off[-1] + size)
        for k in stream_keys:
            out[k] = np.concatenate(pieces[k])
        out[tid_k] = np.array(tid_off, np.uint64)
    return out


def _same(got, want, what):
    for k in KEYS:
        assert np.array_equal(got[k], want[k]), (what, k, len(got[k]), len(want[k]))
    assert np.array_equal(np.asarray(got["tid_off"], np.uint64), np.asarray(want["tid_off"], np.uint64)), (what, "tid_off")
    assert np.array_equal(np.asarray(got["tid_off_s"], np.uint64), np.asarray(want["tid_off_s"], np.uint64)), (what, "tid_off_s")


@pytest.mark.parametrize("G", [1, 2, 4])
@pytest.mark.parametrize("name", list(CASES))
def test_stepwise_pool_equals_one_context_and_oracle(name, G):
    """Merged streams, per-tid offsets and lost / unmatched over the ranks == one context == the oracle of the schedule
    that ran, with the library's proposal buffer and with the caller's."""
    n, L, gen, K, T, kw, groups = CASES[name]
    single, want, read, ln = _reference(name)
    _same(single, want, (name, "one context vs oracle"))
    for caller_buffer in (False, True):
        what = (name, G, "caller's buffer" if caller_buffer else "library's buffer")
        per_rank, ran, rounds = _stepwise(name, G, caller_buffer)
        assert ran == groups and rounds > 0
        got = _merge_by_header_rule(per_rank, T, groups)
        _same(got, want, what + ("vs oracle",))
        _same(got, single, what + ("vs run_chains",))
        for k in ("lost", "unmatched"):
            total = sum(int(r["stats"][k]) for r in per_rank)
            assert total == int(want["stats"][k]) == int(single["stats"][k]), (what, k, total, want["stats"][k])
        check_invariants(got, read, ln, L, n)
