"""What the four-chain round kernel no longer loads of a chain's own state: the verdict on its proposal
arrives in its class-list entry from the mark step instead of being read from resv[], the reverse consensus is rebuilt
from the forward one instead of being kept in the chain record, and a chain that picks a seed loads its header only.
None of it may change a result: streams and per-tid offsets bit-exact against the CPU oracle, through reorder_dna with
fused = 3, deep_bins = -1 (k_round_mc) -- on pools where many proposals lose, with two chain groups (a claim by the other
group must arrive as "lost"), over two virtual ranks (k_mg_mark's list), and at the read lengths where the number of
limbs changes and the consensus ends inside a limb."""
import functools

import numpy as np
import pytest

import readsets as rs
from helpers import KEYS, named_set
from oracle import pyoracle as po

pytestmark = pytest.mark.gpu


def _sa():
    import spring_amd
    return spring_amd


def _same(a, b, what):
    for k in KEYS + ("tid_off", "tid_off_s"):
        assert np.array_equal(a[k], b[k]), (what, k, len(a[k]), len(b[k]))


@functools.lru_cache(maxsize=None)
def _named(name):
    dna, n, L = named_set(name)
    read, ln = po.load_dna(dna, n, L)
    return dna, n, L, read, ln


@functools.lru_cache(maxsize=None)
def _want_named(name, K, T):
    _, _, L, read, ln = _named(name)
    return po.reorder_serial(read, ln, L) if K == 1 else po.reorder_rounds(read, ln, L, K, T)


def _run(dna, n, L, K, T, **kw):
    sa = _sa()
    kw.setdefault("fused", 3)
    kw.setdefault("deep_bins", -1)
    return sa.reorder_dna(dna, n, L, sa.ReorderOpts(num_chains=K, num_thr=T, **kw))


@pytest.mark.parametrize("name", ["dups", "heavy", "repeat10k", "syn2k_20"])
@pytest.mark.parametrize("K,T", [(1, 1), (32, 2), (300, 3)])
def test_lost_proposals(name, K, T):
    """Contended pools: many chains propose the same read, seeds included, and all but one of them lose.  At 300 chains
    the loser path must really have been taken."""
    dna, n, L, _, _ = _named(name)
    got = _run(dna, n, L, K, T)
    _same(got, _want_named(name, K, T), (name, K))
    print("lost proposals", name, K, got["stats"]["lost"])
    if K == 300:
        assert got["stats"]["lost"] > 0, (name, K)
    if K == 1:
        assert got["stats"]["lost"] == 0, (name, K)


def test_two_chain_groups():
    """The two-group schedule at its smallest legal shape (4 096 chains): the mark step overrules a chain that holds its
    reservation when the other group has taken the read, and the chain must hear of it through the list."""
    sa = _sa()
    n, L = 20000, 100
    dna = sa.synth_dna_host(n, L, n * L // 25, 1, 10000)
    read, ln = po.load_dna(dna, n, L)
    want = po.reorder_rounds_ph(read, ln, L, 4096, 2)
    for ka in (0, -1):
        got = _run(dna, n, L, 4096, 2, phases=2, known_absent=ka)
        _same(got, want, ("phases", ka))
        assert got["stats"]["phases"] == 2
        assert got["stats"]["lost"] > 0


def test_virtual_ranks():
    """One pool over two virtual ranks (k_round_mc<.., MG = true, ..>: the list comes from k_mg_mark) against one context."""
    from spring_amd.pool import VirtualPool
    name, K, T = "syn5k_150", 64, 3
    dna, n, L, _, _ = _named(name)
    single = _run(dna, n, L, K, T)
    _same(single, _want_named(name, K, T), "single")
    vp = VirtualPool(2, K, T, fused=3, deep_bins=-1)
    try:
        got = vp.run(lambda s: s.load_dna(dna, n, L))
    finally:
        vp.close()
    for k in KEYS:
        assert np.array_equal(got[k], single[k]), ("pool", k)


@functools.lru_cache(maxsize=None)
def _length_pool(L, var):
    n = 3000
    a = rs.np_reads(700 + L, n * L // 25, n, L, 0.01)
    if var:  # the same reads cut to random lengths: the consensus length is rarely a multiple of 32
        rng = np.random.default_rng(L)
        cut = [bytes(r[:int(k)]) for r, k in zip(a, rng.integers(L // 2, L + 1, n))]
        cut[0] = bytes(a[0])  # (the pool's maximum read length stays L)
        dna = rs.pack_var(cut)
    else:
        dna = rs.pack_fixed(a)
    read, ln = po.load_dna(dna, n, L)
    return dna, n, po.reorder_rounds(read, ln, L, 48, 2)


@pytest.mark.parametrize("var", [False, True], ids=["fixed", "cut"])
@pytest.mark.parametrize("L", [101, 127, 128, 129, 160, 191, 192])
def test_read_lengths(L, var):
    """The lengths at which the number of limbs changes (128 | 129, 160 | 161, 192) and the rebuilt reverse consensus has a
    partial top limb; with the masks and without, with the presence-table sweep and without."""
    dna, n, want = _length_pool(L, var)
    for ka in (0, -1):
        for sf in (0, -1):
            got = _run(dna, n, L, 48, 2, known_absent=ka, strand_filter=sf)
            _same(got, want, (L, var, ka, sf))
