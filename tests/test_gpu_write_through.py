"""Per-round state is stored write-through: the count columns, the chain record (header, consensus,
known-absent masks), the emission records and chunk tags, the proposal words and the mark step's lists leave the L2 as
they are made instead of at the end of the kernel.  Only the flavour of the stores changed, so nothing may change in a
result: streams and per-tid offsets bit-exact against the CPU oracle, one case per store path at the smallest shape that
reaches it -- the kernel variants pinned by the options test_gpu_chain_state.py and test_gpu_parity.py use (fused = 3,
deep_bins = -1: k_round_mc; deep_bins = 1: the one-chain deep-bin kernels with k_long)."""
import functools

import numpy as np
import pytest

import readsets as rs
from helpers import KEYS, named_set
from oracle import pyoracle as po

pytestmark = pytest.mark.gpu

MC = dict(fused=3, deep_bins=-1)


def _sa():
    import spring_amd
    return spring_amd


def _same(a, b, what):
    for k in KEYS + ("tid_off", "tid_off_s"):
        assert np.array_equal(a[k], b[k]), (what, k, len(a[k]), len(b[k]))


def _run(dna, n, L, K, T, **kw):
    sa = _sa()
    return sa.reorder_dna(dna, n, L, sa.ReorderOpts(num_chains=K, num_thr=T, **kw))


@functools.lru_cache(maxsize=None)
def _two_group_pool():
    sa = _sa()
    n, L = 20000, 100
    dna = sa.synth_dna_host(n, L, n * L // 25, 1, 10000)
    read, ln = po.load_dna(dna, n, L)
    return dna, n, L, po.reorder_rounds_ph(read, ln, L, 4096, 2)


@pytest.mark.parametrize("ka", [0, -1], ids=["masks", "no_masks"])
def test_two_chain_groups(ka):
    """Two chain groups at the smallest legal shape (4 096 chains): the count quads, the header (stored twice in a round), the
    mask line, the verdict list and won[] of k_ph_mark_wide, all read by the NEXT launch -- of this group or of the other."""
    dna, n, L, want = _two_group_pool()
    got = _run(dna, n, L, 4096, 2, phases=2, known_absent=ka, **MC)
    _same(got, want, ("phases", ka))
    assert got["stats"]["phases"] == 2
    assert got["stats"]["lost"] > 0  # (verdicts travelled through the list)


def test_wide_count_format():
    """Four chains on a 300-base genome: every chain merges more than 255 reads over the same positions, so the columns go
    over to the int4 format (the generic path's 16-byte stores) and, after a new seed, back to bytes.
    Why it must: 6 000 x 100 bases over 300 bases put 2 000 reads on every base of the genome, about 500 per chain; a column
    keeps a base's counts for as long as the base lies under the consensus, and a contig ends only when a search fails in
    both directions, so the count of the consensus base passes 255 (a byte) wherever a chain merges more than half of its
    share in one contig.  The library keeps no counter of format changes, so the case asserts the result only."""
    sa = _sa()
    n, L, K = 6000, 100, 4
    dna = sa.synth_dna_host(n, L, 300, 5, 10000)
    read, ln = po.load_dna(dna, n, L)
    want = po.reorder_rounds(read, ln, L, K, 2)
    got = _run(dna, n, L, K, 2, **MC)
    _same(got, want, "wide counts")
    assert got["stats"]["lost"] >= 0


@functools.lru_cache(maxsize=None)
def _length_pool(kind):
    n = 2000
    if kind == "L250":  # k_round_mc_long: eight position quads per lane
        L = 250
        dna = rs.pack_fixed(rs.np_reads(250, n * L // 25, n, L, 0.01))
    elif kind == "var60_150":  # uniform_len off: the read length is loaded per update
        L = 150
        reads = rs.var_length_reads(60150, n * 105 // 25, n, 60, 150, 0.01)
        reads[0] = reads[0] + b"A" * (L - len(reads[0]))  # (the pool's maximum read length is L)
        dna = rs.pack_var(reads)
    else:  # L = 64: a window shorter than 32 bases
        L = 64
        dna = rs.pack_fixed(rs.np_reads(64, n * L // 25, n, L, 0.01))
    read, ln = po.load_dna(dna, n, L)
    return dna, n, L, po.reorder_rounds(read, ln, L, 48, 2)


@pytest.mark.parametrize("kind", ["L250", "var60_150", "L64"])
def test_long_and_variable_reads(kind):
    dna, n, L, want = _length_pool(kind)
    _same(_run(dna, n, L, 48, 2, **MC), want, kind)


@functools.lru_cache(maxsize=None)
def _phix_like():
    sa = _sa()
    n, L = 40000, 150
    dna = sa.synth_dna_host(n, L, 5400, 9, 10000)
    read, ln = po.load_dna(dna, n, L)
    return dna, n, L, read, ln


@pytest.mark.parametrize("alts", [-1, 2], ids=["defaults", "two_candidates"])
def test_one_chain_deep_bin_kernels(alts):
    """A PhiX-like pool (1 100x) at the library's defaults (its chain count, its choice of candidates per proposal) and with
    two candidates per proposal: the one-chain round kernels' stores (wave_update_compute, pack_consensus, store_hot,
    emit_rec) and the proposal words k_long_fin writes."""
    sa = _sa()
    dna, n, L, read, ln = _phix_like()
    T = 2
    with sa.ReorderStage(sa.ReorderOpts(num_chains=0, num_thr=T, alternatives=alts)) as s:
        s.load_dna(dna, n, L)
        s.build_dict()
        K, deep = s.auto_chains()
        s.run_chains()
        s.finalize()
        got = s.streams()
    assert deep
    A = got["stats"]["alternatives"]
    assert alts < 0 or A == alts
    want = po.reorder_rounds(read, ln, L, K, T, alternatives=A) if A == 2 else po.reorder_rounds(read, ln, L, K, T)
    _same(got, want, ("phix-like", alts, K, A))


def test_two_virtual_ranks():
    """One pool over two virtual ranks: k_mg_mark's needy bitmap and class lists, the proposal words through the exchange."""
    from spring_amd.pool import VirtualPool
    name, K, T = "syn2k_20", 64, 3
    dna, n, L = named_set(name)
    read, ln = po.load_dna(dna, n, L)
    want = po.reorder_rounds(read, ln, L, K, T)
    vp = VirtualPool(2, K, T, **MC)
    try:
        got = vp.run(lambda s: s.load_dna(dna, n, L))
    finally:
        vp.close()
    _same(got, want, "pool")
