"""The strand-symmetric presence table of the four-chain round kernel (opts.strand_filter): a chain
whose seed has no match yet sweeps the windows of its consensus through a small probe-only table of canonical windows
before it searches, and every absence the table proves goes into the chain's known-absent masks for both strands.  The
table can only say "absent", so the bar is the one of the masks themselves: bit-exact against the CPU oracle with the
option at its default, switched off, and with a table so small that nearly every lookup answers "unknown"."""
import functools

import numpy as np
import pytest

import readsets as rs
from helpers import KEYS, named_set
from oracle import pyoracle as po

pytestmark = pytest.mark.gpu

_ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)


def _sa():
    import spring_amd
    return spring_amd


def _same(a, b, what):
    for k in KEYS:
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


def _run(dna, n, L, K, T, sf, **kw):
    sa = _sa()
    kw.setdefault("fused", 3)
    kw.setdefault("deep_bins", -1)
    return sa.reorder_dna(dna, n, L, sa.ReorderOpts(num_chains=K, num_thr=T, strand_filter=sf, **kw))


NAMES = ["syn5k_150", "syn2k_100", "syn3k_64", "syn2k_20", "var2k", "var_short", "heavy", "tandem", "repeat10k", "dups", "test_1+2"]


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("K,T", [(1, 1), (32, 2), (300, 3)])
def test_named_sets(name, K, T):
    """Fixed and variable lengths, windows of 32, 20 and 6 bases (6: palindromes and saturated buckets come by themselves),
    contended pools, lone seeds that turn round: the same streams as the oracle with the sweep and without."""
    dna, n, L, _, _ = _named(name)
    want = _want_named(name, K, T)
    for sf in (0, -1):
        got = _run(dna, n, L, K, T, sf)
        _same(got, want, (name, K, sf))
        if sf < 0:
            assert got["stats"]["strand_filter"] == 0 and got["stats"]["strand_filter_dropped"] == 0
        else:  # every one of these pools has reads of at most 192 bases and adjacent, equally long dictionary windows: the sweep runs
            assert L <= 192 and got["stats"]["strand_filter"] == 1, (name, L)


@pytest.mark.parametrize("name", ["syn5k_150", "syn3k_64", "var2k"])
@pytest.mark.parametrize("K,T", [(1, 1), (32, 2), (300, 3)])
def test_capped_table(name, K, T):
    """16 buckets for thousands of keys: every bucket is full, keys are dropped, nearly all lookups answer "unknown" --
    and the few that answer at all still only ever say "absent" where it is true."""
    dna, n, L, _, _ = _named(name)
    want = _want_named(name, K, T)
    got = _run(dna, n, L, K, T, 4)
    _same(got, want, (name, K, "capped"))
    assert got["stats"]["strand_filter"] == 1
    assert got["stats"]["strand_filter_dropped"] > 0


def _rc(a):
    return (3 - a)[..., ::-1]


def _palindrome_pool(L, seed):
    """~2 000 reads (codes A0 C1 G2 T3, complement 3 - x): a 25x background; reads whose dictionary-0 / dictionary-1 window
    is a reverse palindrome (W == rc(W)), alone and in small groups that share it; pairs where one read carries W as its
    dictionary-0 key and another rc(W) as its dictionary-1 key; and pairs from fresh sequence where the only read that
    overlaps a read lies on the other strand."""
    rng = np.random.default_rng(seed)
    (s0, s1), (e0, _) = po.dict_windows(L)
    wl = e0 - s0 + 1
    assert wl % 2 == 0
    parts = []
    n_bg = 1200
    g = rng.integers(0, 4, n_bg * L // 25, dtype=np.uint8)
    pos = rng.integers(0, len(g) - L + 1, n_bg)
    bg = g[pos[:, None] + np.arange(L)[None, :]]
    e = rng.random((n_bg, L)) < 0.01
    bg = np.where(e, (bg + rng.integers(1, 4, (n_bg, L), dtype=np.uint8)) % 4, bg).astype(np.uint8)
    flip = rng.random(n_bg) < 0.5
    bg[flip] = _rc(bg[flip])
    parts.append(bg)
    # palindromic windows: x + rc(x)
    for start, count in ((s0, 120), (s1, 120)):
        r = rng.integers(0, 4, (count, L), dtype=np.uint8)
        x = rng.integers(0, 4, (count // 3, wl // 2), dtype=np.uint8)
        pal = np.concatenate([x, _rc(x)], axis=1)
        r[:, start:start + wl] = pal[np.arange(count) % len(pal)]  # every palindrome in three otherwise unrelated reads
        parts.append(r)
    # a palindromic window inside reads that do overlap: a locus with a palindrome, covered on both strands
    loc = rng.integers(0, 4, (30, L + 40), dtype=np.uint8)
    x = rng.integers(0, 4, (30, wl // 2), dtype=np.uint8)
    loc[:, s0 + 20:s0 + 20 + wl] = np.concatenate([x, _rc(x)], axis=1)
    for sh in (20, 14, 27, 20 - (s1 - s0)):
        if 0 <= sh <= 40:
            r = loc[:, sh:sh + L].copy()
            parts.append(r if sh % 2 == 0 else _rc(r))
    # W as a dictionary-0 key here, rc(W) as a dictionary-1 key there
    w = rng.integers(0, 4, (150, wl), dtype=np.uint8)
    a = rng.integers(0, 4, (150, L), dtype=np.uint8)
    b = rng.integers(0, 4, (150, L), dtype=np.uint8)
    a[:, s0:s0 + wl] = w
    b[:, s1:s1 + wl] = _rc(w)
    parts += [a, b]
    # lone seeds whose only partner sits on the other strand
    seg = rng.integers(0, 4, (150, L + 12), dtype=np.uint8)
    off = rng.integers(1, 13, 150)
    parts.append(seg[:, :L].copy())
    parts.append(_rc(np.stack([seg[i, o:o + L] for i, o in enumerate(off)])))
    reads = np.concatenate(parts).astype(np.uint8)
    rng.shuffle(reads, axis=0)
    win0 = reads[:, s0:s0 + wl]
    assert int(np.all(win0 == _rc(win0), axis=1).sum()) >= 100  # the pool does hold palindromic dictionary windows
    return _ACGT[reads]


@pytest.mark.parametrize("L", [150, 64])
def test_palindromes_and_cross_strand_keys(L):
    a = _palindrome_pool(L, 900 + L)
    n = a.shape[0]
    dna = rs.pack_fixed(a)
    read, ln = po.load_dna(dna, n, L)
    want = po.reorder_rounds(read, ln, L, 48, 2)
    for sf in (0, -1, 4):
        got = _run(dna, n, L, 48, 2, sf)
        _same(got, want, (L, sf))
        assert got["stats"]["strand_filter"] == (0 if sf < 0 else 1)


@pytest.mark.parametrize("L", [101, 127, 128, 160, 191, 192])
def test_read_lengths(L):
    """The lengths where the masks' place in the chain record moves and the longest reads the kernel takes; with the same
    reads cut to random lengths the consensus length differs from L, so the mirrored offset ref_len - wl - o moves."""
    n = 4000
    a = rs.np_reads(500 + L, n * L // 25, n, L, 0.01)
    rng = np.random.default_rng(L)
    cut = [bytes(r[:int(k)]) for r, k in zip(a, rng.integers(L // 2, L + 1, n))]
    cut[0] = bytes(a[0])  # (the pool's maximum read length stays L)
    for dna in (rs.pack_fixed(a), rs.pack_var(cut)):
        read, ln = po.load_dna(dna, n, L)
        want = po.reorder_rounds(read, ln, L, 48, 2)
        for sf in (0, -1):
            got = _run(dna, n, L, 48, 2, sf)
            _same(got, want, (L, sf))
            assert got["stats"]["strand_filter"] == (1 if sf == 0 else 0)


def test_two_chain_groups():
    """The two-group schedule at its smallest legal shape: 4 096 chains, two launches of k_round_mc side by side."""
    sa = _sa()
    n, L = 20000, 100
    dna = sa.synth_dna_host(n, L, n * L // 25, 1, 10000)
    read, ln = po.load_dna(dna, n, L)
    want = po.reorder_rounds_ph(read, ln, L, 4096, 2)
    for sf in (0, -1):
        got = _run(dna, n, L, 4096, 2, sf, phases=2)
        _same(got, want, ("phases", sf))
        assert got["stats"]["phases"] == 2 and got["stats"]["strand_filter"] == (1 if sf == 0 else 0)


def test_virtual_ranks():
    """One pool over two virtual ranks (k_round_mc<.., MG = true, KA = true>) against one context."""
    from spring_amd.pool import VirtualPool
    name, K, T = "syn5k_150", 64, 3
    dna, n, L, _, _ = _named(name)
    want = _want_named(name, K, T)
    single = _run(dna, n, L, K, T, 0)
    _same(single, want, "single")
    for sf in (0, -1):
        vp = VirtualPool(2, K, T, fused=3, deep_bins=-1, strand_filter=sf)
        try:
            got = vp.run(lambda s: s.load_dna(dna, n, L))
        finally:
            vp.close()
        _same(got, single, ("pool", sf))


@pytest.mark.parametrize("kw,on", [(dict(), 1), (dict(strand_filter=-1), 0), (dict(strand_filter=6), 1), (dict(known_absent=-1), 0),
                                   (dict(fused=2), 0), (dict(table_mode=2), 0), (dict(collect_stats=True, fused=0), 0),
                                   (dict(fused=0), 0)])
def test_stats(kw, on):
    """stats.strand_filter says whether the sweep ran: only in the four-chain kernel with the masks, on the hash-addressed
    table; where it does not run the table is not built either (nothing dropped).  (fused = 0 at 64 chains: the library's
    own choice is the one-chain kernel.)"""
    sa = _sa()
    name, K, T = "syn5k_150", 64, 3
    dna, n, L, _, _ = _named(name)
    o = dict(fused=3, deep_bins=-1)
    o.update(kw)
    if o.get("collect_stats"):
        o.pop("deep_bins")
    got = sa.reorder_dna(dna, n, L, sa.ReorderOpts(num_chains=K, num_thr=T, **o))
    _same(got, _want_named(name, K, T), kw)
    assert got["stats"]["strand_filter"] == on, kw
    if not on:
        assert got["stats"]["strand_filter_dropped"] == 0


@pytest.mark.parametrize("bad", [-2, 33, 1000])
def test_refused_values(bad):
    sa = _sa()
    with pytest.raises(Exception):
        sa.ReorderStage(sa.ReorderOpts(strand_filter=bad))
