"""GPU tests of the presence table's build (dict_build.hip: k_pres_write + k_pres_insert; run with
`pytest -m gpu` on an MI355X).  The table is read back through spring_reorder_presence_table and held against the keys cut
from the reads on the host with the numpy model of tests/pres_model.py: every key is in the table or met a full bucket,
every slot is explained by keys and carries exactly the OR of their flags, no fingerprint twice in a bucket, no hole in a
bucket, and the drop count is the number of keys the table lacks.  That holds whatever order the keys were entered in, so
it holds for the table written once (the keys that are their own canonical form, by blocks of buckets) plus the rest, and
for the previous build (opts.dict_build_mode = 1) alike; where neither table has a full bucket the two hold the same
words.  The streams of the whole stage equal the oracle's under either build."""
import functools

import numpy as np
import pytest

import pres_model as pm
import readsets as rs
from helpers import KEYS, named_set
from oracle import pyoracle as po
from test_gpu_strand_filter import _palindrome_pool

pytestmark = pytest.mark.gpu

WRITE_LG = 10  # lg2 of the buckets a workgroup of k_pres_write writes (PRES_WRITE_LG, dict_build.h)


def _sa():
    import spring_amd
    return spring_amd


@functools.lru_cache(maxsize=None)
def _pool(name):
    """-> (dna, n, L, the two dictionaries' unique keys, window length)"""
    if name == "syn150":
        n, L = 4000, 150
        dna = rs.pack_fixed(rs.np_reads(610, n * L // 25, n, L, 0.01))
    elif name == "syn100":  # windows of 32 bases at L = 100 too; 20 000 reads: a table of 2^16 buckets
        n, L = 20000, 100
        dna = rs.pack_fixed(rs.np_reads(611, n * L // 25, n, L, 0.01))
    elif name == "syn64":   # windows of 20 bases: wl < 32
        n, L = 3000, 64
        dna = rs.pack_fixed(rs.np_reads(612, n * L // 25, n, L, 0.01))
    elif name == "pal150":  # palindromic windows, and W here / rc(W) there across the two dictionaries
        a = _palindrome_pool(150, 1050)
        n, L = a.shape
        dna = rs.pack_fixed(a)
    elif name == "pal64":
        a = _palindrome_pool(64, 964)
        n, L = a.shape
        dna = rs.pack_fixed(a)
    elif name == "few":     # a few hundred keys: a table smaller than one workgroup's block
        n, L = 200, 100
        dna = rs.pack_fixed(rs.np_reads(613, n * L // 25, n, L, 0.01))
    elif name == "short":   # reads of 60 bases in a pool of up to 100: dictionary 1 is empty (its window ends at base 81)
        n, L = 1500, 100
        a = rs.np_reads(614, n * 60 // 25, n, 60, 0.01)
        dna = rs.pack_var([bytes(r) for r in a])
    else:
        raise KeyError(name)
    read, ln = po.load_dna(dna, n, L)
    windows = po.dict_windows(L)
    return dna, n, L, pm.dict_keys(read, ln, windows), pm.window_len(windows)


def _build(name, **kw):
    """build_dict with the options the strand-filter tests use -> (lgb, slots, stats)"""
    sa = _sa()
    dna, n, L, _, _ = _pool(name)
    o = dict(num_chains=48, num_thr=2, fused=3, deep_bins=-1)
    o.update(kw)
    with sa.ReorderStage(sa.ReorderOpts(**o)) as s:
        s.load_dna(dna, n, L)
        s.build_dict()
        lgb, slots = s.presence_table()
        return lgb, slots, s.stats()


def _check(name, want_build=2, **kw):
    _, _, _, keys, wl = _pool(name)
    lgb, slots, st = _build(name, **kw)
    assert st["strand_filter_build"] == want_build, (name, kw)
    info = pm.check_table(slots, lgb, keys, wl, st["strand_filter_dropped"])
    assert st["numkeys"] == [len(keys[0]), len(keys[1])] and info["keys"] == sum(st["numkeys"])
    return lgb, slots, st, info


@pytest.mark.parametrize("name", ["syn150", "syn100", "syn64", "pal150", "pal64", "few", "short"])
@pytest.mark.parametrize("cap", [0, 4, 6, WRITE_LG, WRITE_LG + 1])
def test_table_contents(name, cap):
    """Uncapped (one bucket per key and up), 16 and 64 buckets for thousands of keys (one workgroup strides over all of
    them, nearly every bucket full), exactly one workgroup's block, and two blocks."""
    _, _, _, keys, _ = _pool(name)
    nm = len(keys[0]) + len(keys[1])
    lgb, _, st, info = _check(name, strand_filter=cap)
    free = (nm - 1).bit_length()  # one bucket per key, the next power of two
    assert lgb == (min(cap, free) if cap else free), (name, cap, lgb, nm)
    if name == "short":
        assert st["numkeys"][1] == 0
    if name.startswith("pal"):
        assert info["slots"] < info["held"] or info["full_buckets"]  # W and rc(W), and keys of both dictionaries, share slots
    if cap in (4, 6) and nm > 1000:
        assert st["strand_filter_dropped"] > 0 and info["full_buckets"] == 1 << lgb


@pytest.mark.parametrize("name", ["syn150", "pal150"])
@pytest.mark.parametrize("tab_scale", [1, 4])
def test_table_contents_beside_a_smaller_and_a_larger_main_table(name, tab_scale):
    """The main table has 0.625 * tab_scale buckets a key (to the next power of two), the presence table one: fewer at
    tab_scale = 1, more at 4 -- the two writers' blocks cut the same arrays differently, side by side."""
    _check(name, tab_scale=tab_scale)


@pytest.mark.parametrize("name", ["syn150", "syn100", "syn64", "pal150", "short"])
def test_written_once_equals_the_previous_build(name):
    """opts.dict_build_mode = 0 against 1 on uncapped tables: both pass the contents test, and every bucket that is full in
    neither holds the same slot words (in whatever order its keys claimed them)."""
    _, a, sa_, _ = _check(name, want_build=2, dict_build_mode=0)
    _, b, sb_, _ = _check(name, want_build=1, dict_build_mode=1)
    assert a.shape == b.shape
    open_ = (a[:, 3] == 0) & (b[:, 3] == 0)
    assert open_.sum() > 0.9 * len(a)
    assert np.array_equal(np.sort(a[open_], axis=1), np.sort(b[open_], axis=1))
    if not (~open_).any():
        assert sa_["strand_filter_dropped"] == sb_["strand_filter_dropped"] == 0


def test_second_table_on_memory_of_the_first():
    """Two builds in one process: the stage of the small pool gets blocks the first stage gave back to the library's block
    pool, and nothing clears a table before it is written -- a bucket k_pres_write left out would show what was there."""
    sa = _sa()
    _check("syn100")
    _check("syn100", dict_build_mode=1, want_build=1)  # (more blocks of every size with something in them)
    lgb, _, _, _ = _check("few")
    assert lgb < WRITE_LG
    _check("syn150", strand_filter=WRITE_LG + 1)
    with pytest.raises(sa.ReorderError):  # no table where the chain phase would not read it
        _build("few", strand_filter=-1)


@functools.lru_cache(maxsize=None)
def _want(name, K, T):
    dna, n, L = named_set(name)
    read, ln = po.load_dna(dna, n, L)
    return po.reorder_rounds(read, ln, L, K, T)


def _run_both_builds(dna, n, L, want, K, T, ph, what):
    sa = _sa()
    for mode, build in ((0, 2), (1, 1)):
        got = sa.reorder_dna(dna, n, L, sa.ReorderOpts(num_chains=K, num_thr=T, fused=3, deep_bins=-1, phases=ph,
                                                       dict_build_mode=mode))
        for k in KEYS:
            assert np.array_equal(got[k], want[k]), (what, K, mode, k)
        st = got["stats"]
        assert st["strand_filter"] == 1 and st["phases"] == ph and st["strand_filter_build"] == build, (what, K, mode)


@pytest.mark.parametrize("name", ["syn5k_150", "syn2k_100", "syn3k_64", "var2k", "dups", "test_1+2"])
def test_streams_equal_the_oracle_under_both_builds(name):
    """The four-chain kernel with the presence table written once and built the previous way: the same streams, the
    oracle's, and the sweep ran."""
    dna, n, L = named_set(name)
    for K, T in ((32, 2), (300, 3)):
        _run_both_builds(dna, n, L, _want(name, K, T), K, T, 1, name)


def test_streams_equal_the_oracle_under_both_builds_two_chain_groups():
    """... and with two chain groups at their smallest legal shape: 4 096 chains, two launches of k_round_mc side by side."""
    n, L = 20000, 100
    dna = _sa().synth_dna_host(n, L, n * L // 25, 1, 10000)
    read, ln = po.load_dna(dna, n, L)
    _run_both_builds(dna, n, L, po.reorder_rounds_ph(read, ln, L, 4096, 2), 4096, 2, 2, "two groups")
