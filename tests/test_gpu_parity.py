"""GPU parity tests (run with `pytest -m gpu` on an MI355X): the HIP path, called through the
C ABI (spring_amd._lib -> libspring_reorder_hip.so), against the CPU oracle on identical inputs.
Bar: bit-exact (integer / byte / index work)."""
import gzip
import os

import numpy as np
import pytest

import readsets as rs
from helpers import GOLDEN, KEYS, SMALL_SETS, check_invariants, early_stop_set, named_set
from oracle import pyoracle as po

pytestmark = pytest.mark.gpu


def _sa():
    import spring_amd
    return spring_amd


def _gpu(name, K, T=1, **kw):
    sa = _sa()
    dna, n, L = named_set(name)
    # the library picks four chains per wavefront (k_round_mc) only from 49 152 chains on; the test sets are small, so
    # a run that does not say otherwise asks for that kernel (fused = 3) -- the automatic choice (one chain per
    # wavefront here) is what the fuzz's fused = 0 legs and the tests that pass `fused` themselves run
    if "fused" not in kw and not kw.get("collect_stats") and not kw.get("force_literal_update"):
        kw["fused"] = 3
    return sa.reorder_dna(dna, n, L, sa.ReorderOpts(num_chains=K, num_thr=T, **kw))


def _same(a, b, what):
    for k in KEYS:
        assert np.array_equal(a[k], b[k]), (what, k, len(a[k]), len(b[k]))


@pytest.mark.parametrize("name", ["test_1+2", "syn2k_100", "syn5k_150", "syn3k_64", "syn2k_251", "var2k",
                                  "var_short", "heavy", "one", "empty"])
def test_unpack_matches_readDnaFile(name):
    sa = _sa()
    dna, n, L = named_set(name)
    read, ln = po.load_dna(dna, n, L)
    with sa.ReorderStage() as s:
        s.load_dna(dna, n, L)
        limbs, lens = s.download_reads()
    assert np.array_equal(limbs, read) and np.array_equal(lens, ln)


@pytest.mark.parametrize("name", ["test_1+2", "syn2k_100", "syn5k_150", "syn3k_64", "syn2k_251", "var2k",
                                  "var_short", "heavy", "dups", "tandem"])
def test_dictionary_matches_constructdictionary(name):
    sa = _sa()
    dna, n, L = named_set(name)
    read, ln = po.load_dna(dna, n, L)
    with sa.ReorderStage() as s:
        s.load_dna(dna, n, L)
        s.build_dict()
        st = s.stats()
        for which in (0, 1):
            keys, sp, ids = po.build_dict(read, ln, L, which)
            assert st["numkeys"][which] == len(keys) and st["dict_numreads"][which] == len(ids)
            absent = keys ^ np.uint64(0x3333)
            absent = absent[~np.isin(absent, keys)]
            sizes, gids = s.dict_lookup(which, np.concatenate([keys, absent]))
            assert np.array_equal(sizes[:len(keys)], np.diff(sp).astype(np.uint32))
            assert np.all(sizes[len(keys):] == 0xFFFFFFFF)
            assert np.array_equal(gids[:len(ids)], ids)  # same ids, same in-bin order, bins in key order


@pytest.mark.parametrize("name", ["tandem", "repeat10k", "syn5k_150", "var2k"])
def test_minimizer_table_modes_agree(name):
    """The dictionary table addressed by the key's hash (default) and by its minimizer (table_mode = 2; applies to 32-base
    windows, reads up to 192 bases; an experiment of the four-chain round kernel, which keeps the window minimizers of a
    consensus in LDS): same streams as the rounds oracle.  `tandem` is built so
    that table neighbourhoods are over-subscribed: their keys live at the redirect address (TAG_MARK)."""
    sa = _sa()
    dna, n, L = named_set(name)
    read, ln = po.load_dna(dna, n, L)
    with sa.ReorderStage(sa.ReorderOpts(table_mode=2)) as s:
        s.load_dna(dna, n, L)
        s.build_dict()
        st = s.stats()
        for which in (0, 1):  # every key's bin through the minimizer-addressed table, incl. redirected keys
            keys, sp, ids = po.build_dict(read, ln, L, which)
            sizes, gids = s.dict_lookup(which, keys)
            assert np.array_equal(sizes, np.diff(sp).astype(np.uint32)) and np.array_equal(gids[:len(ids)], ids)
    assert st["table_minz"] == 1
    if name == "tandem":
        assert st["table_marked_lines"] > 0
    with sa.ReorderStage() as s:
        s.load_dna(dna, n, L)
        s.build_dict()
        assert s.stats()["table_minz"] == 0
    for K, T in ((1, 1), (32, 2)):
        want = po.reorder_rounds(read, ln, L, K, T)
        # (deep_bins = -1: `tandem` and `repeat10k` average enough reads per key for the deep-bin kernel variant, which the
        # minimizer experiment does not cover)
        for kw in (dict(fused=3, table_mode=2, deep_bins=-1), dict(fused=3, table_mode=2, tab_scale=4, deep_bins=-1),
                   dict(fused=3, table_mode=2, first_shifts=16, deep_bins=-1), dict(fused=3, deep_bins=-1), dict(fused=2)):
            _same(_gpu(name, K, T, **kw), want, (name, K, kw))
    # the one-chain kernels do not know minimizers: the combination is refused, not silently wrong
    with pytest.raises(sa.ReorderError):
        _gpu(name, 8, 1, fused=2, table_mode=2)


@pytest.mark.parametrize("fused", [0, -1])
@pytest.mark.parametrize("name", SMALL_SETS)
def test_k1_bit_exact_vs_serial_oracle(name, fused):
    """K = 1 must reproduce the reference's `-t 1` order byte for byte -- with the fused round kernel (default) and
    with the two-kernel round."""
    dna, n, L = named_set(name)
    read, ln = po.load_dna(dna, n, L)
    want = po.reorder_serial(read, ln, L)
    got = _gpu(name, 1, collect_stats=True, fused=fused)
    _same(got, want, name)
    for k in ("unmatched", "probes", "keyok", "cands", "hits", "iterations"):
        assert got["stats"][k] == want["stats"][k], (name, k, got["stats"][k], want["stats"][k])


@pytest.mark.parametrize("name", ["syn2k_100", "syn5k_150", "syn3k_64", "syn2k_251", "syn1k_511", "syn2k_20", "var_long",
                                  "var2k", "var_short", "heavy", "repeat10k", "dups", "test_1+2"])
@pytest.mark.parametrize("K,T", [(2, 1), (5, 2), (64, 8), (1000, 3)])
def test_chains_bit_exact_vs_rounds_oracle(name, K, T):
    dna, n, L = named_set(name)
    read, ln = po.load_dna(dna, n, L)
    want = po.reorder_rounds(read, ln, L, K, T)
    got = _gpu(name, K, T, collect_stats=True)
    _same(got, want, (name, K, T))
    assert np.array_equal(got["tid_off"], want["tid_off"]) and np.array_equal(got["tid_off_s"], want["tid_off_s"])
    for k in ("unmatched", "probes", "keyok", "cands", "hits", "iterations", "lost"):
        assert got["stats"][k] == want["stats"][k], (name, K, k, got["stats"][k], want["stats"][k])
    check_invariants(got, read, ln, L, n)


@pytest.mark.parametrize("name", ["syn2k_100", "var2k", "var_short", "syn2k_251", "syn1k_511", "var_long"])
def test_literal_and_parallel_consensus_paths_agree(name):
    a = _gpu(name, 8, 2)
    b = _gpu(name, 8, 2, force_literal_update=True)
    _same(a, b, name)


@pytest.mark.parametrize("name", ["syn2k_100", "var2k", "heavy"])
def test_golden_fixtures(name):
    g = np.load(os.path.join(GOLDEN, name + ".npz"))
    got = _gpu(name, 1)
    for k in KEYS:
        assert np.array_equal(got[k], g[k]), (name, k)
    for K in (4, 64):
        got = _gpu(name, K, 2)
        for k in KEYS:
            assert np.array_equal(got[k], g["K%d_%s" % (K, k)]), (name, K, k)


@pytest.mark.parametrize("name", ["syn2k_100", "var2k", "test_1+2"])
def test_emit_dna_matches_writetofile(name):
    sa = _sa()
    dna, n, L = named_set(name)
    read, ln = po.load_dna(dna, n, L)
    T = 3
    with sa.ReorderStage(sa.ReorderOpts(num_chains=16, num_thr=T)) as s:
        s.load_dna(dna, n, L)
        out = s.run().streams()
        for t in range(T):
            a, b = int(out["tid_off"][t]), int(out["tid_off"][t + 1])
            assert s.emit_dna(t) == po.write_dna_stream(read, ln, L, out["order"][a:b], out["rc"][a:b])
        assert s.emit_dna(-1) == po.write_dna_stream(read, ln, L, out["order_s"], None)


@pytest.mark.parametrize("paired", [False, True])
def test_call_reorder_file_contract(tmp_path, paired):
    """spring::call_reorder drop-in: consumes input_clean_*.dna, writes every file encoder_main<> opens."""
    sa = _sa()
    from spring_amd.reorder import CompressionParams
    if paired:
        d1, n1, L1 = named_set("syn2k_100")
        d2, n2, L2 = named_set("syn3k_64")
        dna, n, L = d1 + d2, n1 + n2, max(L1, L2)
        (tmp_path / "input_clean_1.dna").write_bytes(d1)
        (tmp_path / "input_clean_2.dna").write_bytes(d2)
        cp = CompressionParams(L, [n1, n2], num_thr=4, paired_end=True)
    else:
        dna, n, L = named_set("var2k")
        (tmp_path / "input_clean_1.dna").write_bytes(dna)
        cp = CompressionParams(L, [n, 0], num_thr=4, paired_end=False)
    K = 1
    sa.call_reorder(str(tmp_path), cp, sa.ReorderOpts(num_chains=K, num_thr=4))
    assert not (tmp_path / "input_clean_1.dna").exists()  # inputs are consumed (reorder.h:232,241)
    read, ln = po.load_dna(dna, n, L)
    want = po.reorder_serial(read, ln, L)
    # K=1 -> everything lands in tid 0; tids 1..3 must exist and be empty
    for t in range(4):
        for f in ("read_order.bin", "read_rev.txt", "tempflag.txt", "temppos.txt", "read_lengths.bin", "temp.dna"):
            assert (tmp_path / ("%s.%d" % (f, t))).exists(), (f, t)
    assert np.array_equal(np.fromfile(tmp_path / "read_order.bin.0", np.uint32), want["order"])
    assert gzip.open(tmp_path / "read_rev.txt.0").read() == want["rc"].tobytes()
    assert gzip.open(tmp_path / "tempflag.txt.0").read() == want["flag"].tobytes()
    assert gzip.open(tmp_path / "temppos.txt.0").read() == want["pos"].tobytes()
    assert gzip.open(tmp_path / "read_lengths.bin.0").read() == want["rlen"].tobytes()
    assert (tmp_path / "temp.dna.0").read_bytes() == po.write_dna_stream(read, ln, L, want["order"], want["rc"])
    assert (tmp_path / "temp.dna.singleton").read_bytes() == po.write_dna_stream(read, ln, L, want["order_s"], None)
    assert np.array_equal(np.fromfile(tmp_path / "read_order.bin.singleton", np.uint32), want["order_s"])
    assert np.fromfile(tmp_path / "temp.dna.singleton.count", np.uint32).tolist() == [len(want["order_s"])]
    for t in range(1, 4):
        assert (tmp_path / ("read_order.bin.%d" % t)).stat().st_size == 0
        assert gzip.open(tmp_path / ("read_rev.txt.%d" % t)).read() == b""


def test_error_behaviour():
    sa = _sa()
    from spring_amd.reorder import CompressionParams
    with pytest.raises(sa.ReorderError, match="Wrong bitset size"):
        sa.call_reorder("/tmp", CompressionParams(600, [1, 0]))
    with pytest.raises(sa.ReorderError):
        sa.call_reorder("/nonexistent_dir_xyz", CompressionParams(100, [1, 0]))
    with sa.ReorderStage() as s:
        with pytest.raises(sa.ReorderError):
            s.run_chains()  # out of order
        with pytest.raises(sa.ReorderError):
            s.load_dna(b"\x64\x00\x00", 1, 100)  # truncated record


def test_synth_host_equals_device():
    sa = _sa()
    n, L, G = 5000, 150, 30000
    with sa.ReorderStage() as s:
        s.load_synth(n, L, G, 11, 10000)
        dev = s.download_dna()
    assert dev == sa.synth_dna_host(n, L, G, 11, 10000)
    rep = 20000 | 0x80000000  # SPRING_SYNTH_REPEATS: genome with four exact copies of one unit
    with sa.ReorderStage() as s:
        s.load_synth(n, L, G, 12, rep)
        dev2 = s.download_dna()
    assert dev2 == sa.synth_dna_host(n, L, G, 12, rep) and dev2 != dev
    gen = 10000 | sa.SYNTH_GENOMIC  # genome with repeat families, tandem repeats, low-complexity runs
    with sa.ReorderStage() as s:
        s.load_synth(n, L, 40 * G, 13, gen)
        dev3 = s.download_dna()
    assert dev3 == sa.synth_dna_host(n, L, 40 * G, 13, gen) and dev3 != dev


@pytest.mark.parametrize("K,T,kw", [(1, 1, dict(collect_stats=True)), (64, 3, dict(collect_stats=True)), (256, 2, dict(fused=3, deep_bins=-1)),
                                    (256, 2, dict(deep_bins=1)), (256, 2, dict(fused=3, table_mode=2, deep_bins=-1)),
                                    (256, 2, dict(deep_bins=1, long_budget=1, long_split=1)), (300, 2, dict(deep_bins=1, long_budget=2, long_split=3, long_blocks=2)),
                                    (256, 2, dict(deep_bins=1, long_budget=1, long_split=1, entry_flags=-1)), (0, 3, dict(entry_flags=-1)),
                                    (0, 2, dict())])
def test_genome_like_pool_vs_oracle(K, T, kw):
    """A pool drawn from the genome-like generator (SYN_GENOMIC_FLAG: 64 Zipf-sized repeat families at 5-20 % divergence,
    tandem repeats, low-complexity runs, 72 % unique sequence): bins of hundreds of reads beside single-read bins,
    near-identical repeat copies within the Hamming threshold.  Every kernel family against the oracles."""
    sa = _sa()
    n, L = 120_000, 150
    G = n * L // 12
    dna = sa.synth_dna_host(n, L, G, 31, 10000 | sa.SYNTH_GENOMIC)
    read, ln = po.load_dna(dna, n, L)
    with sa.ReorderStage(sa.ReorderOpts(num_chains=K, num_thr=T, **kw)) as s:
        s.load_dna(dna, n, L)
        got = s.run().streams()
        Kused = got["stats"]["chains"]
    want = po.reorder_serial(read, ln, L) if K == 1 else po.reorder_rounds(read, ln, L, Kused, T)
    _same(got, want, ("genome-like", K, kw))
    if kw.get("collect_stats"):
        for k in ("unmatched", "probes", "keyok", "cands", "hits"):
            assert got["stats"][k] == want["stats"][k], k
    # the pool has what it is meant to have: deep bins and plenty of singletons
    keys, sp, ids = po.build_dict(read, ln, L, 0)
    assert np.diff(sp).max() > 20  # (thousands at 20 M reads: the families grow with the genome)


def test_config2_1M_100bp_k1_bit_exact():
    """BASELINE config 2: 1 M synthetic 100 bp reads, bit-exact read order vs the CPU `-t 1` oracle
    (the data set whose reference counters SURVEY.md section 8(c) records)."""
    sa = _sa()
    n, L = 1_000_000, 100
    dna = rs.pack_fixed(rs.np_reads(7, 4_000_000, n, L, 0.01))
    read, ln = po.load_dna(dna, n, L)
    want = po.reorder_serial(read, ln, L)
    got = sa.reorder_dna(dna, n, L, sa.ReorderOpts(num_chains=1, collect_stats=True))
    _same(got, want, "1M")
    assert got["stats"]["unmatched"] == 96_389 and got["stats"]["probes"] == 44_478_214
    assert got["stats"]["cands"] == 928_070 and got["stats"]["keyok"] == 927_453


def test_1M_150bp_many_chains_vs_rounds_oracle():
    sa = _sa()
    n, L, K, T = 1_000_000, 150, 4096, 8
    dna = sa.synth_dna_host(n, L, n * L // 25, 5, 10000)
    read, ln = po.load_dna(dna, n, L)
    want = po.reorder_rounds(read, ln, L, K, T)
    got = sa.reorder_dna(dna, n, L, sa.ReorderOpts(num_chains=K, num_thr=T))
    _same(got, want, "1M150")
    check_invariants(got, read, ln, L, n)


def test_full_size_properties_100M_150bp():
    """BASELINE config 3 at full size: size-independent properties of the output (the oracle cannot
    run 100 M reads in test time): permutation of the clean reads, flag/RC/pos/length consistency,
    per-tid streams made of whole contigs, determinism across two runs."""
    sa = _sa()
    n, L, T = 100_000_000, 150, 8
    outs = []
    for _ in range(2):
        with sa.ReorderStage(sa.ReorderOpts(num_thr=T, phases=-1)) as s:  # (the library's choice: two chain groups at this size)
            s.load_synth(n, L, n * L // 25, 11, 10000)  # counter-based generator: same bytes both times
            outs.append(s.run().streams())
            if len(outs) == 2:
                read, ln = s.download_reads()
    a, b = outs
    assert a["stats"]["phases"] == 2 and a["stats"]["chains"] == 65536
    for k in KEYS:
        assert np.array_equal(a[k], b[k]), k
    seen = np.zeros(n, dtype=np.uint8)
    seen[a["order"]] += 1
    seen[a["order_s"]] += 1
    assert len(a["order"]) + len(a["order_s"]) == n and seen.min() == 1 and seen.max() == 1
    f0 = a["flag"] == ord("0")
    assert np.all(a["pos"][f0] == 0) and np.all(a["rc"][f0] == ord("d")) and np.all(a["rlen"] == L)
    toff = [int(x) for x in a["tid_off"]]
    for lo, hi in zip(toff[:-1], toff[1:]):
        fl = a["flag"][lo:hi]
        assert fl[0] == ord("0") and fl[-1] == ord("1")
        assert not np.any((fl[:-1] == ord("0")) & (fl[1:] == ord("0")))
    assert a["stats"]["unmatched"] == int(f0.sum()) + len(a["order_s"])
    # every one of the ~86 M matched records replayed through the reference's state machine (orc_check_contigs): the read, at
    # its recorded orientation and position, is one search_match accepts on the consensus its contig had built by then
    c = po.check_contigs(read, ln, L, a)
    assert c["bad"] == 0 and c["contigs"] == int(f0.sum()) and c["matches"] == len(a["order"]) - c["contigs"], c
    if po.ref_units() is not None:  # ... and once more with the consensus kept by the reference's own updaterefcount<N>
        assert po.check_contigs(read, ln, L, a, reference_update=True) == c


@pytest.mark.parametrize("pool", ["6400x", "25600x", "phix", "genomic"])
def test_deep_pools_at_size_replay_check(pool):
    """20 M / 10 M-read pools of the coverage sweep with the library's own choices (chain count, deep-bin kernel variants, two
    chain groups or long-search kernels, two candidates per proposal where the pool is contended): the output is a
    permutation of the reads and every matched record verifies in the replay check -- sizes no oracle run reaches."""
    sa = _sa()
    L = 150
    n, G, err = {"6400x": (20_000_000, 468_750, 10000), "25600x": (20_000_000, 117_187, 10000), "phix": (10_000_000, 5_400, 10000),
                 "genomic": (20_000_000, 120_000_000, 10000 | sa.SYNTH_GENOMIC)}[pool]
    with sa.ReorderStage(sa.ReorderOpts(num_thr=8, phases=-1, alternatives=-1)) as s:
        s.load_synth(n, L, G, 21, err)
        got = s.run().streams()
        read, ln = s.download_reads()
    check_invariants(got, read, ln, L, n)
    c = po.check_contigs(read, ln, L, got)
    assert c["bad"] == 0 and c["matches"] == len(got["order"]) - c["contigs"], (pool, c, got["stats"]["phases"], got["stats"]["alternatives"])


@pytest.mark.parametrize("name,K", [("syn5k_150", 64), ("var2k", 24), ("heavy", 48), ("repeat10k", 96), ("test_1+2", 8)])
@pytest.mark.parametrize("G", [1, 2, 4])
def test_single_pool_is_independent_of_gpu_count(name, K, G):
    """sharding the chains of ONE read pool over G ranks (all-gather of proposals per
    round) must give exactly the single-GPU K-chain output.  G virtual ranks on one device."""
    from spring_amd.pool import VirtualPool
    sa = _sa()
    dna, n, L = named_set(name)
    read, ln = po.load_dna(dna, n, L)
    T = 3
    want = po.reorder_rounds(read, ln, L, K, T)
    single = sa.reorder_dna(dna, n, L, sa.ReorderOpts(num_chains=K, num_thr=T))
    vp = VirtualPool(G, K, T, fused=3)  # (four chains per wavefront on every rank; `single` runs the automatic choice)
    try:
        got = vp.run(lambda s: s.load_dna(dna, n, L))
    finally:
        vp.close()
    for k in KEYS:
        assert np.array_equal(got[k], want[k]), (name, G, k)
        assert np.array_equal(got[k], single[k]), (name, G, k)
    assert np.array_equal(got["tid_off"], want["tid_off"]) and np.array_equal(got["tid_off_s"], want["tid_off_s"])


@pytest.mark.parametrize("G", [2, 4])
def test_single_pool_on_a_contended_deep_pool(G):
    """The multi-GPU instantiation of the trimming kernel variant (balanced bin scan, resumed searches) plus bin
    compaction on every rank's replica: G virtual ranks over one contended pool == one GPU == rounds oracle."""
    from spring_amd.pool import VirtualPool
    sa = _sa()
    n, L, Gn, K, T = 60_000, 150, 600, 256, 2
    with sa.ReorderStage(sa.ReorderOpts(num_chains=K, num_thr=T, deep_bins=1)) as s:
        s.load_synth(n, L, Gn, 29, 10000)
        single = s.run().streams()
        dna = s.download_dna()
    vp = VirtualPool(G, K, T, deep_bins=1)
    try:
        got = vp.run(lambda s: s.load_synth(n, L, Gn, 29, 10000))
    finally:
        vp.close()
    read, ln = po.load_dna(dna, n, L)
    want = po.reorder_rounds(read, ln, L, K, T)
    for k in KEYS:
        assert np.array_equal(got[k], single[k]), (G, k)
        assert np.array_equal(got[k], want[k]), (G, k)


def test_single_pool_1M_4_virtual_ranks():
    from spring_amd.pool import VirtualPool
    sa = _sa()
    n, L, K, T, G = 1_000_000, 150, 4096, 8, 4
    single = None
    with sa.ReorderStage(sa.ReorderOpts(num_chains=K, num_thr=T)) as s:
        s.load_synth(n, L, n * L // 25, 5, 10000)
        single = s.run().streams()
    vp = VirtualPool(G, K, T)
    try:
        got = vp.run(lambda s: s.load_synth(n, L, n * L // 25, 5, 10000))
    finally:
        vp.close()
    for k in KEYS:
        assert np.array_equal(got[k], single[k]), k


@pytest.mark.parametrize("kw", [dict(first_shifts=1), dict(first_shifts=4), dict(first_shifts=-1), dict(deep_bins=1), dict(deep_bins=-1), dict(first_shifts=16), dict(seed_wide=-1),
                                dict(tab_scale=1), dict(tab_scale=4), dict(search_wpb=2), dict(search_wpb=4),
                                dict(dbg_search_lds=20000), dict(dbg_apply_lds=20000, fused=-1), dict(fused=-1),
                                dict(first_shifts=3, seed_wide=-1, tab_scale=1, search_wpb=4, fused=-1),
                                dict(table_mode=1, tab_scale=4), dict(plan0=(4, 4, 8, 16)), dict(plan0=(16,), plan1=(2, 2, 4), fused=3),
                                dict(plan0=(1, 1, 2, 4, 8, 16), deep_bins=1), dict(long_min=64, long_blocks=7, long_budget=2, deep_bins=1),
                                dict(deep_bins=1, entry_flags=-1), dict(known_absent=-1, fused=3, deep_bins=-1)])
@pytest.mark.parametrize("name,K,T", [("syn5k_150", 64, 3), ("var2k", 7, 2), ("heavy", 16, 1), ("tandem", 32, 2)])
def test_tuning_opts_do_not_change_results(name, K, T, kw):
    """Every tuning / experiment field of spring_reorder_opts at a non-default value: same streams, same per-tid
    offsets, same reference-equivalent work counters as the rounds oracle (the fields only move work between
    batches, table sizes and block shapes)."""
    dna, n, L = named_set(name)
    read, ln = po.load_dna(dna, n, L)
    want = po.reorder_rounds(read, ln, L, K, T)
    got = _gpu(name, K, T, collect_stats=True, **kw)
    _same(got, want, (name, kw))
    assert np.array_equal(got["tid_off"], want["tid_off"])
    for k in ("probes", "keyok", "cands", "hits", "unmatched"):
        assert got["stats"][k] == want["stats"][k], (k, kw)


@pytest.mark.parametrize("name", ["syn5k_150", "syn2k_100", "syn3k_64", "syn2k_20", "var2k", "var_short", "heavy", "tandem", "repeat10k", "dups", "test_1+2"])
@pytest.mark.parametrize("K,T", [(1, 1), (32, 2), (300, 3)])
def test_known_absent_windows_do_not_change_results(name, K, T):
    """The four-chain round kernel with and without the chains' known-absent window masks (opts.known_absent; reads up to
    192 bases: fixed and variable length, windows of 32 bases and shorter, lone seeds that turn round, contended pools where
    most proposals are lost and the search is repeated): the same streams as the rounds oracle either way -- a skipped probe
    is one whose answer was "absent" (the table never changes)."""
    dna, n, L = named_set(name)
    read, ln = po.load_dna(dna, n, L)
    want = po.reorder_serial(read, ln, L) if K == 1 else po.reorder_rounds(read, ln, L, K, T)
    for ka in (0, -1):
        _same(_gpu(name, K, T, fused=3, deep_bins=-1, known_absent=ka), want, (name, K, ka))


@pytest.mark.parametrize("L", [101, 127, 128, 160, 191, 192])
def test_known_absent_windows_read_lengths(L):
    """... at the read lengths where the masks' place in the chain record moves (the forward strand's four limbs start at
    limb dstart[0] / 32) and at the longest reads the kernel takes: fixed-length pools and the same reads cut to random
    lengths (the reverse cases of updaterefcount, reorder.h:157-200, move the masks by other amounts than the shift)."""
    sa = _sa()
    n = 4000
    a = rs.np_reads(500 + L, n * L // 25, n, L, 0.01)
    rng = np.random.default_rng(L)
    cut = [bytes(r[:int(k)]) for r, k in zip(a, rng.integers(L // 2, L + 1, n))]
    cut[0] = bytes(a[0])  # (the pool's maximum read length stays L)
    for dna in (rs.pack_fixed(a), rs.pack_var(cut)):
        read, ln = po.load_dna(dna, n, L)
        want = po.reorder_rounds(read, ln, L, 48, 2)
        for ka in (0, -1):
            got = sa.reorder_dna(dna, n, L, sa.ReorderOpts(num_chains=48, num_thr=2, fused=3, deep_bins=-1, known_absent=ka))
            _same(got, want, (L, ka))


@pytest.mark.parametrize("n,L,G,K", [(60_000, 100, 300, 256), (40_000, 150, 2_000, 500), (30_000, 150, 400, 37)])
def test_resumed_search_after_lost_proposals(n, L, G, K):
    """Contended pools (hundreds of chains on a genome of a few hundred bases: most proposals are lost, bins of
    hundreds to thousands of reads, some beyond MAX_SEARCH) through the trimming kernel variant WITHOUT work counting:
    that is the build in which a chain that lost its proposal resumes its search at the last winner's probe
    (search_step).  Streams must equal the rounds oracle, which always searches from the first probe; the counting
    run of the same pool must agree with both."""
    sa = _sa()
    outs = []
    for stats in (False, True):
        with sa.ReorderStage(sa.ReorderOpts(num_chains=K, num_thr=2, deep_bins=1, collect_stats=stats)) as st:
            st.load_synth(n, L, G, 23, 10000)
            outs.append(st.run().streams())
            dna = st.download_dna()
    read, ln = po.load_dna(dna, n, L)
    want = po.reorder_rounds(read, ln, L, K, 2)
    _same(outs[0], want, "resumed search")
    _same(outs[1], want, "counting run")
    assert outs[0]["stats"]["lost"] > n // 10  # the regime the test is about


@pytest.mark.parametrize("K", [16, 64, 300])
def test_resumed_search_with_bins_beyond_max_search(K):
    """Same build, on the set whose bins hold more than MAX_SEARCH_REORDER reads.  A probe that stopped at the cap may
    succeed later (deeper candidates come into reach), so a search after a lost proposal does not resume past such a
    probe (prop_rev bit 2); this set walks those bins, but does not by itself produce that sequence of events -- it
    guards the path, the rule is argued in search_step."""
    dna, n, L = named_set("heavy")
    read, ln = po.load_dna(dna, n, L)
    _same(_gpu("heavy", K, 1, deep_bins=1), po.reorder_rounds(read, ln, L, K, 1), ("heavy", K))


@pytest.mark.parametrize("budget,split,blocks", [(1, 0, 0), (3, 0, 0), (0, 0, 0), (1, 1, 0), (1, 2, 3), (1, 1, 1), (3, 16, 0)])
@pytest.mark.parametrize("n,L,G,K", [(60_000, 100, 300, 256), (40_000, 150, 2_000, 500), (30_000, 150, 400, 37)])
def test_long_searches_through_k_long(n, L, G, K, budget, split, blocks):
    """Deep-bin pools: a search that has used up `long_budget` compare passes in k_round is finished by k_long (one
    block of 16 wavefronts per chain, same probes / priority order / MAX_SEARCH rule).  budget 1 sends nearly every
    search over a multi-read bin there, 3 a mixture, 0 is the default (8 passes, and only searches with thousands of
    bin entries still ahead of them); the streams equal the rounds oracle and
    the run with k_long switched off.  split: chunks of 64 bin entries per part of a split search (long_split; 1 splits
    every search with four chunks ahead of it into up to eight parts that other blocks -- with `blocks` = 1 the same block,
    later -- take over); the default (128) never fires on pools of this size."""
    sa = _sa()
    outs = {}
    for b in (budget, -1):
        with sa.ReorderStage(sa.ReorderOpts(num_chains=K, num_thr=2, deep_bins=1, long_budget=b, long_split=split, long_blocks=blocks)) as st:
            st.load_synth(n, L, G, 23, 10000)
            outs[b] = st.run().streams()
            dna = st.download_dna()
    read, ln = po.load_dna(dna, n, L)
    want = po.reorder_rounds(read, ln, L, K, 2)
    _same(outs[budget], want, ("k_long", budget))
    _same(outs[-1], want, "k_long off")
    assert outs[-1]["stats"]["long_searches"] == 0
    if split in (1, 2):
        assert outs[budget]["stats"]["long_splits"] > 0
    assert outs[-1]["stats"]["long_splits"] == 0
    if budget > 0:  # (the default budget only fires on searches longer than these pools have)
        assert outs[budget]["stats"]["long_searches"] > (n // 20 if budget == 1 else 0), outs[budget]["stats"]["long_searches"]


@pytest.mark.parametrize("split", [0, 1, 4])
@pytest.mark.parametrize("K", [16, 300])
def test_long_searches_with_bins_beyond_max_search(K, split):
    """k_long on the set whose bins hold more than MAX_SEARCH_REORDER reads (the live-entry limit is kept per bin across
    the 64-entry chunks the wavefronts of a block take), also over two virtual ranks (proposal words instead of resv[])."""
    from spring_amd.pool import VirtualPool
    dna, n, L = named_set("heavy")
    read, ln = po.load_dna(dna, n, L)
    want = po.reorder_rounds(read, ln, L, K, 1)
    got = _gpu("heavy", K, 1, deep_bins=1, long_budget=1, long_split=split)
    _same(got, want, ("heavy k_long", K))
    assert got["stats"]["long_searches"] > 0
    vp = VirtualPool(2, K, 1, deep_bins=1, long_budget=1, long_split=split)
    try:
        got2 = vp.run(lambda s: s.load_dna(dna, n, L))
    finally:
        vp.close()
    for k in KEYS:
        assert np.array_equal(got2[k], want[k]), ("heavy k_long pool", K, k)


def test_paired_pool_through_pe_encode():
    """BASELINE config 4 at test size (tools/pe_config4.py runs it at 1 M and 50 M pairs): a paired synthetic pool
    (file-1 reads then their mates, reorder.h:233-242) -> reorder == rounds oracle -> encoder -> pe_encode == the
    real reference pe_encode.cpp when oracle/_ref/ref_order is present, else the oracle twin; mates end up n/2 apart."""
    sa = _sa()
    from spring_amd import order_ops as oo
    from spring_amd.encoder import EncoderStage
    npairs, L, K, T = 60_000, 150, 117, 4
    n = 2 * npairs
    with sa.ReorderStage(sa.ReorderOpts(num_chains=K, num_thr=T)) as st:
        st.load_synth(n, L, n * L // 25, 17, 10000 | sa.SYNTH_PAIRED)
        got = st.run().streams()
        dna = st.download_dna()
        with EncoderStage() as enc:
            enc.encode(st)
            es = enc.streams()
    assert dna == sa.synth_dna_host(n, L, n * L // 25, 17, 10000 | sa.SYNTH_PAIRED)   # device generator == host generator
    read, ln = po.load_dna(dna, n, L)
    _same(got, po.reorder_rounds(read, ln, L, K, T), "paired pool")
    new, _ = oo.pe_encode(es["order"])
    ref = po.ref_order("pe_encode", es["order"]) if po.ref_order_bin() else po.pe_encode(es["order"])
    assert np.array_equal(new, ref)
    order, half = es["order"], npairs
    pos_of = np.empty(n, np.uint32)
    pos_of[order] = np.arange(n, dtype=np.uint32)
    f1 = order < half
    assert np.array_equal(new[f1], np.arange(half, dtype=np.uint32))
    assert np.array_equal(new[~f1], new[pos_of[order[~f1] - half]] + half)


def _perm_and_flags(a, n, L):
    """size-independent properties of a reorder output at sizes no oracle run reaches (fixed-length pool)"""
    seen = np.zeros(n, dtype=np.uint8)
    seen[a["order"]] += 1
    seen[a["order_s"]] += 1
    assert len(a["order"]) + len(a["order_s"]) == n and seen.min() == 1 and seen.max() == 1
    f0 = a["flag"] == ord("0")
    assert np.all(a["pos"][f0] == 0) and np.all(a["rc"][f0] == ord("d")) and np.all(a["rlen"] == L)
    toff = [int(x) for x in a["tid_off"]]
    for lo, hi in zip(toff[:-1], toff[1:]):
        fl = a["flag"][lo:hi]
        assert fl[0] == ord("0") and fl[-1] == ord("1")
        assert not np.any((fl[:-1] == ord("0")) & (fl[1:] == ord("0")))
    return f0


def test_full_size_config4_paired_end_50M_pairs():
    """BASELINE config 4 at full size: 50 M mate pairs = 100 M reads x 150 bp as ONE pool (file-1 reads, then their mates:
    reorder.h:233-242) through reorder with the library's defaults -> replay check of every matched record -> encoder stage
    -> spring_order_pe_encode, with the size-independent properties of pe_encode.cpp:24-84: file-1 reads keep their
    reordered rank among themselves, every mate sits exactly n / 2 behind its file-1 read."""
    sa = _sa()
    from spring_amd import order_ops as oo
    from spring_amd.encoder import EncoderStage
    npairs, L, T = 50_000_000, 150, 8
    n = 2 * npairs
    with sa.ReorderStage(sa.ReorderOpts(num_thr=T, phases=-1)) as st:
        st.load_synth(n, L, n * L // 25, 17, 10000 | sa.SYNTH_PAIRED)
        a = st.run().streams()
        read, ln = st.download_reads()
        with EncoderStage() as enc:
            info = enc.encode(st)
            order = enc.streams()["order"]
    assert a["stats"]["phases"] == 2 and a["stats"]["chains"] == 65536
    f0 = _perm_and_flags(a, n, L)
    c = po.check_contigs(read, ln, L, a)
    assert c["bad"] == 0 and c["contigs"] == int(f0.sum()) and c["matches"] == len(a["order"]) - c["contigs"], c
    del read, ln
    assert len(order) == n and info["num_contigs"] > 0
    new, _ = oo.pe_encode(order)
    pos_of = np.empty(n, np.uint32)
    pos_of[order] = np.arange(n, dtype=np.uint32)   # (also: the encoder's read_order is a permutation)
    f1 = order < npairs
    assert int(f1.sum()) == npairs
    assert np.array_equal(new[f1], np.arange(npairs, dtype=np.uint32))
    assert np.array_equal(new[~f1], new[pos_of[order[~f1] - npairs]] + npairs)


def test_pool_200M_reads_one_rank_rccl():
    """Half of BASELINE config 5's pool (200 M x 150 bp, 262 144 chains) through the multi-GPU path -- spring_reorder_mg_run,
    the per-round exchange an in-place ncclAllGather on a 1-rank RCCL communicator: permutation and flag invariants over the
    whole output, the replay check on the records of one tid."""
    from spring_amd.pool import DistPool, OneRankComm
    sa = _sa()
    n, L, T, K = 200_000_000, 150, 8, 262_144
    comm = OneRankComm(0)
    try:
        dp = DistPool(comm, K, num_thr=T)
        try:
            st = dp.run(lambda s: s.load_synth(n, L, n * L // 25, 13, 10000))
            a = dp.streams()
            read, ln = dp.stage.download_reads()
        finally:
            dp.close()
    finally:
        comm.close()
    assert st["chains"] == K and st["n_matched"] + st["n_single"] == n
    _perm_and_flags(a, n, L)
    toff = [int(x) for x in a["tid_off"]]
    lo, hi = toff[3], toff[4]
    one = {k: a[k][lo:hi] for k in ("order", "rc", "flag", "pos")}
    one["tid_off"] = np.array([0, hi - lo], np.uint64)
    c = po.check_contigs(read, ln, L, one)
    assert c["bad"] == 0 and c["matches"] == (hi - lo) - c["contigs"] and c["contigs"] > 0, c


@pytest.mark.slow
def test_parity_10M_reads():
    """10 M x 150 bp (auto chains, 8 output sets): every reorder stream, the per-tid offsets and the reference-
    equivalent work counters against the rounds oracle.  The oracle side takes about two minutes of one CPU core;
    tools/parity_10M.py runs the same check (plus the encoder stage) at any size -- 50 M: profiles/r02_parity_50M.txt."""
    sa = _sa()
    n, L, T = 10_000_000, 150, 8
    K = max(1, min(65536, n >> 10))
    with sa.ReorderStage(sa.ReorderOpts(num_chains=K, num_thr=T, collect_stats=True)) as st:
        st.load_synth(n, L, n * L // 25, 3, 10000)
        got = st.run().streams()
        dna = st.download_dna()
    read, ln = po.load_dna(dna, n, L)
    del dna
    want = po.reorder_rounds(read, ln, L, K, T)
    _same(got, want, "10M")
    assert np.array_equal(got["tid_off"], want["tid_off"]) and np.array_equal(got["tid_off_s"], want["tid_off_s"])
    for k in ("probes", "keyok", "cands", "hits", "unmatched", "iterations", "lost"):
        assert got["stats"][k] == want["stats"][k], (k, got["stats"][k], want["stats"][k])
    # the production build (no counters: four chains per wavefront) on the same reads
    del got
    # (four chains per wavefront -- what a pool of 50 M reads and more runs by default -- and the automatic choice at
    # this chain count, one chain per wavefront)
    for fused in (3, 0):
        with sa.ReorderStage(sa.ReorderOpts(num_chains=K, num_thr=T, fused=fused)) as st:
            st.load_synth(n, L, n * L // 25, 3, 10000)
            got = st.run().streams()
        _same(got, want, ("10M-production", fused))
        assert np.array_equal(got["tid_off"], want["tid_off"]) and np.array_equal(got["tid_off_s"], want["tid_off_s"])
        for k in ("unmatched", "lost"):
            assert got["stats"][k] == want["stats"][k], (k, got["stats"][k], want["stats"][k])


@pytest.mark.slow
def test_parity_10M_reads_two_chain_groups():
    """The same pool under the schedule with two chain groups (opts.phases = 2, what the library runs from 16 384 chains
    on): the counting build (streams + reference-equivalent work counters) and both production mappings against
    orc_reorder_rounds_ph."""
    sa = _sa()
    n, L, T = 10_000_000, 150, 8
    K = max(1, min(65536, n >> 10))
    with sa.ReorderStage(sa.ReorderOpts(num_chains=K, num_thr=T, collect_stats=True, phases=2)) as st:
        st.load_synth(n, L, n * L // 25, 3, 10000)
        got = st.run().streams()
        dna = st.download_dna()
    assert got["stats"]["phases"] == 2
    read, ln = po.load_dna(dna, n, L)
    del dna
    want = po.reorder_rounds_ph(read, ln, L, K, T)
    _same(got, want, "10M, two groups")
    assert np.array_equal(got["tid_off"], want["tid_off"]) and np.array_equal(got["tid_off_s"], want["tid_off_s"])
    for k in ("probes", "keyok", "cands", "hits", "unmatched", "iterations", "lost"):
        assert got["stats"][k] == want["stats"][k], (k, got["stats"][k], want["stats"][k])
    del got
    for fused in (3, 0):
        with sa.ReorderStage(sa.ReorderOpts(num_chains=K, num_thr=T, fused=fused, phases=2)) as st:
            st.load_synth(n, L, n * L // 25, 3, 10000)
            got = st.run().streams()
        _same(got, want, ("10M-production, two groups", fused))
        assert np.array_equal(got["tid_off"], want["tid_off"]) and np.array_equal(got["tid_off_s"], want["tid_off_s"])
        for k in ("unmatched", "lost"):
            assert got["stats"][k] == want["stats"][k], (k, got["stats"][k], want["stats"][k])


def test_1M_150bp_k1_reference_counters_on_the_gpu():
    """SURVEY.md section 8(c), second data set (1 M x 150 bp, default_rng(11), G = 6 Mb): the counters the surveyor
    recorded from the real reference at -t 1, reproduced by the GPU's K = 1 path (and its streams == serial oracle)."""
    sa = _sa()
    n, L = 1_000_000, 150
    dna = rs.pack_fixed(rs.np_reads(11, 6_000_000, n, L, 0.01))
    read, ln = po.load_dna(dna, n, L)
    want = po.reorder_serial(read, ln, L)
    got = sa.reorder_dna(dna, n, L, sa.ReorderOpts(num_chains=1, collect_stats=True))
    _same(got, want, "1M150-k1")
    st = got["stats"]
    assert st["unmatched"] == 137_664 and len(got["order_s"]) == 127_731
    assert st["probes"] == 92_923_476 and st["cands"] == 996_385


def test_early_stop_fires_on_both_sides():
    """STOP_CRITERIA_REORDER (reorder.h:433-439, params.h): K = 1, > 50 % of the first million iterations unmatched
    -> stop_searching; every read left after that is emitted as a singleton without a search."""
    sa = _sa()
    dna, n, L, rel_dna = early_stop_set()
    read, ln = po.load_dna(dna, n, L)
    want = po.reorder_serial(read, ln, L)
    # the stop fired in the oracle: exactly one million iterations searched (50 shifts x 2 directions each), and the
    # related reads, which cluster when they are on their own, all came out as singletons
    assert want["stats"]["search_calls"] == 100_000_000 and len(want["order"]) == 0 and len(want["order_s"]) == n
    cread, cln = po.load_dna(rel_dna, 40_000, L)
    assert len(po.reorder_serial(cread, cln, L)["order_s"]) < 8_000
    for kw in (dict(collect_stats=True), dict()):
        got = sa.reorder_dna(dna, n, L, sa.ReorderOpts(num_chains=1, **kw))
        _same(got, want, "early-stop")
        assert got["stats"]["unmatched"] == n


def test_default_chain_count_on_a_deep_pool_vs_oracle():
    """num_chains = 0 on a deep-coverage pool: the library picks n / 128 (dictionary >= 1.3 reads per key), says so
    in its statistics, and the result equals the rounds oracle at that K."""
    sa = _sa()
    n, L, T = 300_000, 100, 3
    dna = sa.synth_dna_host(n, L, n * L // 400, 21, 10000)
    read, ln = po.load_dna(dna, n, L)
    with sa.ReorderStage(sa.ReorderOpts(num_chains=0, num_thr=T)) as s:
        s.load_dna(dna, n, L)
        s.build_dict()
        K, deep = s.auto_chains()
        s.run_chains()
        s.finalize()
        got = s.streams()
    assert deep and K == n >> 7
    assert got["stats"]["chains"] == K and got["stats"]["deep_pool"] & 1
    want = po.reorder_rounds(read, ln, L, K, T)
    _same(got, want, "auto-deep")
    # a shallow pool takes n / 1024
    dna2 = sa.synth_dna_host(n, L, n * L // 25, 22, 10000)
    with sa.ReorderStage(sa.ReorderOpts(num_chains=0, num_thr=T)) as s:
        s.load_dna(dna2, n, L)
        s.build_dict()
        assert s.auto_chains() == (n >> 10, False)


def _read_file_set(d, T):
    """-> the per-tid streams of a call_reorder output directory, concatenated in tid order (+ per-tid counts)"""
    out = {k: [] for k in ("order", "rc", "flag", "pos", "rlen", "dna")}
    cnt = []
    for t in range(T):
        o = np.fromfile(d / ("read_order.bin.%d" % t), np.uint32)
        cnt.append(len(o))
        out["order"].append(o.tobytes())
        out["rc"].append(gzip.open(d / ("read_rev.txt.%d" % t)).read())
        out["flag"].append(gzip.open(d / ("tempflag.txt.%d" % t)).read())
        out["pos"].append(gzip.open(d / ("temppos.txt.%d" % t)).read())
        out["rlen"].append(gzip.open(d / ("read_lengths.bin.%d" % t)).read())
        out["dna"].append((d / ("temp.dna.%d" % t)).read_bytes())
    res = {k: b"".join(v) for k, v in out.items()}
    res["cnt"] = cnt
    res["order_s"] = np.fromfile(d / "read_order.bin.singleton", np.uint32)
    res["dna_s"] = (d / "temp.dna.singleton").read_bytes()
    res["count_s"] = np.fromfile(d / "temp.dna.singleton.count", np.uint32).tolist()
    return res


def _check_file_set(got, want, read, ln, L, T):
    assert got["order"] == want["order"].tobytes() and got["rc"] == want["rc"].tobytes()
    assert got["flag"] == want["flag"].tobytes() and got["pos"] == want["pos"].tobytes()
    assert got["rlen"] == want["rlen"].tobytes()
    assert got["cnt"] == np.diff(want["tid_off"]).tolist()
    assert got["dna"] == po.write_dna_stream(read, ln, L, want["order"], want["rc"])
    assert np.array_equal(got["order_s"], want["order_s"]) and got["count_s"] == [len(want["order_s"])]
    assert got["dna_s"] == po.write_dna_stream(read, ln, L, want["order_s"], None)


@pytest.mark.parametrize("devices", [(), (0, 0), (0, 0, 0)])
def test_call_reorder_many_chains_and_device_list(tmp_path, devices):
    """The drop-in on a device list (SURVEY 8(b) `opts`): one pool over the listed devices inside ONE call -- host
    threads, contexts and the exchange live in the library -- writes the same merged per-tid file set as one device
    (here the entries repeat device 0, so the exchange goes through host memory).  200 k reads of 100 bp: the input is
    several pinned chunks, the outputs cross the 64 KiB stored-block size many times."""
    sa = _sa()
    from spring_amd.reorder import CompressionParams
    n, L, K, T = 200_000, 100, 510, 5
    dna = sa.synth_dna_host(n, L, n * L // 25, 31, 10000)
    (tmp_path / "input_clean_1.dna").write_bytes(dna)
    sa.call_reorder(str(tmp_path), CompressionParams(L, [n, 0], num_thr=T), sa.ReorderOpts(num_chains=K, num_thr=T, devices=devices))
    read, ln = po.load_dna(dna, n, L)
    want = po.reorder_rounds(read, ln, L, K, T)
    _check_file_set(_read_file_set(tmp_path, T), want, read, ln, L, T)


def test_call_reorder_two_chain_groups(tmp_path):
    """The drop-in with the chains in two groups (opts.phases = 2 -- what the call chooses by itself from 16 384 chains on):
    the file set == the two-group oracle's streams."""
    sa = _sa()
    from spring_amd.reorder import CompressionParams
    n, L, K, T = 200_000, 100, 4096, 5
    dna = sa.synth_dna_host(n, L, n * L // 25, 31, 10000)
    (tmp_path / "input_clean_1.dna").write_bytes(dna)
    sa.call_reorder(str(tmp_path), CompressionParams(L, [n, 0], num_thr=T), sa.ReorderOpts(num_chains=K, num_thr=T, phases=2))
    read, ln = po.load_dna(dna, n, L)
    want = po.reorder_rounds_ph(read, ln, L, K, T)
    _check_file_set(_read_file_set(tmp_path, T), want, read, ln, L, T)


@pytest.mark.parametrize("devices", [(), (0, 0)])
@pytest.mark.parametrize("L", [150, 153])
def test_call_reorder_file_set_at_lengths_not_a_multiple_of_four(tmp_path, L, devices):
    """The drop-in's temp.dna.<tid> / temp.dna.singleton where the fixed-length writer takes a reverse-complemented
    record's bytes across a limb boundary and masks the last, partial byte (L % 4 = 2: the workload's 150, whose 40-byte
    records never straddle an output word; L % 4 = 1: 153, whose 41-byte records do), on one device and on a device list."""
    sa = _sa()
    from spring_amd.reorder import CompressionParams
    n, K, T = 50_000, 256, 5
    dna = sa.synth_dna_host(n, L, n * L // 25, 31, 10000)
    (tmp_path / "input_clean_1.dna").write_bytes(dna)
    sa.call_reorder(str(tmp_path), CompressionParams(L, [n, 0], num_thr=T), sa.ReorderOpts(num_chains=K, num_thr=T, devices=devices))
    read, ln = po.load_dna(dna, n, L)
    want = po.reorder_rounds(read, ln, L, K, T)
    assert np.count_nonzero(want["rc"] == ord("r")) > 0 and np.count_nonzero(want["rc"] == ord("d")) > 0
    _check_file_set(_read_file_set(tmp_path, T), want, read, ln, L, T)


def test_call_reorder_two_chain_groups_150bp(tmp_path):
    """... and with the chains in two groups at the workload's length: a tid's temp.dna stream is written in two pieces, split
    at `records of the first group * record size` bytes."""
    sa = _sa()
    from spring_amd.reorder import CompressionParams
    n, L, K, T = 200_000, 150, 4096, 5
    dna = sa.synth_dna_host(n, L, n * L // 25, 31, 10000)
    (tmp_path / "input_clean_1.dna").write_bytes(dna)
    sa.call_reorder(str(tmp_path), CompressionParams(L, [n, 0], num_thr=T), sa.ReorderOpts(num_chains=K, num_thr=T, phases=2))
    read, ln = po.load_dna(dna, n, L)
    want = po.reorder_rounds_ph(read, ln, L, K, T)
    assert np.count_nonzero(want["rc"] == ord("r")) > 0
    _check_file_set(_read_file_set(tmp_path, T), want, read, ln, L, T)


def test_call_reorder_lengths_that_hide_in_a_fixed_size_stream(tmp_path):
    """Reads of 97..100 bases all take 2 + 25 bytes: the stream has the size of a fixed-length one, the device-side
    length check notices, and the stage falls back to walking the records."""
    sa = _sa()
    from spring_amd.reorder import CompressionParams
    reads = rs.var_length_reads(77, 9000, 3000, 97, 100, 0.01)
    assert len(set(len(r) for r in reads)) > 1
    dna, n, L = rs.pack_var(reads), len(reads), 100
    assert len(dna) == n * 27
    (tmp_path / "input_clean_1.dna").write_bytes(dna)
    sa.call_reorder(str(tmp_path), CompressionParams(L, [n, 0], num_thr=2), sa.ReorderOpts(num_chains=16, num_thr=2))
    read, ln = po.load_dna(dna, n, L)
    want = po.reorder_rounds(read, ln, L, 16, 2)
    _check_file_set(_read_file_set(tmp_path, 2), want, read, ln, L, 2)
    got = sa.reorder_dna(dna, n, L, sa.ReorderOpts(num_chains=16, num_thr=2))  # the in-memory entry takes the same path
    _same(got, want, "same-size")
