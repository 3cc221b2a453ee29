"""The reorder and encoder oracles (oracle/reorder_oracle.c, encoder_oracle.c) against the REFERENCE'S OWN WHOLE STAGES:
reorder_main<N> -- reorder()'s loop (reorder.h:320-641: order of calls, position / RC / flag bookkeeping, early stop) and
writetofile (:643-730) -- and encoder_main<N> -- encode<>() (encoder.h:124-494: sliding window, per-thread merge, position
prefix) with encoder.cpp whole, built by oracle/Makefile into oracle/_ref/ref_reorder and ref_encoder.  The one thing
left out of the reference is the gzip filter: its four intermediate files cross the disk uncompressed.  Every comparison
is byte-exact, file by file, and the set of files left is compared too.  Skipped where oracle/_ref is not built.

One divergence is known and kept: write_dnaN_in_bits counts bytes in a uint8_t (util.cpp:330), so for a read of exactly
511 bases the reference writes the length and no payload; the oracle and the GPU write the 256 bytes (oracle/README.md).
`_as_reference_writes_dnaN` applies that to the expected read_unaligned.txt, at max_readlen = 511 only."""
import functools
import os

import numpy as np
import pytest

import ref_stage_cases as sc
from helpers import GOLDEN, early_stop_set, encoder_file_set, named_set, reorder_file_set, unpack_dnaN
from oracle import pyoracle as po

needs_ref = pytest.mark.skipif(po.ref_reorder_bin() is None or po.ref_encoder_bin() is None,
                               reason="oracle/_ref/ref_reorder, ref_encoder not built (needs the reference sources)")

NAMED = ["syn2k_100", "syn5k_150", "syn3k_64", "syn2k_251", "syn1k_511", "syn2k_20", "var2k", "var_short", "var_long",
         "heavy", "repeat10k", "dups", "test_1+2", "one", "empty"]
REORDER_LEFT = sorted(["read_order.bin.0", "read_rev.txt.0", "tempflag.txt.0", "temppos.txt.0", "read_lengths.bin.0",
                       "temp.dna.0", "temp.dna.singleton", "read_order.bin.singleton", "temp.dna.singleton.count"])


@functools.lru_cache(maxsize=None)
def _pool(name):
    dna, n, L = sc.short_contig_set() if name == "short_contigs" else named_set(name)
    read, ln = po.load_dna(dna, n, L)
    read.setflags(write=False)
    ln.setflags(write=False)
    return dna, n, L, read, ln


def _same_files(got, left, want, what):
    assert left == sorted(want), (what, left)
    for k in sorted(want):
        assert got[k] == want[k], (what, k, len(got[k]), len(want[k]))


def _reorder_vs_reference(what, dna1, dna2, L, n1, n2):
    dna, n = dna1 + (dna2 or b""), n1 + n2
    read, ln = po.load_dna(dna, n, L)
    want = po.reorder_serial(read, ln, L)
    got, left, unmatched = po.ref_reorder(dna1, dna2, L, n1, n2)
    assert left == REORDER_LEFT, (what, left)          # inputs consumed (reorder.h:232,241), nothing else left
    _same_files(got, left, reorder_file_set(read, ln, L, want), what)
    assert unmatched == want["stats"]["unmatched"], what
    return want


# ---------------------------------------------------------------- reorder_main, one thread
@needs_ref
@pytest.mark.parametrize("name", NAMED + ["tandem"])
def test_reorder_main_equals_serial_oracle(name):
    dna, n, L, _, _ = _pool(name)
    _reorder_vs_reference(name, dna, None, L, n, 0)


@needs_ref
def test_reorder_main_paired_pool_of_two_files():
    """input_clean_1.dna + input_clean_2.dna as one pool (reorder.h:233-242), the lengths of the two files differ."""
    d1, n1, L1 = named_set("syn2k_100")
    d2, n2, L2 = named_set("syn3k_64")
    _reorder_vs_reference("paired", d1, d2, max(L1, L2), n1, n2)


@needs_ref
@pytest.mark.slow
def test_reorder_main_early_stop():
    """The only route by which the reference's own early-stop counters (reorder.h:433-439, :561) are exercised: more than
    half of the first million iterations unmatched -> stop_searching, everything left comes out single without a search.
    Measured: 75 s of one CPU core, reference and oracle together (565 k reads), hence `slow`."""
    dna, n, L, _ = early_stop_set()
    want = _reorder_vs_reference("early-stop", dna, None, L, n, 0)
    assert want["stats"]["search_calls"] == 100_000_000 and len(want["order"]) == 0 and len(want["order_s"]) == n


# ---------------------------------------------------------------- encoder_main, one thread
def _as_reference_writes_dnaN(buf, L):
    if L != 511:
        return buf
    out, p = bytearray(), 0
    while p < len(buf):
        n = int.from_bytes(buf[p:p + 2], "little")
        body = (n + 1) // 2
        out += buf[p:p + 2] + (b"" if body == 256 else buf[p + 2:p + 2 + body])
        p += 2 + body
    return bytes(out)


def _encoder_vs_reference(what, read, ln, L, n, streams, T, dnaN=b"", order_N=None):
    order_N = np.zeros(0, np.uint32) if order_N is None else order_N
    files = reorder_file_set(read, ln, L, streams)
    files["input_N.dna"] = dnaN
    files["read_order_N.bin"] = order_N.tobytes()
    got, left, counts = po.ref_encoder(files, L, T, n + len(order_N), n)
    want = po.encode(read, ln, L, streams, num_thr=T, dnaN=dnaN, order_N=order_N)
    return got, left, counts, want


def _check_encoder(what, got, left, counts, want, L):
    exp = encoder_file_set(want)
    exp["read_unaligned.txt"] = _as_reference_writes_dnaN(exp["read_unaligned.txt"], L)
    _same_files(got, left, exp, what)                  # every input consumed, every stream, .raw / .tail per tid
    assert counts == (want["matched_s"], want["matched_N"]), (what, counts)


@needs_ref
@pytest.mark.parametrize("name,K,nN,deep", [(s, 1, 0, 0) for s in NAMED] +
                         [(s, 6, 200, 0) for s in ("syn2k_100", "var2k", "syn3k_64", "syn2k_20", "var_long", "heavy",
                                                   "dups", "test_1+2", "one", "empty")] +
                         [(s, 8, 50, 3500) for s in ("syn5k_150", "syn2k_251", "var_short", "repeat10k")])
def test_encoder_main_equals_oracle(name, K, nN, deep):
    """(K = 1, no N reads): fed with the serial oracle's file set, which test_reorder_main_equals_serial_oracle shows to
    be the reference's own.  (K = 6, 200 N reads) and (K = 8, 50 N reads + 3500 near-copies in one bin, more than
    MAX_SEARCH_ENCODER): the rounds schedule's streams in one tid.  L = 400 (var_long) and 511 are in; syn2k_20 has
    L <= 50, where the two dictionary windows differ in length."""
    dna, n, L, read, ln = _pool(name)
    streams = po.reorder_serial(read, ln, L) if K == 1 else po.reorder_rounds(read, ln, L, K, 1)
    dnaN, order_N, Nreads = sc.n_reads_for(read, ln, n, nN, deep, 5 if deep else 3)
    got, left, counts, want = _encoder_vs_reference(name, read, ln, L, n, streams, 1, dnaN, order_N)
    _check_encoder((name, K, nN, deep), got, left, counts, want, L)
    if deep and n:
        assert 1000 <= want["matched_N"] < len(Nreads)  # the bin is deeper than one probe takes


@needs_ref
def test_encoder_main_gate_closed_on_short_contigs():
    """No contig reaches max_readlen: `ref.size() >= max_readlen` (encoder.h:231) stays closed, nothing aligns although
    singletons and N reads (copies of clean reads, which would align) are there."""
    dna, n, L, read, ln = _pool("short_contigs")
    streams = po.reorder_serial(read, ln, L)
    spans = sc.contig_spans(streams)
    assert len(spans) > 100 and spans.max() < L and len(streams["order_s"]) > 0
    dnaN, order_N, Nreads = sc.n_reads_for(read, ln, n, 60, 0, 3)
    got, left, counts, want = _encoder_vs_reference("short contigs", read, ln, L, n, streams, 1, dnaN, order_N)
    assert counts == (0, 0)
    _check_encoder("short contigs", got, left, counts, want, L)


# ---------------------------------------------------------------- encoder_main, three threads (the deterministic case only)
@needs_ref
def test_encoder_main_three_threads_merge_and_position_prefix():
    """The per-thread merge (encoder.h:386-423) and the file_len_seq_thr position prefix (:465-487), trivial with one
    thread.  The reference's threads race for singletons, so its output is defined only when no singleton can align:
    the singleton pool is replaced by 300 uniform-random reads, and the reference's own matched counts are asserted to
    be 0 first.  No other multi-thread reference run belongs here: they are racy by design."""
    dna, n, L = sc.three_thread_set()
    read, ln = po.load_dna(dna, n, L)
    streams = sc.three_thread_streams(read, ln, L, 3000)
    assert all(int(x) > 0 for x in np.diff(streams["tid_off"]))     # all three tids hold contigs
    got, left, counts, want = _encoder_vs_reference("three threads", read, ln, L, n, streams, 3)
    assert counts == (0, 0), counts
    _check_encoder("three threads", got, left, counts, want, L)
    assert np.count_nonzero(want["seq_len_tid"]) == 3


# ---------------------------------------------------------------- the recorded fixtures (tests/golden/ref_stage_*.npz)
def _fixture(case):
    return np.load(os.path.join(GOLDEN, "ref_stage_%s.npz" % case))


@pytest.mark.parametrize("case", sc.FIXTURES)
def test_stage_fixture_holds_its_case_and_equals_the_oracle(case):
    """Runs without the reference: the fixture's inputs are the case's, its edge is there, and the reference's recorded
    files are what the oracles give."""
    z = _fixture(case)
    inp = sc.fixture_inputs(case)
    n, L, T = int(z["n"]), int(z["L"]), int(z["T"])
    assert (n, L, T, int(z["K"])) == (inp["n"], inp["L"], inp["T"], inp["K"])
    assert z["in.dna"].tobytes() == inp["dna"] and z["in.dnaN"].tobytes() == inp["dnaN"]
    assert np.array_equal(z["in.order_N"], inp["order_N"])
    rfiles, efiles = sc.fixture_files(z, "reorder"), sc.fixture_files(z, "encoder")
    read, ln = po.load_dna(inp["dna"], n, L)
    if bool(z["reorder_by_reference"]):
        streams = po.reorder_serial(read, ln, L)
        assert int(z["unmatched"]) == streams["stats"]["unmatched"]
        # at least one '0' that closes a contig (encoder.h:215), i.e. a second contig opens
        assert rfiles["tempflag.txt.0"].count(b"0") >= 2 and rfiles["tempflag.txt.0"].count(b"1") > 0
    else:
        streams = sc.three_thread_streams(read, ln, L, 240)
    assert rfiles == reorder_file_set(read, ln, L, streams)
    want = po.encode(read, ln, L, streams, num_thr=T, dnaN=inp["dnaN"], order_N=inp["order_N"])
    assert efiles == encoder_file_set(want)
    assert tuple(z["matched"].tolist()) == (want["matched_s"], want["matched_N"])
    # the edge each case is recorded for
    na = len(efiles["read_pos.bin"]) // 8
    order = np.frombuffer(efiles["read_order.bin"], np.uint32)[:na]
    rlen = np.frombuffer(efiles["read_lengths.bin"], np.uint16)[:na]
    rev = np.frombuffer(efiles["read_rev.txt"], np.uint8)
    isN = np.zeros(n + len(inp["order_N"]), bool)
    isN[inp["order_N"]] = True
    single = isN.copy()                                   # positions in the original file of singletons and N reads
    single[np.flatnonzero(~isN)[streams["order_s"]]] = True
    if case == "fixed100":
        assert L == 100 and np.all(ln == 100) and want["matched_s"] > 0
    elif case == "var":     # a reverse-strand singleton hit of a read shorter than max_readlen: pos = j + L - len
        assert np.any(single[order] & (rev == ord("r")) & (rlen < L)), "no reverse hit with len < L"
        assert np.any(single[order] & (rev == ord("d")) & (rlen < L))
    elif case == "short20":
        assert L == 20 and want["matched_s"] + want["matched_N"] > 0
    elif case == "long300":
        assert L > 256 and want["matched_s"] + want["matched_N"] > 0
    elif case == "deepN":   # one bin of the first dictionary window (bases 0..20) deeper than MAX_SEARCH_ENCODER
        heads = [s[:21] for s in unpack_dnaN(inp["dnaN"]) if "N" not in s[:21]]
        depth = max(heads.count(h) for h in set(heads))
        assert depth > 1000 and 1000 <= want["matched_N"] < len(inp["order_N"])
    elif case == "thr3":
        assert tuple(z["matched"].tolist()) == (0, 0) and np.count_nonzero(want["seq_len_tid"]) == 3
    elif case in sc.R_RECORD_CASES:   # one read length, no multiple of four, and a reverse-complemented record in temp.dna.0
        assert L == sc.R_RECORD_CASES[case][1] and L % 4 != 0 and np.all(ln == L)
        assert sc.holds_r_record(rfiles, L) and b"d" in rfiles["read_rev.txt.0"]
    else:
        raise KeyError(case)


@needs_ref
@pytest.mark.parametrize("case", sc.FIXTURES)
def test_stage_fixture_is_what_the_reference_writes(case):
    z = _fixture(case)
    now = sc.record_fixture(case)
    assert sorted(now) == sorted(z.files)
    for k in now:
        assert np.array_equal(np.asarray(now[k]), z[k]), (case, k)
