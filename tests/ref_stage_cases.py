"""Inputs of the whole-stage comparisons with the reference (tests/test_oracle_vs_ref_stages.py) and of the recorded
fixtures tests/golden/ref_stage_<case>.npz (tests/golden/make_ref_golden.py, tests/test_gpu_vs_ref_stages.py).
Test infrastructure; generators only, nothing here runs the reference."""
import numpy as np

import readsets as rs
from helpers import interleave_order_N, make_N_reads, read_strings
from oracle import pyoracle as po


def short_contig_set():
    """Contigs shorter than max_readlen: 150 islands of 120 random bases, ten reads of 80..110 bases on each, and one
    read of 150 bases that sets max_readlen.  No contig can span 150 bases, so encode<>() never opens its
    `ref.size() >= max_readlen` gate (encoder.h:231) although singletons and N reads are waiting."""
    rng = np.random.default_rng(131)
    letters = np.frombuffer(b"ACGT", np.uint8)
    comp = np.array([3, 2, 1, 0], np.uint8)
    reads = []
    for _ in range(150):
        g = rng.integers(0, 4, 120, dtype=np.uint8)
        for _ in range(10):
            ln = int(rng.integers(80, 111))
            p = int(rng.integers(0, 120 - ln + 1))
            r = g[p:p + ln].copy()
            e = rng.random(ln) < 0.01
            r[e] = (r[e] + rng.integers(1, 4, int(e.sum()), dtype=np.uint8)) % 4
            if rng.random() < 0.5:
                r = comp[r][::-1]
            reads.append(letters[r].tobytes())
    reads.insert(len(reads) // 2, letters[rng.integers(0, 4, 150)].tobytes())
    return rs.pack_var(reads), len(reads), 150


def contig_spans(res):
    """Bases each contig of a reorder result spans (max(pos + len) - min(pos) over its records)."""
    if len(res["order"]) == 0:
        return np.zeros(0, np.int64)
    start = np.flatnonzero(res["flag"] == ord("0"))
    lo = np.minimum.reduceat(res["pos"], start)
    hi = np.maximum.reduceat(res["pos"] + res["rlen"].astype(np.int64), start)
    return hi - lo


def three_thread_set(n=3000, G=20000, extra=300):
    """The one multi-thread case whose reference run is deterministic: `n` reads of 100 bp of a small genome at 1 %
    substitutions, then `extra` uniform-random reads, which become the singleton pool.  -> (dna, n + extra, L)."""
    a = rs.np_reads(5, G, n, 100, 0.01)
    rnd = np.frombuffer(b"ACGT", np.uint8)[np.random.default_rng(77).integers(0, 4, (extra, 100))]
    return rs.pack_fixed(np.concatenate([a, rnd]).astype(np.uint8)), n + extra, 100


def three_thread_streams(read, ln, L, n_rel):
    """reorder_rounds(K = 6, T = 3) with order_s REPLACED by the indices of the appended random reads: no singleton can
    align to a contig, so the reference's threads have nothing to race for.  (Clean reads that the schedule left as
    singletons are then referenced by no file; the encoder only ever sees what the files hold.)"""
    res = dict(po.reorder_rounds(read, ln, L, 6, 3))
    res["order_s"] = np.arange(n_rel, len(ln), dtype=np.uint32)
    return res


def n_reads_for(read, ln, n, nN, deep, seed):
    Nreads = make_N_reads(read_strings(read, ln), nN, seed, deep=deep) if (nN or deep) else []
    return po.pack_dnaN(Nreads), interleave_order_N(n, len(Nreads), seed + 7), Nreads


# ------------------------------------------------------------------ the recorded fixtures
# case -> (what it carries).  Sizes are the smallest at which the edge still occurs and the .npz stays below the
# largest fixture of tests/golden (the inputs are random bases: they do not compress, and temp.dna.* holds them again).
FIXTURES = ("fixed100", "var", "short20", "long300", "deepN", "thr3", "fixed33", "fixed150", "fixed251")
# One read length that is no multiple of four, residues 1, 2 and 3: the fixed-length temp.dna writer takes a
# reverse-complemented record's bytes across a limb boundary and masks the last, partial byte only there.  case -> (seed,
# L, n): reads of a genome of 5 L bases at 1 % substitutions, n the smallest at which the reference's -t 1 run leaves two
# contigs and temp.dna.0 holds a reverse-complemented record.
R_RECORD_CASES = {"fixed33": (206, 33, 9), "fixed150": (207, 150, 9), "fixed251": (208, 251, 12)}


def holds_r_record(reorder_files, L):
    """temp.dna.0 of a one-thread file set of one read length holds a record written reverse-complemented."""
    rev = reorder_files["read_rev.txt.0"]
    return b"r" in rev and len(reorder_files["temp.dna.0"]) == len(rev) * (2 + (L + 3) // 4)


def fixture_inputs(case):
    """-> dict(dna, n, L, dnaN, order_N, T, K): the clean pool, the N reads, threads of the encoder run and the chains
    of the reorder run that feeds it (K = 1: the reference's own reorder_main; thr3: three_thread_streams)."""
    T, K, nN, deep, seed = 1, 1, 12, 0, 3
    if case == "fixed100":
        dna, n, L = rs.pack_fixed(rs.np_reads(201, 1500, 300, 100, 0.015)), 300, 100
    elif case == "var":      # variable length 50..150, 3 % substitutions: reads the reorder stage leaves single (more than
        reads = rs.var_length_reads(202, 1200, 260, 50, 150, 0.03)   # 4 mismatches) and the encoder aligns (up to 24)
        dna, n, L = rs.pack_var(reads), len(reads), max(len(r) for r in reads)
    elif case == "short20":  # L <= 50: the two singleton-dictionary windows differ in length
        dna, n, L = rs.pack_fixed(rs.np_reads(203, 4000, 900, 20, 0.0)), 900, 20
        nN = 40
    elif case == "long300":  # more than 256 bases: 10 limbs at 2 bits per base, 15 at 3
        dna, n, L = rs.pack_fixed(rs.np_reads(204, 1500, 100, 300, 0.01)), 100, 300
        nN = 6
    elif case == "deepN":    # 1600 near-copies (1067 forward) of one read with an N outside both windows: one bin > MAX_SEARCH_ENCODER
        dna, n, L = rs.pack_fixed(rs.np_reads(205, 800, 120, 100, 0.01)), 120, 100
        nN, deep, seed = 4, 1600, 5
    elif case == "thr3":
        dna, n, L = three_thread_set(240, 1600, 24)
        T, K, nN = 3, 6, 0
    elif case in R_RECORD_CASES:   # 11-byte records; the workload's length; 8 limbs
        rseed, L, n = R_RECORD_CASES[case]
        dna, nN = rs.pack_fixed(rs.np_reads(rseed, 5 * L, n, L, 0.01)), 4
    else:
        raise KeyError(case)
    read, ln = po.load_dna(dna, n, L)
    dnaN, order_N, _ = n_reads_for(read, ln, n, nN, deep, seed)
    return dict(dna=dna, n=n, L=L, dnaN=dnaN, order_N=order_N, T=T, K=K)


def fixture_reorder_files(case, inp):
    """The file set the fixture's encoder run starts from, when it is not the reference's own reorder output (thr3:
    the hand-made three-thread set, from the oracle's rounds schedule); None otherwise."""
    if case != "thr3":
        return None
    from helpers import reorder_file_set
    read, ln = po.load_dna(inp["dna"], inp["n"], inp["L"])
    return reorder_file_set(read, ln, inp["L"], three_thread_streams(read, ln, inp["L"], 240))


def record_fixture(case):
    """Runs the reference's two stages on the case (needs oracle/_ref) -> the arrays of ref_stage_<case>.npz."""
    u8 = lambda b: np.frombuffer(bytes(b), np.uint8)  # noqa: E731
    inp = fixture_inputs(case)
    n, L = inp["n"], inp["L"]
    out = {"in.dna": u8(inp["dna"]), "in.dnaN": u8(inp["dnaN"]), "in.order_N": inp["order_N"], "n": np.uint32(n),
           "L": np.uint32(L), "T": np.uint32(inp["T"]), "K": np.uint32(inp["K"])}
    files = fixture_reorder_files(case, inp)
    out["reorder_by_reference"] = np.bool_(files is None)
    if files is None:
        files, _, unmatched = po.ref_reorder(inp["dna"], None, L, n, 0)
        out["unmatched"] = np.uint32(unmatched)
    for k, v in files.items():
        out["reorder/" + k] = u8(v)
    files = dict(files)
    files["input_N.dna"] = inp["dnaN"]
    files["read_order_N.bin"] = inp["order_N"].tobytes()
    enc, _, matched = po.ref_encoder(files, L, inp["T"], n + len(inp["order_N"]), n)
    for k, v in enc.items():
        out["encoder/" + k] = u8(v)
    out["matched"] = np.array(matched, np.uint32)
    return out


def fixture_files(z, stage):
    """{file name: bytes} of one stage ('reorder' / 'encoder') of a loaded ref_stage_<case>.npz."""
    return {k[len(stage) + 1:]: z[k].tobytes() for k in z.files if k.startswith(stage + "/")}
