"""GPU tests of the quality and id stage (include/spring_qualid.h) against the checker tests/qualid_model.py: bytes,
line lengths and the block table byte for byte over every alignment the 16-byte copy meets, the tables, the two
input forms, the paired-id check, the rest of the pipeline, and the refusals."""
import functools
import gzip
import os

import numpy as np
import pytest

import qualid_model as qm
import ref_cases as rc
from helpers import GOLDEN, interleave_order_N, make_N_reads, named_set, read_strings
from oracle import pyoracle as po

pytestmark = pytest.mark.gpu

LENGTHS = (0, 1, 15, 16, 17, 31, 63, 64, 65, 255, 511)
N_REC = 3003   # 273 cycles of LENGTHS
# every quality value 33..126, and bytes below 33 ('\n' and '\r' end lines)
QUAL_BYTES = np.array([c for c in range(1, 127) if c not in (10, 13)], np.uint8)
ID_BYTES = np.array([c for c in range(32, 127)], np.uint8)


@functools.lru_cache(maxsize=None)
def synth(seed, n=N_REC, final_newline=True):
    """A FASTQ text of n records: read / quality lengths cycle through LENGTHS (file 2 starts elsewhere in the cycle),
    ids of 1 .. 1200 bytes with a few of exactly 16 and 32, about a tenth of the lines end in CR LF."""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        L = LENGTHS[(i + 3 * seed) % len(LENGTHS)]
        il = 16 if i % 97 == 5 else 32 if i % 97 == 6 else 1 + (i * 7919 + seed) % 1200
        rid = b"@" + ID_BYTES[rng.integers(0, len(ID_BYTES), il - 1)].tobytes()
        read = np.frombuffer(b"ACGTN", np.uint8)[rng.integers(0, 5, L)].tobytes()
        qual = QUAL_BYTES[rng.integers(0, len(QUAL_BYTES), L)].tobytes()
        for line in (rid, read, b"+", qual):
            out.append(line + (b"\r\n" if rng.random() < 0.1 else b"\n"))
    text = b"".join(out)
    return text if final_newline else text[:-2] if text.endswith(b"\r\n") else text[:-1]


def orders(which, num_reads):
    if which == "identity":
        return None
    if which == "reversed":
        return np.arange(num_reads, dtype=np.uint32)[::-1].copy()
    return np.random.default_rng(num_reads).permutation(num_reads).astype(np.uint32)


def same(stage, kind, want, what=""):
    data, ln, off = stage.download(kind)
    assert np.array_equal(off, want["block_off"]), (what, "block table")
    assert np.array_equal(ln, want["len"]), (what, "len")
    assert data == want["bytes"], (what, "bytes")
    assert stage.info["bytes"][kind] == len(want["bytes"]) and stage.info["max_len"][kind] == want["max_len"], what
    assert stage.info["num_units"] == len(want["len"]) and stage.info["num_blocks"] == len(want["block_off"]) - 1


@pytest.mark.parametrize("pe", [False, True])
@pytest.mark.parametrize("which", ["identity", "reversed", "random"])
def test_shapes_against_the_checker(pe, which):
    from spring_amd import QualIdStage
    files = [synth(1), synth(2)] if pe else [synth(1)]
    n = N_REC * len(files)
    order = orders(which, n)
    slots = qm.order_array(order, n, pe)
    with QualIdStage() as qs:
        qs.set_order(order, n, pe)
        for j, f in enumerate(files):
            for B in (1, 3, 4, 1000, 1 << 30):
                info = qs.from_fastq(f, num_reads_per_block=B)
                assert info["num_blocks"] == (N_REC + B - 1) // B and info["bytes_changed"] == 0
                for kind in (qm.QUALITY, qm.ID):
                    same(qs, kind, qm.from_fastq(f, kind, slots, B), (pe, which, j, B, kind))
        # the kinds one at a time give the same, and the other kind is then not there
        from spring_amd.reorder import ReorderError
        for kind in (qm.QUALITY, qm.ID):
            qs.from_fastq(files[-1], want=kind, num_reads_per_block=3)
            same(qs, kind, qm.from_fastq(files[-1], kind, slots, 3), (pe, which, "alone", kind))
            with pytest.raises(ReorderError, match="code -4"):
                qs.download(1 - kind)


def test_blocks_are_the_string_arrays():
    from spring_amd import QualIdStage
    f = synth(1)
    order = orders("random", N_REC)
    slots = qm.order_array(order, N_REC, False)
    with QualIdStage() as qs:
        qs.set_order(order, N_REC)
        qs.from_fastq(f, num_reads_per_block=1000)
        for kind in (qm.QUALITY, qm.ID):
            want = qm.from_fastq(f, kind, slots, 1000)["lines"]
            assert qs.blocks(kind) == [want[0:1000], want[1000:2000], want[2000:3000], want[3000:]]


@pytest.mark.parametrize("which", ["identity", "random"])
def test_no_final_newline_and_tiny_inputs(which):
    from spring_amd import QualIdStage
    f = synth(3, final_newline=False)
    assert not f.endswith(b"\n")
    order = orders(which, N_REC)
    slots = qm.order_array(order, N_REC, False)
    with QualIdStage() as qs:
        qs.set_order(order, N_REC)
        for B in (4, 1000):
            qs.from_fastq(f, num_reads_per_block=B)
            for kind in (qm.QUALITY, qm.ID):
                same(qs, kind, qm.from_fastq(f, kind, slots, B), (which, B, kind))
        # n = 1 single-end, n = 2 paired-end (one record per file)
        one = [b"@a\nACGTA\n+\nIJKLM\n", b"@b 2\nAC\n+\n#I"]
        for pe, n, order in ((False, 1, None), (False, 1, [0]), (True, 2, None), (True, 2, [1, 0]), (True, 2, [0, 1])):
            qs.set_order(order, n, pe)
            for f1 in one:
                qs.from_fastq(f1, num_reads_per_block=1)
                for kind in (qm.QUALITY, qm.ID):
                    same(qs, kind, qm.from_fastq(f1, kind, [0], 1), (pe, n, kind))
        # nothing at all
        qs.set_order(None, 0)
        info = qs.from_fastq(b"", num_reads_per_block=5)
        assert info["num_units"] == 0 and info["num_blocks"] == 0 and info["bytes"] == [0, 0]
        assert qs.download(0)[0] == b"" and qs.download(1)[2].tolist() == [0]


@pytest.mark.parametrize("which", ["identity", "random"])
def test_many_short_lines(which):
    """More slots in 4 KiB of output than the copy keeps in LDS (1024), about as many, and fewer: the first third of
    the records has reads of 0 or 1 bases, the second of 3 .. 5 (about 1024 lines per 4 KiB), the last of 30 .. 40; ids
    of 1 .. 3 bytes ('\n' included: 2 .. 4 per slot)."""
    from spring_amd import QualIdStage
    n = 9000
    rng = np.random.default_rng(9)
    recs = []
    for i in range(n):
        L = int(rng.integers(0, 2)) if i < n // 3 else int(rng.integers(3, 6)) if i < 2 * n // 3 else int(rng.integers(30, 41))
        rid = b"@" + ID_BYTES[rng.integers(0, len(ID_BYTES), i % 3)].tobytes()
        recs.append(b"%s\n%s\n+\n%s\n" % (rid, b"ACGTN"[:1] * L, QUAL_BYTES[rng.integers(0, len(QUAL_BYTES), L)].tobytes()))
    f = b"".join(recs)
    order = orders(which, n)
    slots = qm.order_array(order, n, False)
    t = QualIdStage.quality_table("binary", 20, 40, 6)
    with QualIdStage() as qs:
        qs.set_order(order, n)
        info = qs.from_fastq(f, table=t, num_reads_per_block=1000)
        want = qm.from_fastq(f, qm.QUALITY, slots, 1000, qm.binary_table(20, 40, 6))
        same(qs, qm.QUALITY, want, which)
        assert info["bytes_changed"] == want["changed"]
        same(qs, qm.ID, qm.from_fastq(f, qm.ID, slots, 1000), which)
        if which == "identity":   # the three densities really are there
            off = want["block_off"]
            per4k = [np.searchsorted(np.cumsum(want["len"]), 4096 * (k + 1)) for k in range(int(off[-1]) // 4096)]
            d = np.diff([0] + per4k)
            assert d.max() > 1024 and d.min() < 1024


@pytest.mark.parametrize("rest", [1, 15])
def test_outputs_that_end_in_a_partial_word(rest):
    """Quality and id bytes of 16 k + 1 and 16 k + 15 in all: the copy's last word is written byte by byte, with and
    without a table."""
    from spring_amd import QualIdStage
    lq = (10, 11, 11 + rest)             # 32 + rest quality bytes
    li = (13, 14, 2 + (16 - rest))       # with their '\n': 48 - rest id bytes, the other remainder
    f = b"".join(b"@%s\n%s\n+\n%s\n" % (b"i" * (a - 1), b"A" * b, b"I5#"[k:k + 1] * b) for k, (a, b) in enumerate(zip(li, lq)))
    t, mt = QualIdStage.quality_table("illumina"), qm.illumina_table()
    with QualIdStage() as qs:
        qs.set_order([2, 0, 1], 3)
        slots = qm.order_array(np.array([2, 0, 1], np.uint32), 3, False)
        for table, model in ((None, None), (t, mt)):
            info = qs.from_fastq(f, table=table, num_reads_per_block=2)
            assert info["bytes"] == [32 + rest, 48 - rest]
            want = qm.from_fastq(f, qm.QUALITY, slots, 2, model)
            same(qs, qm.QUALITY, want, (rest, table is not None))
            same(qs, qm.ID, qm.from_fastq(f, qm.ID, slots, 2), (rest, "id"))
            assert info["bytes_changed"] == (want["changed"] if table is not None else 0)


@pytest.mark.parametrize("table", ["none", "illumina", "binary"])
def test_tables(table):
    from spring_amd import QualIdStage
    f = synth(1)
    assert set(range(33, 127)) <= set(b"".join(qm.fastq_lines(f)[2]))
    order = orders("random", N_REC)
    slots = qm.order_array(order, N_REC, False)
    t = {"none": None, "illumina": QualIdStage.quality_table("illumina"),
         "binary": QualIdStage.quality_table("binary", 20, 40, 6)}[table]
    mt = {"none": None, "illumina": qm.illumina_table(), "binary": qm.binary_table(20, 40, 6)}[table]
    with QualIdStage() as qs:
        qs.set_order(order, N_REC)
        for B in (3, 1000):
            info = qs.from_fastq(f, table=t, num_reads_per_block=B)
            want = qm.from_fastq(f, qm.QUALITY, slots, B, mt)
            same(qs, qm.QUALITY, want, (table, B))
            same(qs, qm.ID, qm.from_fastq(f, qm.ID, slots, B), (table, B, "id"))   # ids never see the table
            assert info["bytes_changed"] == want["changed"]
            assert (want["changed"] > 0) == (table != "none")


@pytest.mark.parametrize("case", sorted(rc.QUALID_FIXTURES))
@pytest.mark.parametrize("table", ["none", "illumina"])
def test_equals_reference_written_blocks(case, table):
    """Bytes, line lengths and block table against what the reference's own reorder_compress_quality_id wrote
    (tests/golden/ref_qualid_<case>.npz, recorded by tests/golden/make_ref_golden.py; the Illumina case by the real
    quantize_quality before the real writer, as preprocess does), from both input forms: no model in between."""
    from spring_amd import QualIdStage
    g = rc.load_qualid_fixture(case)
    t = QualIdStage.quality_table("illumina") if table == "illumina" else None
    with QualIdStage() as qs:
        qs.set_order(g["order"], g["N"], g["pe"])
        for m in range(2 if g["pe"] else 1):
            qname, iname = "quality_%d" % (m + 1), "id_%d" % (m + 1)
            wq, wi = g["want"][(qname, table)], g["want"][(iname, "none")]
            quals, ids = g["files"][qname].split(b"\n")[:-1], g["files"][iname].split(b"\n")[:-1]
            fastq = b"".join(b"%s\n%s\n+\n%s\n" % (i, b"A" * len(q), q) for i, q in zip(ids, quals))
            info = qs.from_fastq(fastq, table=t, num_reads_per_block=g["B"])
            same(qs, qm.QUALITY, wq, (case, table, m, "fastq"))
            same(qs, qm.ID, wi, (case, table, m, "fastq id"))
            assert (info["bytes_changed"] > 0) == (table == "illumina")
            qs.from_lines(qm.QUALITY, g["files"][qname], table=t, num_reads_per_block=g["B"])
            same(qs, qm.QUALITY, wq, (case, table, m, "lines"))
            qs.from_lines(qm.ID, g["files"][iname], table=t, num_reads_per_block=g["B"])
            same(qs, qm.ID, wi, (case, table, m, "lines id"))


@pytest.mark.parametrize("pe", [False, True])
def test_lines_and_gzip_equal_the_fastq(pe):
    from spring_amd import QualIdStage
    f = synth(2)
    n = N_REC * (2 if pe else 1)
    order = orders("random", n)
    ids, _, quals = qm.fastq_lines(f)
    images = {qm.QUALITY: b"".join(q + b"\n" for q in quals), qm.ID: b"".join(i + b"\n" for i in ids)}
    t = QualIdStage.quality_table("illumina")
    with QualIdStage() as qs, QualIdStage() as ql:
        qs.set_order(order, n, pe)
        ql.set_order(order, n, pe)
        info = qs.from_fastq(f, table=t, num_reads_per_block=7)
        ref = {k: qs.download(k) for k in (qm.QUALITY, qm.ID)}
        for kind in (qm.QUALITY, qm.ID):
            li = ql.from_lines(kind, images[kind], table=t, num_reads_per_block=7)
            got = ql.download(kind)
            assert got[0] == ref[kind][0] and np.array_equal(got[1], ref[kind][1]) and np.array_equal(got[2], ref[kind][2])
            assert li["bytes"][kind] == info["bytes"][kind] and li["bytes"][1 - kind] == 0
            assert li["bytes_changed"] == (info["bytes_changed"] if kind == qm.QUALITY else 0)
        # a last line without its '\n'
        ql.from_lines(qm.ID, images[qm.ID][:-1], num_reads_per_block=7)
        assert ql.download(qm.ID)[0] == ref[qm.ID][0]
        gi = ql.from_fastq(gzip.compress(f, 1), table=t, num_reads_per_block=7)
        assert gi["bytes"] == info["bytes"] and gi["bytes_changed"] == info["bytes_changed"]
        for kind in (qm.QUALITY, qm.ID):
            assert ql.download(kind)[0] == ref[kind][0]


# ---------------------------------------------------------------- against the rest of the pipeline
TR = bytes.maketrans(b"ACGTN", b"I5#?!")
TR_BACK = bytes.maketrans(b"I5#?!", b"ACGTN")


def _fastq(ids, reads):
    return b"".join(b"%s\n%s\n+\n%s\n" % (i, r, r.translate(TR)) for i, r in zip(ids, reads))


def _golden(j):
    lines = open(os.path.join(GOLDEN, "test_%d.fastq" % j), "rb").read().split(b"\n")
    return _fastq([x.strip() for x in lines[0:-1:4]], [x.strip() for x in lines[1:-1:4]])


def _single_end_with_N():
    dna, n, L = named_set("var2k")
    read, ln = po.load_dna(dna, n, L)
    strs = read_strings(read, ln)
    Nreads = make_N_reads(strs, 80, 5)
    order_N = interleave_order_N(n, len(Nreads), 12)
    isN = np.zeros(n + len(Nreads), bool)
    isN[order_N] = True
    it_c, it_N = iter(strs), iter(Nreads)
    reads = [(next(it_N) if isN[p] else next(it_c)).encode() for p in range(n + len(Nreads))]
    return _fastq([b"@r.%d" % i for i in range(len(reads))], reads)


@pytest.mark.parametrize("case", ["golden_pe", "single_end_N"])
def test_quality_lines_follow_the_decoded_reads(case):
    import spring_amd
    from spring_amd import DecodeStage, QualIdStage, StreamsStage
    from spring_amd.encoder import EncoderStage
    f = [_golden(1), _golden(2)] if case == "golden_pe" else [_single_end_with_N()]
    pe = len(f) == 2
    with spring_amd.ReorderStage(spring_amd.ReorderOpts(num_chains=8, num_thr=2)) as st:
        info = st.load_fastq(f[0], f[1] if pe else None)
        N = sum(info["num_reads"])
        st.run()
        dnaN, order_N = st.fastq_N(0)
        if pe:
            d2, o2 = st.fastq_N(1)
            dnaN, order_N = dnaN + d2, np.concatenate([order_N, o2 + info["num_reads"][0]]).astype(np.uint32)
        assert len(order_N) > 0
        with EncoderStage() as enc, StreamsStage() as ss, DecodeStage() as ds, QualIdStage() as qa, QualIdStage() as qb:
            enc.encode(st, dnaN, order_N)
            order = enc.streams()["order"].copy()
            ss.from_encoder(enc, N, pe, False, 97)
            ds.seq_from_encoder(enc)
            ds.from_streams(ss)
            qa.set_order_from_encoder(enc, N, pe)
            qb.set_order(order, N, pe)
            for m in range(len(f)):
                decoded = ds.reads(m)
                ia = qa.from_fastq(f[m], num_reads_per_block=97)
                ib = qb.from_fastq(f[m], num_reads_per_block=97)
                assert ia["bytes"] == ib["bytes"] and ia["num_blocks"] == ib["num_blocks"] == (len(decoded) + 96) // 97
                for kind in (qm.QUALITY, qm.ID):
                    a, b = qa.download(kind), qb.download(kind)
                    assert a[0] == b[0] and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])
                quals = [q for blk in qa.blocks(qm.QUALITY) for q in blk]
                assert len(quals) == len(decoded)
                assert [q.translate(TR_BACK).decode() for q in quals] == decoded, m
                # ... and the ids sit in the slots of their reads
                ids, reads, _ = qm.fastq_lines(f[m])
                by_id = dict(zip(ids, reads))
                got_ids = [i for blk in qa.blocks(qm.ID) for i in blk]
                assert [by_id[i].decode() for i in got_ids] == decoded
            assert np.array_equal(enc.streams()["order"], order)   # the encoder's order is as it was


# ---------------------------------------------------------------- paired ids
def _id_files(fmt1, fmt2, n=2000):
    a = [fmt1 % i for i in range(n)]
    b = [fmt2 % i for i in range(n)]
    return a, b


def _fq_ids(ids):
    return b"".join(i + b"\nACGT\n+\nIIII\n" for i in ids)


@pytest.mark.parametrize("fmt1,fmt2,code", [(b"@r%d/1", b"@r%d/2", 1), (b"@SRR.%d x", b"@SRR.%d x", 2),
                                            (b"@M:%d 1:N:0", b"@M:%d 2:N:0", 3)])
def test_id_pattern(fmt1, fmt2, code):
    from spring_amd import QualIdStage
    a, b = _id_files(fmt1, fmt2)
    n = len(a)
    assert QualIdStage.id_pattern(_fq_ids(a), _fq_ids(b)) == code == qm.id_pattern(_fq_ids(a), _fq_ids(b))
    assert QualIdStage.id_pattern(gzip.compress(_fq_ids(a), 1), _fq_ids(b).replace(b"\n", b"\r\n")) == code
    # one pair deep in the file breaks the pattern
    broken = list(b)
    broken[n - 2] = b[n - 2][:-1] + b"7"
    assert QualIdStage.id_pattern(_fq_ids(a), _fq_ids(broken)) == 0 == qm.id_pattern(_fq_ids(a), _fq_ids(broken))
    # ... or has ids of different lengths
    longer = list(b)
    longer[n - 2] = b[n - 2] + b"x"
    assert QualIdStage.id_pattern(_fq_ids(a), _fq_ids(longer)) == 0
    # the first pair decides which pattern is looked for
    first = list(b)
    first[0] = b"@other"
    assert QualIdStage.id_pattern(_fq_ids(a), _fq_ids(first)) == 0


def test_id_pattern_corner_cases():
    from spring_amd import QualIdStage
    from spring_amd.reorder import ReorderError
    for a, b in (([b"@A 1", b"@B 1"], [b"@A 2", b"@B 2"]), ([b"", b""], [b"", b""]), ([b"@A 1:", b""], [b"@A 2:", b""]),
                 ([b"@a/1", b""], [b"@a/2", b""]), ([b"@A x 1:N"], [b"@A x 2:N"]), ([b"@A 1:N "], [b"@A 2:N "])):
        assert QualIdStage.id_pattern(_fq_ids(a), _fq_ids(b)) == qm.id_pattern(_fq_ids(a), _fq_ids(b)), (a, b)
    assert QualIdStage.id_pattern(b"", b"") == 0
    with pytest.raises(ReorderError, match="code -1"):
        QualIdStage.id_pattern(_fq_ids([b"@a", b"@b"]), _fq_ids([b"@a"]))
    with pytest.raises(ReorderError, match="multiple of 4"):
        QualIdStage.id_pattern(_fq_ids([b"@a"]) + b"@b\n", _fq_ids([b"@a"]))


# ---------------------------------------------------------------- refusals
def test_refusals():
    from spring_amd import QualIdStage
    from spring_amd.reorder import ReorderError
    n = 40
    f = synth(4, n)
    ids, reads, quals = qm.fastq_lines(f)
    good = np.random.default_rng(1).permutation(n).astype(np.uint32)
    t = QualIdStage.quality_table("illumina")

    def refused(qs, call, code="code -1"):
        with pytest.raises(ReorderError, match=code):
            call()
        for kind in (0, 1):
            with pytest.raises(ReorderError, match="code -4"):
                qs.download(kind)

    with QualIdStage() as qs:
        # any call before an order is set
        refused(qs, lambda: qs.from_fastq(f), "code -4")
        refused(qs, lambda: qs.from_lines(0, b"II\n"), "code -4")
        # orders: each refusal leaves the context without an order, whatever it held before
        dup = good.copy()
        dup[1] = dup[0]
        big = good.copy()
        big[2] = n
        for order, num, pe in ((dup, n, False), (big, n, False), (dup, n, True), (good[:n - 1] % (n - 1), n - 1, True),
                               (None, n - 1, True)):
            qs.set_order(good, n)
            qs.from_fastq(f)
            refused(qs, lambda: qs.set_order(order, num, pe))
            refused(qs, lambda: qs.from_fastq(f), "code -4")
        qs.set_order(good, n)
        qs.from_fastq(f, num_reads_per_block=3)
        assert qs.download(0)[0] == qm.from_fastq(f, 0, qm.order_array(good, n, False), 3)["bytes"]
        # one line too many / too few, in both input forms
        more = f + b"@x\nAC\n+\nII\n"
        fewer = b"".join(b"%s\n%s\n+\n%s\n" % r for r in list(zip(ids, reads, quals))[:n - 1])
        qimg = b"".join(q + b"\n" for q in quals)
        for call in (lambda: qs.from_fastq(more), lambda: qs.from_fastq(fewer), lambda: qs.from_lines(0, qimg + b"I\n"),
                     lambda: qs.from_lines(0, qimg[:qimg[:-1].rindex(b"\n") + 1]), lambda: qs.from_lines(1, b""),
                     # B = 0
                     lambda: qs.from_fastq(f, num_reads_per_block=0), lambda: qs.from_lines(0, qimg, num_reads_per_block=0),
                     # 4k + 1 lines
                     lambda: qs.from_fastq(f + b"@x\n"), lambda: qs.from_fastq(f + b"@x")):
            qs.from_fastq(f)   # a result that the refused call has to take away
            refused(qs, call)
        # byte 200 in a quality: refused under a table, accepted without one
        k = max(range(n), key=lambda i: len(quals[i]))
        q200 = list(quals)
        q200[k] = q200[k][:5] + b"\xc8" + q200[k][6:]
        f200 = b"".join(b"%s\n%s\n+\n%s\n" % r for r in zip(ids, reads, q200))
        refused(qs, lambda: qs.from_fastq(f200, table=t))
        refused(qs, lambda: qs.from_lines(0, b"".join(q + b"\n" for q in q200), table=t))
        qs.from_fastq(f200, num_reads_per_block=3)
        assert qs.download(0)[0] == qm.from_fastq(f200, 0, qm.order_array(good, n, False), 3)["bytes"]
        qs.from_fastq(f200, want="id", table=t)   # the ids alone never meet the table
        # a quality one byte shorter than its read, whichever kinds are asked for
        short = list(quals)
        short[k] = short[k][:-1]
        fshort = b"".join(b"%s\n%s\n+\n%s\n" % r for r in zip(ids, reads, short))
        for want in (("quality", "id"), "quality", "id"):
            refused(qs, lambda: qs.from_fastq(fshort, want=want))
        with pytest.raises(ReorderError, match="does not match quality length"):
            qs.from_fastq(fshort)
        # and the context still works
        qs.from_fastq(f, num_reads_per_block=3)
        assert qs.download(1)[0] == qm.from_fastq(f, 1, qm.order_array(good, n, False), 3)["bytes"]
