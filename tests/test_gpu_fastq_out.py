"""GPU tests of the FASTQ assembler (include/spring_fastq_out.h) against the checker tests/fastq_out_model.py: text and
record offsets byte for byte over every source / destination misalignment, tiny records, numbered ids, modify_id,
ranges, sources in HBM against sources from the host, the round trip to the FASTQ that went in, refusals, write()."""
import functools
import hashlib
import os
import types

import numpy as np
import pytest

import fastq_out_model as fm
import qualid_model as qm
from helpers import GOLDEN, interleave_order_N, make_N_reads, named_set, read_strings
from oracle import pyoracle as po

pytestmark = pytest.mark.gpu

LENGTHS = (0, 1, 15, 16, 17, 31, 63, 64, 65, 255, 511)
N_REC = 3003   # 273 cycles of LENGTHS
QUAL_BYTES = np.array([c for c in range(1, 256) if c not in (10, 13)], np.uint8)   # bytes pass through unchanged
ID_BYTES = np.array([c for c in range(32, 127)], np.uint8)


@functools.lru_cache(maxsize=None)
def synth(seed, n=N_REC):
    """(ids, reads, quals) of n records (the generator idea of test_gpu_qualid.synth): read lengths cycle through
    LENGTHS, ids of 1 .. 1200 bytes with some of exactly 15, 16, 31 and 32."""
    rng = np.random.default_rng(seed)
    ids, reads, quals = [], [], []
    for i in range(n):
        L = LENGTHS[(i + 3 * seed) % len(LENGTHS)]
        il = {4: 15, 5: 16, 6: 32, 7: 31}.get(i % 97, 1 + (i * 7919 + seed) % 1200)
        ids.append(b"@" + ID_BYTES[rng.integers(0, len(ID_BYTES), il - 1)].tobytes())
        reads.append(np.frombuffer(b"ACGTN", np.uint8)[rng.integers(0, 5, L)].tobytes())
        quals.append(QUAL_BYTES[rng.integers(0, len(QUAL_BYTES), L)].tobytes())
    return ids, reads, quals


@functools.lru_cache(maxsize=None)
def synth_want(seed, quality):
    ids, reads, quals = synth(seed)
    return fm.assemble(ids, reads, quals if quality else None)


def shifted(data, k):
    """data behind k other bytes: the pointer the library gets is k bytes into its buffer."""
    return np.frombuffer(b"\xee" * k + bytes(data), np.uint8)[k:]


def same(fo, want, what=""):
    text, off = fo.download()
    assert np.array_equal(off, want[1]), (what, "rec_off")
    assert text == want[0], (what, "text")
    assert fo.info["bytes"] == len(want[0]) and fo.info["num_units"] == len(want[1]) - 1, what


# ---------------------------------------------------------------- alignments
@pytest.mark.parametrize("quality", [False, True])
def test_alignments(quality):
    from spring_amd import FastqOutStage
    ids, reads, quals = synth(1)
    want = synth_want(1, quality)
    assert {len(i) for i in ids} >= {15, 16, 31, 32, 1, 1200} and len(want[0]) % 16 != 0
    bases, off = fm.reads_image(reads)
    qimg, iimg = b"".join(quals), fm.id_image(ids)
    seen = set()
    with FastqOutStage() as fo:
        for k in range(16):
            kb, ki, kq = k, (3 * k + 1) % 16, (7 * k + 5) % 16
            src = [shifted(bases, kb), shifted(iimg, ki), shifted(qimg, kq)]
            seen.add(tuple(a.ctypes.data % 16 for a in src))
            for B in ((1000, 1 << 30) if k == 0 else (1000,)):
                fo.assemble((src[0], off), N_REC, quality=(src[2], fm.block_table(quals, B, 0)) if quality else None,
                            ids=(src[1], fm.block_table(ids, B, 1)), num_reads_per_block=B)
                same(fo, want, (quality, k, B))
        assert len({s[0] for s in seen}) == len({s[1] for s in seen}) == len({s[2] for s in seen}) == 16
        # without block tables
        fo.assemble((bases, off), N_REC, quality=qimg if quality else None, ids=iimg, num_reads_per_block=1000)
        same(fo, want, "no tables")
        assert fo.info["first_slot"] == 0 and fo.info["ms_device"] > 0


# ---------------------------------------------------------------- many tiny records
@pytest.mark.parametrize("quality", [False, True])
def test_many_tiny_records(quality):
    """Records of 3 and 4 bytes ("@\\n\\n", "@\\nA\\n"): more than 1024 of them in 4 KiB of output, so the copy searches
    the record offsets in memory; with quality 6 and 8 bytes, fewer than 1024: searched in LDS."""
    from spring_amd import FastqOutStage
    n = 40000
    rng = np.random.default_rng(7)
    reads = [b"ACGT"[i % 4:i % 4 + 1] if x else b"" for i, x in enumerate(rng.integers(0, 2, n))]
    quals = [b"I" * len(r) for r in reads]
    ids = [b"@"] * n
    want = fm.assemble(ids, reads, quals if quality else None)
    per4k = np.diff(np.searchsorted(want[1], np.arange(0, len(want[0]), 4096)))
    assert (per4k.min() > 1024) if not quality else (per4k.max() < 1024)
    with FastqOutStage() as fo:
        fo.assemble(fm.reads_image(reads), n, quality=b"".join(quals) if quality else None, ids=fm.id_image(ids),
                    num_reads_per_block=999)
        same(fo, want)


def test_numbered_ids():
    from spring_amd import FastqOutStage
    from spring_amd.reorder import ReorderError
    n, B = 70000, 1000
    reads = [b"ACGTN"[:(i * 7 + i // 11) % 3] for i in range(n)]
    quals = [r.translate(bytes.maketrans(b"ACGTN", b"I5#?!")) for r in reads]
    img = fm.reads_image(reads)
    with FastqOutStage() as fo:
        for mate, pe in ((0, False), (1, True)):
            for q in (None, quals):
                want = fm.assemble(fm.numbered_ids(0, n, mate), reads, q)   # 1 .. 70000: every digit count up to 5
                fo.assemble(img, n * (2 if pe else 1), quality=None if q is None else b"".join(q), preserve_id=False,
                            paired_end=pe, mate=mate, num_reads_per_block=B)
                same(fo, want, (mate, q is None))
        # a window that does not start the file: blocks [9, 12) hold the numbers 9001 .. 12000
        lo, hi = 9 * B, 12 * B
        want = fm.assemble(fm.numbered_ids(lo, hi - lo, 0), reads[lo:hi], quals[lo:hi])
        fo.assemble(fm.reads_image(reads[lo:hi]), n, quality=b"".join(quals[lo:hi]), preserve_id=False,
                    num_reads_per_block=B, first_block=9, num_blocks=3)
        same(fo, want, "window")
        assert want[0].startswith(b"@9001/1\n") and fo.info["first_slot"] == lo
        # ... and a range inside it keeps the global numbers
        fo.assemble(fm.reads_image(reads[lo:hi]), n, quality=b"".join(quals[lo:hi]), preserve_id=False,
                    num_reads_per_block=B, first_block=9, num_blocks=3, unit_range=(998, 1002))
        same(fo, fm.assemble(fm.numbered_ids(lo, hi - lo, 0), reads[lo:hi], quals[lo:hi], (998, 1002)), "window range")
        assert fo.download()[0].startswith(b"@9999/1\n") and fo.info["first_slot"] == lo + 998
        # stored ids together with numbered ids
        with pytest.raises(ReorderError, match="code -1"):
            fo.assemble(img, n, ids=fm.id_image([b"@"] * n), preserve_id=False, num_reads_per_block=B)
        with pytest.raises(ReorderError, match="code -4"):
            fo.download()


# ---------------------------------------------------------------- modify_id
@pytest.mark.parametrize("fmt1,fmt2,code", [(b"@r%d/1", b"@r%d/2", 1), (b"@SRR.%d x", b"@SRR.%d x", 2),
                                            (b"@M:%d 1:N:0", b"@M:%d 2:N:0", 3)])
def test_modify_id_on_the_id_patterns(fmt1, fmt2, code):
    from spring_amd import FastqOutStage
    n = 2000
    ids1, ids2 = [fmt1 % i for i in range(n)], [fmt2 % i for i in range(n)]
    assert qm.find_id_pattern(ids1[0], ids2[0]) == code
    _, reads, quals = synth(2, n)
    with FastqOutStage() as fo:
        for q in (None, quals):
            want = fm.assemble(ids2, reads, q)
            assert want[0] == fm.assemble(ids1, reads, q, paired_id_code=code)[0]
            fo.assemble(fm.reads_image(reads), 2 * n, quality=None if q is None else b"".join(q), ids=fm.id_image(ids1),
                        paired_end=True, mate=1, paired_id_code=code, num_reads_per_block=300)
            same(fo, want, (code, q is None))


def test_modify_id_patch_positions():
    """The one changed byte on every byte of a 16-byte word (0 and 15 among them), on the first byte of the text, in its
    last id byte a text can have (three bytes from its end), and only the first space counts under code 3."""
    from spring_amd import FastqOutStage
    n = 400
    with FastqOutStage() as fo:
        for code in (1, 3):
            # code 1: the id "1" alone puts the patch on byte 0 of the text; code 3: " 1" on byte 1, "@x 1 1" has two spaces
            ids = [b"1"] if code == 1 else [b" 1", b"@x 1 1"]
            ids += [b"@" + b"i" * (k % 23) + (b" 1:N 1" if code == 3 else b"/1") for k in range(n - len(ids) - 1)]
            ids += [b"@last/1" if code == 1 else b"@last 1"]
            reads = [b"ACGT"[:k % 5] for k in range(n - 1)] + [b""]
            want = fm.assemble(ids, reads, paired_id_code=code)
            plain = fm.assemble(ids, reads)
            diff = [i for i in range(len(want[0])) if want[0][i] != plain[0][i]]
            assert len(diff) == n and {d % 16 for d in diff} == set(range(16))
            assert diff[0] == (0 if code == 1 else 1) and diff[-1] == len(want[0]) - 3   # "...2\n\n" ends the text
            if code == 3:
                assert want[0].split(b"\n")[2] == b"@x 2 1"
            fo.assemble(fm.reads_image(reads), 2 * n, ids=fm.id_image(ids), paired_end=True, mate=1, paired_id_code=code,
                        num_reads_per_block=64)
            same(fo, want, code)


# ---------------------------------------------------------------- range
def test_ranges():
    from spring_amd import FastqOutStage
    ids, reads, quals = synth(1)
    B, nu = 1000, N_REC
    img, qimg, iimg = fm.reads_image(reads), b"".join(quals), fm.id_image(ids)
    with FastqOutStage() as fo:
        for quality in (False, True):
            text, off = synth_want(1, quality)
            for a, b in ((0, 0), (0, 1), (nu - 1, nu), (1500, 2700), (nu, nu), (0, nu)):
                info = fo.assemble(img, nu, quality=qimg if quality else None, ids=iimg, num_reads_per_block=B,
                                   unit_range=(a, b))
                got, goff = fo.download()
                assert got == text[int(off[a]):int(off[b])], (quality, a, b)
                assert goff.tolist() == (off[a:b + 1] - off[a]).tolist()
                assert info["num_units"] == b - a and info["first_slot"] == a
                assert (got, goff.tolist()) == (lambda w: (w[0], w[1].tolist()))(
                    fm.assemble(ids, reads, quals if quality else None, (a, b)))


# ---------------------------------------------------------------- the rest of the pipeline
TR = bytes.maketrans(b"ACGTN", b"I5#?!")


def _fastq(ids, reads):
    return b"".join(b"%s\n%s\n+\n%s\n" % (i, r, r.translate(TR)) for i, r in zip(ids, reads))


def _golden(j):
    """The golden file's reads under ids that match by paired id code 1."""
    lines = open(os.path.join(GOLDEN, "test_%d.fastq" % j), "rb").read().split(b"\n")
    reads = [x.strip() for x in lines[1:-1:4]]
    return _fastq([b"@pair.%d/%d" % (i, j) for i in range(len(reads))], reads)


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


B_CHAIN = 97


@pytest.fixture(scope="module", params=["single_end_N", "golden_pe", "golden_pe_preserve_order"])
def chain(request):
    """FASTQ -> reorder -> encoder -> streams -> decode, and the quality / id blocks of every file (the chain of
    test_gpu_qualid.test_quality_lines_follow_the_decoded_reads); everything stays in HBM while the tests look."""
    import spring_amd
    from spring_amd import DecodeStage, QualIdStage, StreamsStage
    from spring_amd.encoder import EncoderStage
    case = request.param
    keep_order = case.endswith("preserve_order")
    f = [_golden(1), _golden(2)] if case.startswith("golden") else [_single_end_with_N()]
    pe = len(f) == 2
    with spring_amd.ReorderStage(spring_amd.ReorderOpts(num_chains=8, num_thr=2, alternatives=1, phases=1)) as st:
        info = st.load_fastq(f[0], f[1] if pe else None)
        N = sum(info["num_reads"])
        st.run()
        dnaN, order_N = st.fastq_N(0)
        if pe:
            d2, o2 = st.fastq_N(1)
            dnaN, order_N = dnaN + d2, np.concatenate([order_N, o2 + info["num_reads"][0]]).astype(np.uint32)
        with EncoderStage() as enc, StreamsStage() as ss, DecodeStage() as ds, QualIdStage() as q0, QualIdStage() as q1:
            enc.encode(st, dnaN, order_N)
            order = enc.streams()["order"].copy()
            ss.from_encoder(enc, N, pe, keep_order, B_CHAIN)
            ds.seq_from_encoder(enc)
            ds.from_streams(ss)
            qs = [q0, q1][:len(f)]
            for m, q in enumerate(qs):
                if keep_order:
                    q.set_order(None, N, pe)
                else:
                    q.set_order_from_encoder(enc, N, pe)
                q.from_fastq(f[m], num_reads_per_block=B_CHAIN)
            yield types.SimpleNamespace(case=case, f=f, pe=pe, N=N, order=None if keep_order else order, ds=ds, qs=qs,
                                        U=N // 2 if pe else N, keep_order=keep_order, enc=enc, ss=ss)


def test_sources_in_hbm_equal_sources_from_the_host(chain):
    from spring_amd import FastqOutStage
    c = chain
    with FastqOutStage() as fo, FastqOutStage() as fh:
        for m in range(len(c.f)):
            before = c.ds.download(m), c.qs[m].download(qm.QUALITY), c.qs[m].download(qm.ID)
            (bases, off), (qb, _, qoff), (ib, _, ioff) = before
            # the decode context's bases have no slack behind them: their last 16-byte word is partial in every case
            assert len(bases) == int(off[-1]) and len(bases) % 16 != 0, (c.case, m, len(bases))
            for quality in (False, True):
                fo.assemble(c.ds, c.N, quality=c.qs[m] if quality else None, ids=c.qs[m], paired_end=c.pe,
                            num_reads_per_block=B_CHAIN, mate=m)
                fh.assemble((bases, off), c.N, quality=(qb, qoff) if quality else None, ids=(ib, ioff), paired_end=c.pe,
                            num_reads_per_block=B_CHAIN, mate=m)
                a, b = fo.download(), fh.download()
                assert a[0] == b[0] and np.array_equal(a[1], b[1]) and len(a[1]) == c.U + 1, (c.case, m, quality)
            full, foff = a
            # the contexts are as they were
            after = c.ds.download(m), c.qs[m].download(qm.QUALITY), c.qs[m].download(qm.ID)
            for x, y in zip(before, after):
                assert x[0] == y[0] and all(np.array_equal(p, q) for p, q in zip(x[1:], y[1:]))
            # a window inside the file: the whole-file contexts are read from the middle, the reads come from the host
            nb = (c.U + B_CHAIN - 1) // B_CHAIN
            assert nb >= 2
            for b0, k in ((1, 1), (nb - 1, 1), (nb // 2, min(3, nb - nb // 2))):
                lo, hi = b0 * B_CHAIN, min((b0 + k) * B_CHAIN, c.U)
                wb, woff = bases[int(off[lo]):int(off[hi])], off[lo:hi + 1] - off[lo]
                fo.assemble((wb, woff), c.N, quality=c.qs[m], ids=c.qs[m], paired_end=c.pe, num_reads_per_block=B_CHAIN,
                            mate=m, first_block=b0, num_blocks=k)
                got, goff = fo.download()
                assert got == full[int(foff[lo]):int(foff[hi])] and goff.tolist() == (foff[lo:hi + 1] - foff[lo]).tolist()
                assert fo.info["first_slot"] == lo


def test_round_trip_to_the_users_file(chain):
    from spring_amd import FastqOutStage
    from spring_amd.order_ops import fastq_reorder
    c = chain
    with FastqOutStage() as fo:
        for m in range(len(c.f)):
            fo.assemble(c.ds, c.N, quality=c.qs[m], ids=c.qs[m], paired_end=c.pe, num_reads_per_block=B_CHAIN, mate=m)
            text, off = fo.download()
            assert b"\r" not in c.f[m]
            if c.order is None:                 # preserve_order: the file that went in
                assert text == c.f[m]
            elif not c.pe:                      # slot i holds record order[i]
                assert text == fastq_reorder(c.f[m], c.order)[0]
            ids, reads, quals = qm.fastq_lines(c.f[m])
            slots = qm.order_array(c.order, c.N, c.pe)
            by_slot = [[None] * c.U for _ in range(3)]
            for j, s in enumerate(slots):
                by_slot[0][s], by_slot[1][s], by_slot[2][s] = ids[j], reads[j], quals[j]
            want = fm.assemble(*by_slot)
            assert text == want[0] and np.array_equal(off, want[1]), (c.case, m)
        if c.pe:   # file 2 from the ids of file 1 (paired id code 1) and its own reads and qualities
            assert qm.id_pattern(c.f[0], c.f[1]) == 1
            fo.assemble(c.ds, c.N, quality=c.qs[1], ids=c.qs[0], paired_end=True, num_reads_per_block=B_CHAIN, mate=1,
                        paired_id_code=1)
            assert fo.download()[0] == text
            fo.assemble(c.ds, c.N, ids=c.qs[0], paired_end=True, num_reads_per_block=B_CHAIN, mate=1, paired_id_code=2)
            assert fo.download()[0] == fm.assemble(by_slot[0], by_slot[1])[0].replace(b"/2\n", b"/1\n")


@pytest.mark.skipif(po.ref_decompress_bin() is None or po.ref_qualid_lib() is None,
                    reason="oracle/_ref/ref_decompress not built (needs the reference sources)")
def test_reference_decompressor_reads_what_the_gpu_wrote(chain):
    """The GPU's own stream blocks, packed consensus and quality / id blocks go to files, through the reference's codecs
    (BSC_compress, reorder_compress_quality_id), and the REAL decompress_short (oracle/_ref/ref_decompress, a CPU child
    process) reads them: the file or files it writes are the text FastqOutStage assembled, and with preserve_order the
    file that went in.  For the pair also with paired_id_match (id_2 not written) over a range."""
    import streams_model as sm
    from spring_amd import FastqOutStage
    c = chain
    nf = len(c.f)
    blocks = {s: c.ss.blocks(s) for s in sm.stream_names(c.pe)}
    lens = c.enc.streams()["seq_len_tid"]
    packed, tails = c.enc.seq_packed()
    cut = np.concatenate([[0], np.cumsum(lens // np.uint64(4))]).astype(int)
    pieces = [(packed[cut[t]:cut[t + 1]], tails[t]) for t in range(len(tails))]
    assert len(pieces) == 2 and cut[-1] == len(packed)
    quals = [[x for blk in c.qs[m].blocks(qm.QUALITY) for x in blk] for m in range(nf)]
    ids = [[x for blk in c.qs[m].blocks(qm.ID) for x in blk] for m in range(nf)]
    with FastqOutStage() as fo:
        gpu = []
        for m in range(nf):
            fo.assemble(c.ds, c.N, quality=c.qs[m], ids=c.qs[m], paired_end=c.pe, num_reads_per_block=B_CHAIN, mate=m)
            gpu.append(fo.download()[0])
        texts, left = po.ref_decompress(blocks, pieces, c.N, c.pe, c.keep_order, B_CHAIN, quality=quals, ids=ids, num_thr=3)
        assert left == [] and len(texts) == nf
        for m in range(nf):
            assert texts[m] == gpu[m], (c.case, m)
            if c.keep_order:
                assert texts[m] == c.f[m]
        if c.pe:
            a, b = B_CHAIN - 3, c.U - 1   # starts inside block 0, ends inside the last block
            assert 0 < a < B_CHAIN < b < c.U
            texts, left = po.ref_decompress(blocks, pieces, c.N, True, c.keep_order, B_CHAIN, quality=quals, ids=ids,
                                            paired_id_code=1, paired_id_match=True, num_thr=1, unit_range=(a, b))
            assert left == []   # both blocks opened; id_2.<b> was never there, so file 2's ids can only be modify_id's
            for m in range(2):
                fo.assemble(c.ds, c.N, quality=c.qs[m], ids=c.qs[0], paired_end=True, num_reads_per_block=B_CHAIN, mate=m,
                            paired_id_code=1 if m else None, unit_range=(a, b))
                assert texts[m] == fo.download()[0], (c.case, m, "paired_id_match")


# ---------------------------------------------------------------- refusals
def test_refusals():
    from spring_amd import DecodeStage, FastqOutStage, QualIdStage
    from spring_amd.reorder import ReorderError
    n, B = 40, 16
    ids, reads, quals = synth(4, n)
    img, qimg, iimg = fm.reads_image(reads), b"".join(quals), fm.id_image(ids)
    qtab, itab = fm.block_table(quals, B, 0), fm.block_table(ids, B, 1)
    want = fm.assemble(ids, reads, quals)

    with FastqOutStage() as fo:
        def refused(call, code="code -1", match=None):
            fo.assemble(img, n, quality=(qimg, qtab), ids=(iimg, itab), num_reads_per_block=B)   # a result to take away
            same(fo, want)
            with pytest.raises(ReorderError, match=code) as e:
                call()
            assert match is None or match in str(e.value)
            with pytest.raises(ReorderError, match="code -4"):   # download after a refusal
                fo.download()
            with pytest.raises(ReorderError, match="code -4"):
                fo.write(os.devnull)

        def go(reads=img, num_reads=n, **kw):
            kw.setdefault("quality", qimg)
            kw.setdefault("ids", iimg)
            kw.setdefault("num_reads_per_block", B)
            return lambda: fo.assemble(reads, num_reads, **kw)

        # a quality total off by one byte in either direction
        refused(go(quality=qimg + b"I"), match="quality lines hold")
        refused(go(quality=qimg[:-1]), match="quality lines hold")
        # block tables that do not match: a unit moved across a block boundary, a table that does not span or decreases
        moved = qtab.copy()
        moved[1] -= 1
        refused(go(quality=(qimg, moved)), match="quality block table")
        imoved = itab.copy()
        imoved[2] += 1
        refused(go(ids=(iimg, imoved)), match="id block table")
        refused(go(quality=(qimg, qtab + np.uint64(1))), match="does not span")
        refused(go(ids=(iimg, itab[[0, 2, 1, 3]])), match="not monotone")
        # an id buffer one line short, one line long, without the final newline
        refused(go(ids=fm.id_image(ids[:-1])), match="lines")
        refused(go(ids=iimg + b"@x\n"), match="lines")
        refused(go(ids=iimg[:-1]))
        refused(go(ids=iimg[:-1] + b"\n@x"), match="do not end in a newline")
        # modify_id: code 1 on an empty id, code 3 without a space or with a trailing one, code 4, mate 0
        pair = dict(num_reads=2 * n, paired_end=True, mate=1)
        empty = fm.id_image(ids[:7] + [b""] + ids[8:])
        spaced = [b"@s%d 1:N" % i for i in range(n)]
        refused(go(ids=empty, paired_id_code=1, **pair), match="code 1 on an empty id")
        refused(go(ids=fm.id_image(spaced[:30] + [b"@nospace"] + spaced[31:]), paired_id_code=3, **pair), match="code 3")
        refused(go(ids=fm.id_image(spaced[:39] + [b"@trailing "]), paired_id_code=3, **pair), match="code 3")
        refused(go(ids=fm.id_image(spaced), paired_id_code=4, **pair), match="Invalid paired id code")
        refused(go(ids=fm.id_image(spaced), paired_id_code=0, **pair), match="Invalid paired id code")
        refused(go(ids=fm.id_image(spaced), paired_id_code=3, num_reads=2 * n, paired_end=True, mate=0))
        fo.assemble(img, 2 * n, quality=qimg, ids=fm.id_image(spaced), paired_id_code=3, num_reads_per_block=B,
                    paired_end=True, mate=1)
        same(fo, fm.assemble(spaced, reads, quals, paired_id_code=3))
        fo.assemble(img, 2 * n, quality=qimg, ids=empty, paired_id_code=2, num_reads_per_block=B, paired_end=True, mate=1)
        # mate 1 of single-end data, from the host and from a decode
        refused(go(mate=1), match="mate 1 of single-end")
        # read offsets that decrease or do not start at 0
        bad = img[1].copy()
        bad[5], bad[6] = bad[6], bad[5]
        assert bad[5] > bad[6]
        refused(go(reads=(img[0], bad)), match="read offsets")
        refused(go(reads=(b"A" + img[0], img[1] + np.uint64(1)), quality=b"I" + qimg), match="read offsets")
        # windows, ranges, sources
        refused(go(first_block=2, num_blocks=2), match="outside the file")
        refused(go(unit_range=(3, n + 1)), match="outside the window")
        refused(go(unit_range=(5, 4)), match="outside the window")
        refused(go(num_reads_per_block=0))
        refused(go(ids=None), match="no id source")
        refused(go(reads=None), "code -4", match="no reads")
        # contexts without a result, or of another shape
        with DecodeStage() as ds, QualIdStage() as qs:
            refused(go(reads=ds), "code -4", match="nothing decoded")
            refused(go(reads=ds, mate=1, num_reads=2 * n, paired_end=True), "code -4")
            refused(go(quality=qs), "code -4")
            refused(go(ids=qs), "code -4")
            f = b"".join(b"%s\n%s\n+\n%s\n" % r for r in zip(ids, reads, [q.replace(b"\r", b"!") for q in quals]))
            qs.set_order(None, n)
            qs.from_fastq(f, want="id", num_reads_per_block=B)
            refused(go(quality=qs), "code -4", match="no quality blocks")
            fo.assemble(img, n, quality=qimg, ids=qs, num_reads_per_block=B)
            same(fo, want, "ids from the context")
            refused(go(ids=qs, num_reads_per_block=B + 1), match="in blocks of")
            refused(go(ids=qs, num_reads=n - 1, reads=fm.reads_image(reads[:-1]),
                       quality=b"".join(quals[:-1])), match="units in blocks of")
        # and the context still works
        fo.assemble(img, n, quality=(qimg, qtab), ids=(iimg, itab), num_reads_per_block=B)
        same(fo, want)


# ---------------------------------------------------------------- write()
def test_write(tmp_path):
    from spring_amd import FastqOutStage
    from spring_amd.reorder import ReorderError
    ids, reads, quals = synth(1)
    B = 1000
    text, off = synth_want(1, True)
    with FastqOutStage() as fo:
        fo.assemble(fm.reads_image(reads), N_REC, quality=b"".join(quals), ids=fm.id_image(ids), num_reads_per_block=B)
        p = tmp_path / "whole.fastq"
        p.write_bytes(b"something longer than nothing" * 3)
        info = fo.write(p)
        assert p.read_bytes() == fo.download()[0] == text and info["ms_file"] > 0 and info["bytes"] == len(text)
        # two windows, the second appended
        p2 = tmp_path / "windows.fastq"
        for b0, k in ((0, 2), (2, 2)):
            lo, hi = b0 * B, min((b0 + k) * B, N_REC)
            fo.assemble(fm.reads_image(reads[lo:hi]), N_REC, quality=b"".join(quals[lo:hi]), ids=fm.id_image(ids[lo:hi]),
                        num_reads_per_block=B, first_block=b0, num_blocks=k)
            fo.write(p2, append=b0 > 0)
        assert p2.read_bytes() == text
        # an empty text writes an empty file
        fo.assemble(fm.reads_image(reads), N_REC, quality=b"".join(quals), ids=fm.id_image(ids), num_reads_per_block=B,
                    unit_range=(7, 7))
        fo.write(p2)
        assert p2.read_bytes() == b"" and fo.download()[0] == b""
        with pytest.raises(ReorderError, match="code -2"):
            fo.write(tmp_path / "no_such_directory" / "x.fastq")
        assert fo.download()[1].tolist() == [0]   # an unwritable path leaves the result


# ---------------------------------------------------------------- one sized test
def test_two_million_reads():
    from spring_amd import FastqOutStage
    n, L = 2_000_000, 150
    rng = np.random.default_rng(150)
    base = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, 1 << 20, dtype=np.uint8)]
    bb = np.lib.stride_tricks.sliding_window_view(base, L)[rng.integers(0, (1 << 20) - L, n)].tobytes()
    qb = bb.translate(TR)
    ids = [b"@r.%d" % i for i in range(n)]
    want = fm.assemble(ids, [bb[i:i + L] for i in range(0, n * L, L)], [qb[i:i + L] for i in range(0, n * L, L)])
    with FastqOutStage() as fo:
        info = fo.assemble((bb, np.arange(n + 1, dtype=np.uint64) * np.uint64(L)), n, quality=qb, ids=fm.id_image(ids))
        print("2M x 150: %d bytes, ms_device %.3f (%.1f GB/s written)" % (info["bytes"], info["ms_device"],
                                                                      info["bytes"] / info["ms_device"] / 1e6))
        got = fo.download_array()
        assert info["bytes"] == len(want[0]) and np.array_equal(fo.download(text=False)[1], want[1])
        assert hashlib.blake2b(got).digest() == hashlib.blake2b(want[0]).digest()
