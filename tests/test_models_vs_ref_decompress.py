"""The two checkers of the decompression side -- tests/streams_model.py::read_block (the reader the decoder tests compare
decode.hip with) and tests/fastq_out_model.py (numbered ids, modify_id, the start_num / end_num cut, two-line records,
block windows) -- against the REFERENCE'S OWN decompress_short, built whole by oracle/Makefile into
oracle/_ref/ref_decompress (decompress.cpp where it lies; write_fastq_block by line range without its gzip branch).

Every case runs the reference's writers first (ref_streams = reorder_compress_streams, libref_qualid.so =
reorder_compress_quality_id, the real BSC_compress on the blocks and on the packed consensus), then the reference's
decompressor, and compares the file or files it wrote byte for byte with fm.assemble(ids, sm.read_block(...), quals, ...)
and the set of files it left with the blocks the range does not reach.  Skipped where oracle/_ref is not built.

One divergence is kept, and named here as in tests/test_gpu_decode.py: without preserve_order, a block that opens with an
unaligned read 1 and holds an aligned read 1 later.  The real writer stores that position as a u16 delta against 0
(reorder_compress_streams.cpp:312-328), the real reader takes a block's first read 1 position as a u64
(decompress.cpp:240-245) and so reads past it: the reference cannot decompress what it wrote (real data never has such a
block, :241-242).  read_block is the reader restated and refuses such a block (its streams are not consumed exactly);
the cases below assert that refusal and run the reference on the blocks around it (`quirk_blocks`).

A second divergence was found by these tests and is kept: empty quality lines at the END of a block.  The reference's
BSC_str_array_decompress stops when the block's last byte is placed (bsc_str_array.cpp:149-162: write_str_array resizes a
string only when it moves on to it with bytes left; :472 resizes string 0), so the empty lines after the last non-empty
one are never cleared and decompress_short writes whatever quality_array held there before: file 1's quality of the
same unit when it writes file 2, the previous step's otherwise (decompress.cpp:92-93, :364-371).  The record then carries
a quality line longer than its (empty) read.  The model and FastqOutStage write the empty line; `stale_quality` restates
what the reference leaves there and the expected text is patched with it, nothing else (`STALE_SEEN` shows it happens)."""
import numpy as np
import pytest

import decode_cases as dc
import fastq_out_model as fm
import ref_cases as rc
import streams_model as sm
from helpers import decode_reads
from oracle import pyoracle as po

pytestmark = pytest.mark.skipif(po.ref_decompress_bin() is None or po.ref_streams_bin() is None or po.ref_qualid_lib() is None,
                                reason="oracle/_ref/ref_decompress not built (needs the reference sources)")

BIG = 1 << 30


def quirk_blocks(flag_blocks, preserve_order):
    """The blocks of the kept divergence, from their flags: without preserve_order, a block whose first read 1 is unaligned
    (flag 2 or 4) and which holds an aligned read 1 (flag 0, 1 or 3) later."""
    if preserve_order:
        return []
    return [k for k, f in enumerate(flag_blocks) if f[:1] in (b"2", b"4") and set(f) & set(b"013")]


def model_reads(blocks, seq, U, pe, preserve_order, B):
    """read_block on every block -> per block the list of units' reads, None where the reader refuses the block."""
    out = []
    for b in range(len(blocks["read_flag.txt"])):
        nu = min(B, U - b * B)
        try:
            out.append(sm.read_block({s: v[b] for s, v in blocks.items()}, seq, nu, pe, preserve_order))
        except (AssertionError, IndexError, KeyError):
            out.append(None)
    return out


def files_before(pe, nb, T, quality, ids, match):
    names = ["%s.%d.bsc" % (s, b) for s in sm.stream_names(pe) for b in range(nb)]
    for m in range(2 if pe else 1):
        if quality:
            names += ["quality_%d.%d" % (m + 1, b) for b in range(nb)]
        if ids and not (m == 1 and match):
            names += ["id_%d.%d" % (m + 1, b) for b in range(nb)]
    return names


def same_output(blocks, seq, N, pe, preserve_order, B, T=1, num_thr=1, unit_range=None, ids=None, quality=None, code=None,
                what="", by_block=None):
    """One run of the real decompress_short against the two models.  ids / quality: [file 1's lines, file 2's] in slot
    order or None; code: paired_id_match with that paired id code.  -> the texts."""
    U = N // 2 if pe else N
    a, b = (0, U) if unit_range is None else unit_range
    nb = (U + B - 1) // B
    texts, left = po.ref_decompress(blocks, rc.seq_pieces(seq, T), N, pe, preserve_order, B, quality=quality, ids=ids,
                                    paired_id_code=code or 0, paired_id_match=code is not None, num_thr=num_thr,
                                    unit_range=(a, b))
    used = rc.consumed_blocks(U, B, num_thr, a, b)
    assert used == list(range(used[0], used[-1] + 1)) and used[0] == a // B and used[-1] >= (b - 1) // B, what
    # the files left: every block outside the steps the range touches, still compressed; nothing else
    gone = {n for n in files_before(pe, nb, T, quality, ids, code is not None) if int(n.split(".")[2 if n[0] == "r" else 1]) in used}
    assert left == sorted(set(files_before(pe, nb, T, quality, ids, code is not None)) - gone), what
    # the text: the window of blocks the reference opened, through read_block and assemble
    if by_block is None:
        by_block = model_reads(blocks, seq, U, pe, preserve_order, B)
    lo, hi = used[0] * B, min((used[-1] + 1) * B, U)
    stale = {} if quality is None else stale_quality(quality, U, B, num_thr, pe, used)
    assert all(by_block[k] is not None for k in used), (what, "the range touches a block the reader refuses")
    units = [u for k in used for u in by_block[k]]
    assert len(units) == hi - lo
    for m in range(2 if pe else 1):
        reads = [(u[m] if pe else u).encode() for u in units]
        q = None if quality is None else quality[m][lo:hi]
        if ids is None:
            i_, c_ = fm.numbered_ids(lo, hi - lo, m), None
        elif m == 1 and code is not None:
            i_, c_ = ids[0][lo:hi], code
        else:
            i_, c_ = ids[m][lo:hi], None
        want, off = fm.assemble(i_, reads, q, (a - lo, b - lo), c_)
        assert len(off) == b - a + 1 and int(off[-1]) == len(want)
        assert texts[m] == with_stale(want, off, a, m, stale), (what, m, "window of blocks")
        if all(x is not None for x in by_block):   # ... and the same cut out of the whole file
            every = [(u[m] if pe else u).encode() for blk in by_block for u in blk]
            if ids is None:
                i_ = fm.numbered_ids(0, U, m)
            elif m == 1 and code is not None:
                i_ = ids[0]
            else:
                i_ = ids[m]
            want, off = fm.assemble(i_, every, None if quality is None else quality[m], (a, b), c_)
            assert texts[m] == with_stale(want, off, a, m, stale), (what, m, "file")
    return texts


STALE_SEEN = set()


def stale_quality(quality, U, B, num_thr, pe, used):
    """-> {(file, unit): line} for the units whose quality line the reference does not set (see the module's docstring):
    the contents of decompress_short's quality_array over the steps that open the blocks `used`."""
    arr, out = {}, {}
    for s in range(0, len(used), num_thr):
        for m in range(2 if pe else 1):
            for t, blk in enumerate(used[s:s + num_thr]):
                lines = quality[m][blk * B:min((blk + 1) * B, U)]
                last = max([i for i, x in enumerate(lines) if x] or [0])
                for i, x in enumerate(lines):
                    if i <= last:
                        arr[(t, i)] = x
                    elif arr.get((t, i), b""):
                        out[(m, blk * B + i)] = arr[(t, i)]
    return out


def with_stale(text, off, first_unit, m, stale):
    """The records of `text` (units first_unit ...) with the empty quality lines the reference leaves stale replaced."""
    recs = [text[int(off[i]):int(off[i + 1])] for i in range(len(off) - 1)]
    for i, r in enumerate(recs):
        q = stale.get((m, first_unit + i))
        if q is not None:
            assert r.endswith(b"\n\n+\n\n")   # an empty read, an empty quality line
            recs[i] = r[:-1] + q + b"\n"
            STALE_SEEN.add(len(q))
    return b"".join(recs)


def lines_of(reads, U, pe, form, quality=True):
    nf = 2 if pe else 1
    ids = None if form is None else [rc.ids_for(form, U, m) for m in range(nf)]
    quals = [rc.quality_for(reads[m * U:(m + 1) * U], m) for m in range(nf)] if quality else None
    return ids, quals


def runs_of_readable(by_block):
    """Maximal runs [b0, b1) of blocks the reader takes."""
    out, b0 = [], None
    for k, x in enumerate(list(by_block) + [None]):
        if x is not None and b0 is None:
            b0 = k
        if x is None and b0 is not None:
            out.append((b0, k))
            b0 = None
    return out


def whole_or_around_the_quirk(name, enc, seq, N, reads, pe, preserve_order, B, T, form, thrs=(1, 3), **kw):
    """The whole file at each decompressor thread count; where QUIRK names blocks the reader cannot take, the model must
    refuse exactly those and the reference runs, one block per step, on each run of blocks between them."""
    U = N // 2 if pe else N
    blocks, _ = po.ref_streams(enc, N, pe, preserve_order, B, T)
    by_block = model_reads(blocks, seq, U, pe, preserve_order, B)
    bad = quirk_blocks(blocks["read_flag.txt"], preserve_order)
    assert [k for k, x in enumerate(by_block) if x is None] == bad, (name, B)
    ids, quals = lines_of(reads, U, pe, form, kw.pop("quality", True))
    if not bad:
        got = [r for blk in by_block for r in blk]
        assert ([g[0] for g in got] + [g[1] for g in got] if pe else got) == reads, (name, B)
        for num_thr in thrs:
            same_output(blocks, seq, N, pe, preserve_order, B, T, num_thr, None, ids, quals, what=(name, B, num_thr),
                        by_block=by_block, **kw)
        return []
    assert runs_of_readable(by_block)
    for b0, b1 in runs_of_readable(by_block):
        same_output(blocks, seq, N, pe, preserve_order, B, T, 1, (b0 * B, min(b1 * B, U)), ids, quals, what=(name, B, b0, b1),
                    by_block=by_block, **kw)
    return bad


# ---------------------------------------------------------------- the inputs the suite already has
@pytest.mark.parametrize("case", sorted(rc.STREAM_FIXTURES))
def test_stream_fixture_cases(case):
    """tests/ref_cases.py::STREAM_FIXTURES (deltas, gaps, decreasing, mixed, pair distances, flags, corner cases) at their
    block size: read_block + assemble against the file the real decompressor writes, one and three blocks per step, three
    encoder threads (so three read_seq.bin.<t> pieces); lengths 0 and 511 with quality lines of those lengths, N in
    unaligned reads, noise that fills a read on both strands (se_deltas, pe_flags)."""
    enc, seq, N, reads, pe, preserve_order, B = rc.stream_fixture_inputs(case)
    name = case[:case.index("_B")].replace("_po", "")
    form = sorted(rc.ID_FORMS)[len(case) % 3]
    bad = whole_or_around_the_quirk(name, enc, seq, N, reads, pe, preserve_order, B, 3, form)
    assert bool(bad) == (case in ("pe_corner_B3", "pe_flags_B3"))   # the two test_gpu_decode.QUIRK names


@pytest.mark.parametrize("name", ["se_all_aligned", "se_all_unaligned", "pe_all_aligned", "pe_all_unaligned"])
@pytest.mark.parametrize("preserve_order", [False, True])
def test_all_aligned_and_all_unaligned(name, preserve_order):
    """No unaligned read at all (read_unaligned.txt.<b> empty), no aligned one (every other stream but flags and
    lengths empty; every block opens with a singleton); a last block of one unit."""
    make, pe, _ = rc.STREAM_EDGES[name]
    seq = rc.consensus()
    enc, N, reads = rc.make_enc(make(), seq, shuffle=pe or preserve_order)
    U = N // 2 if pe else N
    B = [B for B in range(2, U) if U % B == 1][-1]
    whole_or_around_the_quirk(name, enc, seq, N, reads, pe, preserve_order, B, 1, "srr", thrs=(3,))


@pytest.mark.parametrize("pe", [False, True])
@pytest.mark.parametrize("preserve_order", [False, True])
@pytest.mark.parametrize("B", [1, 3, 4, 7, BIG])
def test_corner_case_block_sizes(pe, preserve_order, B):
    """streams_model.corner_case at B = 1, 3, 4, 7 (a last block of one unit: 8 units) and 2^30; encoder num_thr 1 and 3."""
    enc, seq, N, reads = sm.corner_case(pe, shuffle=pe or preserve_order)
    whole_or_around_the_quirk("pe_corner" if pe else "se_corner", enc, seq, N, reads, pe, preserve_order, B,
                              3 if B in (3, 7) else 1, "r", thrs=(3,) if B in (1, 4) else (1,))


@pytest.mark.parametrize("name", sorted(dc.escape_cases()))
@pytest.mark.parametrize("B", [3, BIG])
def test_escape_cases(name, B):
    enc, seq, N, reads = dc.custom_case(dc.escape_cases()[name], unaligned=("ACGTN" * 3, ""))
    assert dc.writer_escapes(enc, N, BIG) > 0
    whole_or_around_the_quirk(name, enc, seq, N, reads, False, False, B, 1, "illumina", thrs=(1,) if B == 3 else (3,))


@pytest.mark.parametrize("preserve_order", [False, True])
def test_each_flag_opens_a_block(preserve_order):
    """pe_flags at B = 1: the flags 4 0 3 1 2 0 2 4 1 3 each open (and fill) a block, in both order modes; at B = 2 the
    blocks are 40 31 20 24 13, of which 40 and 20 are the kept divergence and 24 is a block that opens with a singleton
    and holds singletons only."""
    seq = rc.consensus()
    enc, N, reads = rc.make_enc(rc.pe_flags(), seq, shuffle=True)
    assert sm.write_streams(enc, N, True, preserve_order, 1)["read_flag.txt"][0] == b"4031202413"
    whole_or_around_the_quirk("pe_flags", enc, seq, N, reads, True, preserve_order, 1, 1, "srr", thrs=(3,))
    whole_or_around_the_quirk("pe_flags", enc, seq, N, reads, True, preserve_order, 2, 3, "srr", thrs=(1,))


def test_block_that_opens_with_a_singleton():
    """decompress.cpp:240-250 without preserve_order: blocks 4 2 4 / 2 4 2 hold no aligned read 1, so their read_pos.bin
    holds read 2 positions (u64) only and first_read_of_block is never cleared."""
    seq = rc.consensus()
    enc, N, reads = rc.make_enc(rc.pe_singleton_open(), seq, shuffle=True)
    assert sm.blocks_of(sm.write_streams(enc, N, True, False, 3))["read_flag.txt"] == [b"424", b"013", b"242", b"1"]
    whole_or_around_the_quirk("pe_singleton_open", enc, seq, N, reads, True, False, 3, 3, "illumina")


# ---------------------------------------------------------------- modes
@pytest.mark.parametrize("name,pe,preserve_order,B", [("se_deltas", False, False, 4), ("se_mixed", False, True, 4),
                                                      ("pe_singleton_open", True, False, 3), ("pe_flags", True, True, 4)])
@pytest.mark.parametrize("quality", [False, True])
def test_numbered_ids_and_two_line_records(name, pe, preserve_order, B, quality):
    """preserve_id off: "@<slot + 1>/<mate + 1>" across the digit change 9 -> 10 and across block edges (10 or 11 units),
    one and three blocks per step; preserve_quality off: two-line records; single and paired end, both order modes."""
    make = rc.pe_singleton_open if name == "pe_singleton_open" else rc.STREAM_EDGES[name][0]
    seq = rc.consensus()
    enc, N, reads = rc.make_enc(make(), seq, shuffle=pe or preserve_order)
    U = N // 2 if pe else N
    assert U >= 10 and U > 2 * B
    blocks, _ = po.ref_streams(enc, N, pe, preserve_order, B, 1)
    _, quals = lines_of(reads, U, pe, None, quality)
    for num_thr in (1, 3):
        texts = same_output(blocks, seq, N, pe, preserve_order, B, 1, num_thr, None, None, quals, what=(name, num_thr))
        for m, t in enumerate(texts):
            lines = t.split(b"\n")[:-1]
            per = 4 if quality else 2
            assert len(lines) == per * U and lines[0] == b"@1/%d" % (m + 1) and lines[per * 9] == b"@10/%d" % (m + 1)
            assert (lines[2::4] == [b"+"] * U) if quality else all(x[:1] != b"+" for x in lines)


# ---------------------------------------------------------------- paired id codes
@pytest.mark.parametrize("form,code", [("srr", 1), ("r", 2), ("illumina", 3), ("two_spaces", 3), ("one_char", 1)])
def test_paired_id_match(form, code):
    """paired_id_match: id_2 is not read (it is not there) and modify_id turns file 1's ids into file 2's: code 1 the
    last character, code 2 nothing, code 3 the character after the FIRST space (an id with two spaces); code 1 on ids of
    one character."""
    seq = rc.consensus()
    enc, N, reads = rc.make_enc(rc.pe_pairdist(), seq, shuffle=True)
    U = N // 2
    blocks, _ = po.ref_streams(enc, N, True, False, 4, 1)
    quals = lines_of(reads, U, True, None)[1]
    if form == "one_char":
        ids = [[b"1"] * U, [b"2"] * U]
    else:
        ids = [rc.ids_for(form, U, m) for m in range(2)]
    texts = same_output(blocks, seq, N, True, False, 4, 1, 3 if code == 3 else 1, None, ids, quals, code, what=(form, code))
    assert not STALE_SEEN or all(quals[1])   # (this case has no empty line: the texts below are the model's as they are)
    assert texts[0].split(b"\n")[0::4][:-1] == ids[0] and texts[1].split(b"\n")[0::4][:-1] == ids[1]
    if form == "two_spaces":
        assert ids[1][0].count(b" ") == 2 and ids[1][0].endswith(b" 1")


def test_no_paired_id_match_reads_id_2():
    """Without paired_id_match id_2.<b> is read, whatever paired_id_code says: file 2's ids here are of another form
    than file 1's, so no modify_id gives them."""
    seq = rc.consensus()
    enc, N, reads = rc.make_enc(rc.pe_pairdist(), seq, shuffle=True)
    U = N // 2
    blocks, _ = po.ref_streams(enc, N, True, True, 4, 1)
    quals = lines_of(reads, U, True, None)[1]
    ids = [rc.ids_for("srr", U, 0), rc.ids_for("illumina", U, 1)]
    texts, left = po.ref_decompress(blocks, rc.seq_pieces(seq, 1), N, True, True, 4, quality=quals, ids=ids, paired_id_code=1,
                                    paired_id_match=False, num_thr=3)
    assert left == []
    assert texts == same_output(blocks, seq, N, True, True, 4, 1, 3, None, ids, quals, None)
    assert texts[1].split(b"\n")[0::4][:-1] == ids[1]


# ---------------------------------------------------------------- ranges
RANGE_CASES = {
    # name -> (slots, paired_end, preserve_order, B, id form or None = numbered); 11 and 10 units: blocks 3 3 3 2 / 3 3 3 1
    "se": (rc.se_mixed, False, True, 3, "srr"),
    "pe_numbered": (rc.pe_flags, True, True, 3, None),
    "pe_code3": (rc.pe_singleton_open, True, False, 3, ("two_spaces", 3)),
}


def _ranges(name, U):
    out = [(4, 6),               # both ends inside one block
           (3, 9), (0, 3),       # start on a block edge and end on one
           (2, 10),              # start and end in different steps, at one block per step and at three (a step = 9 units)
           (0, U)]
    if name != "pe_code3":
        out += [(4, 5),          # one unit
                (7, U), (1, 8)]  # end_num == units; different steps at one block per step only
    return out


@pytest.mark.slow   # (2 s a case; the six together are a quarter of this module's time)
@pytest.mark.parametrize("name", sorted(RANGE_CASES))
@pytest.mark.parametrize("num_thr", [1, 3])
def test_ranges(name, num_thr):
    """0 <= start_num < end_num <= units (what spring.cpp:352-358 lets through).  `shift` applies to the first step only
    (decompress.cpp:123-126, :402-419); the ids keep their global numbers; both files of a pair; the blocks of the steps
    the range does not reach stay on disk."""
    make, pe, preserve_order, B, idsrc = RANGE_CASES[name]
    seq = rc.consensus()
    enc, N, reads = rc.make_enc(make(), seq, shuffle=True)
    U = N // 2 if pe else N
    blocks, _ = po.ref_streams(enc, N, pe, preserve_order, B, 1)
    by_block = model_reads(blocks, seq, U, pe, preserve_order, B)
    form, code = idsrc if isinstance(idsrc, tuple) else (idsrc, None)
    ids, quals = lines_of(reads, U, pe, form)
    seen = set()
    for a, b in _ranges(name, U):
        t = same_output(blocks, seq, N, pe, preserve_order, B, 1, num_thr, (a, b), ids, quals, code, what=(name, a, b, num_thr),
                        by_block=by_block)
        assert t[0].count(b"\n") == 4 * (b - a)
        if ids is None:
            assert t[0].startswith(b"@%d/1\n" % (a + 1)) and (t[1].startswith(b"@%d/2\n" % (a + 1)))
        used = rc.consumed_blocks(U, B, num_thr, a, b)
        seen.add((a % B != 0, len(used) > num_thr))   # (a shift, more than one step)
    assert seen == {(False, False), (True, False), (False, True), (True, True)}


def test_refused_ranges_never_reach_the_reference():
    """The driver lets through what spring.cpp:352-358 does: an empty or reversed range or one past the end exits with 2
    before decompress_short runs (its `end_num - num_reads_done` would wrap)."""
    import subprocess
    for a, b in ((3, 3), (5, 4), (0, 9), (8, 9)):
        argv = [po.ref_decompress_bin(), "run", "/nonexistent", "/nonexistent/1", "/nonexistent/2", "8", "0", "0", "1", "1", "0",
                "0", "3", "1", "1", str(a), str(b)]
        assert subprocess.run(argv, stderr=subprocess.DEVNULL).returncode == 2


# ---------------------------------------------------------------- encoder-made sets
@pytest.mark.parametrize("name,pe", [("var2k", False), ("test_1+2", True), ("syn2k_100", True)])
@pytest.mark.parametrize("preserve_order", [False, True])
def test_encoder_made(name, pe, preserve_order):
    """About 2 100 reads with N reads, B = 97, three encoder threads, three blocks per step: the models, the original
    reads, and helpers.decode_reads (the decompressor's inverse as tests/test_oracle_encoder.py and the encoder's GPU
    tests use it) against the reads of the real decompressor's output."""
    from test_streams_cpu import encoded, slot_order, with_order
    enc, orig, N = encoded(name)
    e = with_order(enc, slot_order(enc, pe, preserve_order))
    seq = enc["seq"].decode()
    U = N // 2 if pe else N
    blocks, _ = po.ref_streams(e, N, pe, preserve_order, 97, 3)
    texts = same_output(blocks, seq, N, pe, preserve_order, 97, 3, 3, None, None, None, what=name)
    got = [x.decode() for t in texts for x in t.split(b"\n")[1::2]]
    slot = np.asarray(e["order"]) if (pe or preserve_order) else np.arange(N)
    for k in range(N):   # slot slot[k] holds record k, i.e. original read enc["order"][k]
        assert got[int(slot[k])] == orig[int(enc["order"][k])], k
    if preserve_order:
        assert got == orig
    dec = decode_reads(enc)   # {original index: read} of the aligned records
    assert len(dec) == len(enc["pos"]) and (len(dec) > 0 or name == "test_1+2")   # (that set's reads are all singletons)
    where = {int(enc["order"][k]): int(slot[k]) for k in range(N)}
    for o, r in dec.items():
        assert got[where[o]] == r, o


# ---------------------------------------------------------------- the recorded fixtures (tests/golden/ref_decomp_*.npz)
@pytest.mark.parametrize("case", sorted(rc.DECOMP_FIXTURES))
def test_decomp_fixture_holds_its_case_and_is_what_the_reference_writes(case):
    """The file holds the inputs tests/ref_cases.py builds; the reference's writer and decompressor, run again, give the
    stored blocks and texts; and the models give them too."""
    g = rc.load_decomp_fixture(case)
    i = rc.decomp_fixture_inputs(case)
    for k in ("seq", "N", "pe", "preserve_order", "B", "ids", "quality", "code"):
        assert g[k] == i[k], k
    assert g["ranges"] == [tuple(r) for r in i["ranges"]] and sorted(g["text"]) == sorted(g["ranges"])
    blocks, _ = po.ref_streams(i["enc"], i["N"], i["pe"], i["preserve_order"], i["B"], i["T"])
    assert sorted(blocks) == sorted(g["streams"])
    for s, (data, off) in g["streams"].items():
        assert b"".join(blocks[s]) == data and np.diff(off.astype(np.int64)).tolist() == [len(x) for x in blocks[s]], s
    for (a, b, num_thr), texts in g["text"].items():
        got = same_output(blocks, i["seq"], i["N"], i["pe"], i["preserve_order"], i["B"], i["T"], num_thr, (a, b), i["ids"],
                          i["quality"], i["code"], what=(case, a, b))
        assert got == texts, (case, a, b)
        if i["quality"] is not None:   # no record of the kept divergence in a fixture: the GPU tests compare as is
            U = i["N"] // 2 if i["pe"] else i["N"]
            assert not stale_quality(i["quality"], U, i["B"], num_thr, i["pe"], rc.consumed_blocks(U, i["B"], num_thr, a, b))


def test_fixtures_hold_the_cases_named():
    """What the stored cases cover, read off the stored reference texts themselves."""
    seen = set()
    for case in rc.DECOMP_FIXTURES:
        g = rc.load_decomp_fixture(case)
        U = g["N"] // 2 if g["pe"] else g["N"]
        seen.add(("pe" if g["pe"] else "se", "po" if g["preserve_order"] else "any"))
        seen.add("code %s" % g["code"])
        seen.add("quality" if g["quality"] is not None else "two-line records")
        for (a, b, num_thr), texts in g["text"].items():
            assert 0 <= a < b <= U and len(texts) == (2 if g["pe"] else 1)
            if g["ids"] is None:
                seen.add("numbered")
                assert texts[0].startswith(b"@%d/1\n" % (a + 1)) and texts[1].startswith(b"@%d/2\n" % (a + 1))
            if (a, b) != (0, U):
                seen.add("range")
            if a % g["B"]:
                seen.add("shift")
            if len(rc.consumed_blocks(U, g["B"], num_thr, a, b)) > num_thr:
                seen.add("steps")
    assert seen >= {("se", "any"), ("se", "po"), ("pe", "any"), ("pe", "po"), "code 1", "code 2", "code 3", "code None",
                    "quality", "two-line records", "numbered", "range", "shift", "steps"}
