"""The checkers of the stream, decode and quality/id stages (tests/streams_model.py, tests/qualid_model.py, the
decoder model's noise table, pack_seq / unpack_seq) against the REFERENCE'S OWN code, built by oracle/Makefile into
oracle/_ref (ref_streams, libref_qualid.so, libref_units.so): reorder_compress_streams.cpp, reorder_compress_quality_id.cpp,
util.cpp:113-267, decompress.cpp:615-end.  Every comparison is byte-exact.  Skipped where oracle/_ref is not built."""
import os

import numpy as np
import pytest

import decode_cases as dc
import qualid_model as qm
import ref_cases as rc
import streams_model as sm
from oracle import pyoracle as po
from test_gpu_decode import pack_seq, unpack_seq
from test_qualid_cpu import PATTERNS, _illumina_spelled_out, _table
from test_streams_cpu import encoded, slot_order, with_order

needs_streams = pytest.mark.skipif(po.ref_streams_bin() is None, reason="oracle/_ref/ref_streams not built (needs the reference sources)")
needs_qualid = pytest.mark.skipif(po.ref_qualid_lib() is None, reason="oracle/_ref/libref_qualid.so not built (needs the reference sources)")
needs_units = pytest.mark.skipif(po.ref_units() is None or not hasattr(po.ref_units(), "ref_u_dec_noise"),
                                 reason="oracle/_ref/libref_units.so not built (needs the reference sources)")

BIG = 1 << 30


# ---------------------------------------------------------------- write_streams against reorder_compress_streams
def same_streams(enc, N, pe, preserve_order, B, num_thr=1, what=""):
    """Every block of every stream, the set of files the real writer leaves, and stream_sizes against the real sizes."""
    st = sm.write_streams(enc, N, pe, preserve_order, B)
    want = sm.blocks_of(st)
    got, left = po.ref_streams(enc, N, pe, preserve_order, B, num_thr)
    nb = ((N // 2 if pe else N) + B - 1) // B
    assert left == sorted("%s.%d" % (s, b) for s in sm.stream_names(pe) for b in range(nb)), what
    sizes = sm.stream_sizes(enc, N, pe, preserve_order, B)
    for s in sm.stream_names(pe):
        assert len(got[s]) == nb, (what, s)
        for b in range(nb):
            assert got[s][b] == want[s][b], (what, s, b)
        assert np.diff(sizes[s].astype(np.int64)).tolist() == [len(x) for x in got[s]], (what, s, "stream_sizes")
    return got


@needs_streams
@pytest.mark.parametrize("pe", [False, True])
@pytest.mark.parametrize("preserve_order", [False, True])
@pytest.mark.parametrize("B", [1, 2, 3, 4, 8, BIG])
def test_streams_corner_case(pe, preserve_order, B):
    enc, seq, N, reads = sm.corner_case(pe, shuffle=pe or preserve_order)
    same_streams(enc, N, pe, preserve_order, B)


@needs_streams
@pytest.mark.parametrize("name", sorted(dc.escape_cases()))
@pytest.mark.parametrize("B", [1, 3, 7, BIG])
def test_streams_escape_cases(name, B):
    enc, seq, N, reads = dc.custom_case(dc.escape_cases()[name], unaligned=("ACGTN" * 3, ""))
    same_streams(enc, N, False, False, B)
    assert dc.writer_escapes(enc, N, BIG) > 0   # the escapes are really there


@needs_streams
@pytest.mark.parametrize("name", sorted(rc.STREAM_EDGES))
@pytest.mark.parametrize("preserve_order", [False, True])
def test_streams_edges(name, preserve_order):
    """Position deltas of exactly 65534 / 65535 / 65536 and a decreasing position; a pair distance of exactly +-32766 /
    +-32767 / +-32768; each of the five paired flags as the first unit of a block; mates of equal and of opposite
    orientation; lengths 0 and 511, aligned and unaligned; a read without noise, a read whose noise fills it; no aligned
    read at all, no unaligned read at all; num_thr 1 and 3 with more blocks than threads; a last block of one unit."""
    make, pe, any_order = rc.STREAM_EDGES[name]
    if not (preserve_order or any_order):
        preserve_order = True   # the interleaved single-end layout exists only with read_order.bin: run it shuffled twice
        seed = 1
    else:
        seed = 0
    slots = make()
    enc, N, reads = rc.make_enc(slots, rc.consensus(), shuffle=pe or preserve_order, seed=seed)
    U = N // 2 if pe else N
    one_left = [B for B in range(2, U) if U % B == 1][-1]   # the last block holds one unit
    assert U > 3                                            # B = 1: more blocks than threads
    for B in sorted({1, 2, 3, 5, one_left, BIG}):
        for num_thr in (1, 3):
            same_streams(enc, N, pe, preserve_order, B, num_thr, (name, B, num_thr))
    # the model's reader restores the reads from what the real writer wrote, except where a block opens with an
    # unaligned read 1 and holds an aligned one later (reorder_compress_streams.cpp:254-270, decompress.cpp:229-247)
    st = sm.write_streams(enc, N, pe, preserve_order, BIG)
    flags = st["read_flag.txt"][0]
    if preserve_order or flags[:1] not in b"24" or not set(flags) & set(b"013"):
        assert sm.read_all(st, rc.consensus(), N, pe, preserve_order, BIG) == reads


def test_edge_cases_hold_the_edges():
    """The hand-built cases really contain what their names say (checked on the model's output, no reference needed)."""
    seq = rc.consensus()
    enc, N, _ = rc.make_enc(rc.se_deltas(), seq, False)
    p = sm.write_streams(enc, N, False, False, BIG)["read_pos.bin"][0]
    u16, esc = (lambda v: int(v).to_bytes(2, "little")), b"\xff\xff"
    assert p[8:10] == u16(65534) and p[10:12] == esc and p[20:22] == esc and p[30:32] == esc   # 65534, 65535, 65536, down
    assert p[40:42] == u16(1) and p[42:44] == u16(0) and len(p) == 44
    assert {0, 511} <= set(enc["rlen"][:7].tolist()) and {0, 511} <= set(enc["rlen"][7:].tolist())
    enc, N, _ = rc.make_enc(rc.pe_pairdist(), seq, True)
    st = sm.write_streams(enc, N, True, False, BIG)
    assert st["read_flag.txt"][0] == b"011011000"
    assert np.frombuffer(st["read_pos_pair.bin"][0], np.int16).tolist() == [32766, -32766, 32766, -32766, 0]
    assert set(st["read_rev_pair.txt"][0]) == {ord("0"), ord("1")}
    enc, N, _ = rc.make_enc(rc.pe_flags(), seq, True)
    assert sm.write_streams(enc, N, True, False, 1)["read_flag.txt"][0] == b"4031202413"
    assert len(rc.make_enc(rc.se_all_unaligned(), seq, False)[0]["pos"]) == 0
    assert rc.make_enc(rc.pe_all_aligned(), seq, True)[0]["unaligned"] == b""


@needs_streams
@pytest.mark.parametrize("name,pe", [("var2k", False), ("test_1+2", True)])
@pytest.mark.parametrize("preserve_order", [False, True])
def test_streams_encoder_made(name, pe, preserve_order):
    enc, orig, N = encoded(name)
    e = with_order(enc, slot_order(enc, pe, preserve_order))
    for B, num_thr in ((97, 3), (1000, 1)):
        same_streams(e, N, pe, preserve_order, B, num_thr, (name, B))


# ---------------------------------------------------------------- the recorded fixtures (tests/golden/ref_*.npz)
@pytest.mark.parametrize("case", sorted(rc.STREAM_FIXTURES))
def test_stream_fixture_holds_its_case_and_equals_the_model(case):
    """Runs where oracle/_ref is absent: the file holds the inputs tests/ref_cases.py builds, and the recorded blocks
    equal the model's."""
    g = rc.load_stream_fixture(case)
    enc, seq, N, reads, pe, preserve_order, B = rc.stream_fixture_inputs(case)
    assert (g["seq"], g["reads"], g["N"], g["pe"], g["preserve_order"], g["B"]) == (seq, reads, N, pe, preserve_order, B)
    for k in rc.ENC_KEYS:
        if isinstance(enc[k], bytes):
            assert g["enc"][k] == enc[k], k
        else:
            assert g["enc"][k].dtype == enc[k].dtype and np.array_equal(g["enc"][k], enc[k]), k
    want = sm.write_streams(enc, N, pe, preserve_order, B)
    assert sorted(want) == sorted(g["streams"])
    for s, (data, off) in want.items():
        assert g["streams"][s][0] == data and np.array_equal(g["streams"][s][1], off), s


@needs_streams
@pytest.mark.parametrize("case", sorted(rc.STREAM_FIXTURES))
def test_stream_fixture_is_what_the_reference_writes(case):
    g = rc.load_stream_fixture(case)
    got, _ = po.ref_streams(g["enc"], g["N"], g["pe"], g["preserve_order"], g["B"])
    assert {s: b"".join(v) for s, v in got.items()} == {s: d for s, (d, o) in g["streams"].items()}
    for s, v in got.items():
        assert np.diff(g["streams"][s][1].astype(np.int64)).tolist() == [len(x) for x in v]


@pytest.mark.parametrize("case", sorted(rc.QUALID_FIXTURES))
def test_qualid_fixture_holds_its_case_and_equals_the_model(case):
    g = rc.load_qualid_fixture(case)
    files, order, n, pe, B = rc.qualid_fixture_inputs(case)
    assert (g["N"], g["pe"], g["B"]) == (n, pe, B) and np.array_equal(g["order"], order)
    assert g["files"] == {k: rc.image(v) for k, v in files.items()}
    slots = qm.order_array(order, n, pe)
    for (name, table), w in g["want"].items():
        kind = qm.ID if name.startswith("id") else qm.QUALITY
        m = qm.build(files[name], kind, slots, B, qm.illumina_table() if table == "illumina" else None)
        assert w["bytes"] == m["bytes"] and np.array_equal(w["len"], m["len"]), (name, table)
        assert np.array_equal(w["block_off"], m["block_off"]) and w["max_len"] == m["max_len"], (name, table)
        assert (m["changed"] > 0) == (table == "illumina")


# ---------------------------------------------------------------- qualid_model.build against reorder_compress_quality_id
N_REC = 330   # 30 cycles of LENGTHS


def model_blocks(lines, kind, slots, B):
    want = qm.build(lines, kind, slots, B)
    by_slot = want["lines"]
    return want, [by_slot[b:b + B] for b in range(0, len(by_slot), B)]


def same_qualid(files, order, n, pe, B, num_thr=1, paired_id_match=False):
    """files: {"quality_1": lines, "id_1": lines, ...} -> compares every block of every file with the model."""
    slots = qm.order_array(order, n, pe)
    want = {name: model_blocks(lines, qm.ID if name.startswith("id") else qm.QUALITY, slots, B)
            for name, lines in files.items()}
    lens = {name: want[name][0]["len"] for name in files if name.startswith("quality")}
    got, left = po.ref_qualid({name: rc.image(lines) for name, lines in files.items()}, order, n, pe, B, lens, num_thr,
                              paired_id_match)
    U = len(slots)
    nb = (U + B - 1) // B
    written = [name for name in files if not (name == "id_2" and paired_id_match)]
    assert left == sorted(["%s.%d" % (name, b) for name in written for b in range(nb)] + ["read_order.bin"]
                          + (["id_2"] if paired_id_match and "id_2" in files else []))
    for name in written:
        w, blocks = want[name]
        assert len(got[name]) == nb == len(w["block_off"]) - 1
        for b in range(nb):
            if name.startswith("id"):
                assert got[name][b] == blocks[b], (name, b)
                assert b"".join(x + b"\n" for x in got[name][b]) == w["bytes"][int(w["block_off"][b]):int(w["block_off"][b + 1])]
            else:
                assert got[name][b] == b"".join(blocks[b]) == w["bytes"][int(w["block_off"][b]):int(w["block_off"][b + 1])], (name, b)
    return got


def qualid_files(form, pe, n=N_REC):
    files = {}
    for m in range(2 if pe else 1):
        ids, quals = rc.qualid_lines(n, form, m)
        files["quality_%d" % (m + 1)] = quals
        files["id_%d" % (m + 1)] = ids
    return files


@needs_qualid
@pytest.mark.parametrize("form", sorted(rc.ID_FORMS))
def test_id_codec_restores_the_inputs(form):
    """The condition the cases below rest on: ids of these three forms come back from the reference's id codec as they
    went in (compress_id_block / decompress_id_block lie past this stage's boundary).  On the inputs themselves, both
    mates, in file order."""
    for pe in (False, True):
        files = qualid_files(form, pe)
        n = N_REC * (2 if pe else 1)
        got = same_qualid(files, rc.order_of("identity", n), n, pe, 100)
        for name in files:
            if name.startswith("id"):
                assert [x for blk in got[name] for x in blk] == files[name]


@needs_qualid
@pytest.mark.parametrize("pe", [False, True])
@pytest.mark.parametrize("which", ["identity", "reversed", "random"])
@pytest.mark.parametrize("B", [1, 3, 4, 1000])
def test_qualid_writer(pe, which, B):
    """Two conditions: num_reads >= 4 (the reference's `numreads / 4 - 1` wraps below that), and ids of forms the
    reference's id codec restores (test_id_codec_restores_the_inputs).  Lines are CR-free, qualities use every byte
    33..126, lengths cycle through test_gpu_qualid.LENGTHS."""
    per = {1: 44, 3: 110, 4: 110, 1000: N_REC}[B]   # fewer records where every block is a file or two
    n = per * (2 if pe else 1)
    # B = 1, 3, 4: num_reads / 4 > B, reorder_compress makes several passes; B = 1000: one pass, one block
    assert n >= 4 and (n // 4 > B) == (B != 1000) and per % len(rc.LENGTHS) == 0
    form = sorted(rc.ID_FORMS)[(B + len(which)) % 3]
    same_qualid(qualid_files(form, pe, per), rc.order_of(which, n), n, pe, B, num_thr=3 if B == 3 else 1)


@needs_qualid
@pytest.mark.parametrize("form", sorted(rc.ID_FORMS))
def test_qualid_writer_paired_id_match(form):
    """paired_id_match: id_2 is neither written nor removed."""
    n = 2 * N_REC
    same_qualid(qualid_files(form, True), rc.order_of("random", n), n, True, 7, paired_id_match=True)


@needs_qualid
def test_qualid_writer_smallest_and_uneven():
    """num_reads = 4, the smallest the reference takes; a count that is no multiple of B or of the pass size."""
    for n, pe, B in ((4, False, 1), (4, True, 1), (4, False, 3), (331, False, 4), (222, True, 4), (97, False, 5)):
        per = n // 2 if pe else n
        same_qualid(qualid_files("r", pe, per), rc.order_of("random", n), n, pe, B)


# ---------------------------------------------------------------- tables and patterns
BINARY = [(20, 40, 6), (17, 17, 17), (0, 0, 0), (94, 94, 0)]


def test_illumina_table_third_witness():
    """Runs where oracle/_ref is absent: the model, the library and the spelled-out restatement agree."""
    assert list(qm.illumina_table()) == _illumina_spelled_out() == _table(1)[1]


@needs_qualid
def test_illumina_table_equals_the_reference():
    real = po.ref_quality_table("illumina")
    assert len(real) == 128
    assert real == qm.illumina_table() == bytes(_illumina_spelled_out())
    rcode, t = _table(1)
    assert rcode == 0 and bytes(t) == real
    assert real[33 + 1] == 33 and real[33 + 2] == 33 + 6   # the edge between the first two bins


@needs_qualid
@pytest.mark.parametrize("thr,high,low", BINARY)
def test_binary_table_equals_the_reference(thr, high, low):
    real = po.ref_quality_table("binary", thr, high, low)
    assert real == qm.binary_table(thr, high, low)
    rcode, t = _table(2, thr, high, low)
    assert rcode == 0 and bytes(t) == real


@needs_qualid
def test_quantize_quality_equals_the_table_application():
    line = bytes(range(128))
    lines = [line, b"", line[::-1], b"I", bytes(range(33, 127))]
    slots = list(range(len(lines)))
    for table in [qm.illumina_table()] + [qm.binary_table(*b) for b in BINARY]:
        got = po.ref_quantize(lines, table)
        assert got == [bytes(table[c] for c in x) for x in lines]
        assert got == qm.build(lines, qm.QUALITY, slots, 2, table)["lines"]
    # ... and with the real table, as preprocess does
    assert po.ref_quantize(lines, po.ref_quality_table("illumina")) == qm.build(lines, qm.QUALITY, slots, 2, qm.illumina_table())["lines"]


@needs_qualid
@pytest.mark.parametrize("a,b,code", [p for p in PATTERNS if p[0] and p[1]])
def test_id_patterns_equal_the_reference(a, b, code):
    assert po.ref_find_id_pattern(a, b) == code == qm.find_id_pattern(a, b)
    for c in (1, 2, 3):
        assert po.ref_check_id_pattern(a, b, c) == qm.check_id_pattern(a, b, c), c


def _sweep():
    rng = np.random.default_rng(2024)
    alphabet = np.frombuffer(b"a12 :/", np.uint8)
    out = []
    for k in range(6000):
        n = int(rng.integers(1, 9))
        a = alphabet[rng.integers(0, 6, n)]
        kind = k % 4
        if kind == 0:      # unrelated
            b = alphabet[rng.integers(0, 6, int(rng.integers(1, 9)))]
        elif kind == 1:    # equal
            b = a.copy()
        else:              # equal but for one position, or with every '1' turned into '2'
            b = a.copy()
            if kind == 2:
                b[int(rng.integers(0, n))] = alphabet[int(rng.integers(0, 6))]
            else:
                hit = np.flatnonzero(a == ord("1"))
                if len(hit):
                    pick = hit[rng.random(len(hit)) < 0.7]
                    b[pick] = ord("2")
        out.append((a.tobytes(), b.tobytes()))
    return out


@needs_qualid
def test_id_patterns_random_sweep():
    """A few thousand pairs over {a 1 2 ' ' : /}, lengths 1..8; the empty id is left out (the reference indexes
    id[len - 1])."""
    seen = set()
    for a, b in _sweep():
        assert a and b
        f = po.ref_find_id_pattern(a, b)
        assert f == qm.find_id_pattern(a, b), (a, b)
        seen.add(f)
        for c in (1, 2, 3):
            ok = po.ref_check_id_pattern(a, b, c)
            assert ok == qm.check_id_pattern(a, b, c), (a, b, c)
            if ok:   # modify_id turns id_1 into id_2 wherever the pattern holds ...
                if c == 3 and a.count(b" ") != 1:
                    # ... for code 3 with one space: modify_id (util.cpp:261-265) rewrites the byte after the FIRST space
                    # only, and looks for a space without a bound; without one the pattern holds for equal ids alone
                    assert b" " in a or a == b
                    continue
                assert po.ref_modify_id(a, c) == b, (a, b, c)
    assert seen == {0, 1, 2, 3}


@needs_qualid
def test_modify_id_on_the_id_forms():
    for form, (f1, f2, code) in rc.ID_FORMS.items():
        for i in (0, 7, 329):
            a, b = f1(i), f2(i)
            assert po.ref_find_id_pattern(a, b) == code == qm.find_id_pattern(a, b)
            assert po.ref_modify_id(a, code) == b


# ---------------------------------------------------------------- the decoder's noise table and the packed consensus
@needs_units
def test_dec_noise_table():
    U = po.ref_units()
    dec = np.zeros((128, 128), np.uint8)
    enc = np.zeros((128, 128), np.uint8)
    assert U.ref_u_dec_noise(dec.ctypes.data) == 0 and U.ref_u_enc_noise(enc.ctypes.data) == 0
    model = np.zeros((128, 128), np.uint8)
    for base, row in sm.DEC_NOISE.items():
        for k, ch in enumerate(row):
            model[ord(base), ord("0") + k] = ord(ch)
    assert np.array_equal(dec, model)
    # the two real tables invert each other: dec[ref][enc[ref][read]] == read for every substitution
    n = 0
    for ref in b"ACGTN":
        for read in b"ACGTN":
            if enc[ref, read]:
                assert dec[ref, enc[ref, read]] == read, (chr(ref), chr(read))
                n += 1
    assert n == 20 and np.count_nonzero(enc) == 20 and np.count_nonzero(dec) == 20


@needs_units
@pytest.mark.skipif(po.ref_bsc_bin() is None, reason="oracle/_ref/ref_bsc not built")
@pytest.mark.parametrize("num_thr", [1, 2])
def test_unpack_seq_format(tmp_path, num_thr):
    """read_seq.bin.<t> (2 bits per base, A C G T = 0..3, low bits first) + .tail, for consensus lengths = 0..3 mod 4 per
    tid and an empty tid: what pack_seq / unpack_seq and DecodeStage.seq_from_files assume, through the real
    decompress_unpack_seq (the packed file is first deflated with the real BSC_compress, as the encoder leaves it)."""
    import subprocess
    rng = np.random.default_rng(5)
    pieces = ["".join("ACGT"[x] for x in rng.integers(0, 4, n)) for n in (8, 5, 0, 6, 7, 3)]
    assert sorted(set(len(p) % 4 for p in pieces)) == [0, 1, 2, 3]
    base = str(tmp_path / "read_seq.bin")
    packed, tails = [], []
    for t, s in enumerate(pieces):
        lens, pk, tl = pack_seq(s, 1)
        assert lens.tolist() == [len(s)] and len(pk) == len(s) // 4 and tl == [s[len(s) - len(s) % 4:]]
        packed.append(pk)
        tails.append(tl[0])
        open("%s.%d.raw" % (base, t), "wb").write(pk)
        subprocess.run([po.ref_bsc_bin(), "%s.%d.raw" % (base, t), "%s.%d.bsc" % (base, t)], check=True)
        os.remove("%s.%d.raw" % (base, t))
        open("%s.%d.tail" % (base, t), "w").write(tl[0])
    assert po.ref_units().ref_u_unpack_seq(base.encode(), len(pieces), num_thr) == 0
    got = [open("%s.%d" % (base, t)).read() for t in range(len(pieces))]
    assert got == pieces
    assert unpack_seq(packed, tails) == "".join(pieces)
    assert sorted(os.listdir(str(tmp_path))) == sorted("read_seq.bin.%d" % t for t in range(len(pieces)))
    # cut evenly into tids, as the GPU tests do
    whole = "".join(pieces)
    lens, pk, tl = pack_seq(whole, 3)
    cut = np.concatenate([[0], np.cumsum(lens // 4)]).astype(int)
    assert unpack_seq([pk[cut[t]:cut[t + 1]] for t in range(3)], tl) == whole
