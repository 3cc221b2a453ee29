"""GPU tests of the stream decoder (include/spring_decode.h): the reads it restores from the per-block streams against
the checker's reader (tests/streams_model.py) and against the original reads, from every input form; its refusals;
its file contract; one run at size."""
import functools
import os

import numpy as np
import pytest

import decode_cases as dc
import ref_cases as rc
import streams_model as sm
from helpers import GOLDEN, interleave_order_N, make_N_reads, named_set, read_strings
from oracle import pyoracle as po

pytestmark = pytest.mark.gpu

NAT = {c: i for i, c in enumerate("ACGT")}


def pack_seq(seq, T=1):
    """The consensus text cut into T tids -> (seq_len_tid, packed bytes, tails) as EncoderStage.seq_packed gives."""
    cut = [len(seq) * t // T for t in range(T + 1)]
    lens, packed, tails = [], bytearray(), []
    for t in range(T):
        s = seq[cut[t]:cut[t + 1]]
        nb = len(s) // 4
        c = np.array([NAT[x] for x in s[:4 * nb]], np.uint8).reshape(nb, 4) if nb else np.zeros((0, 4), np.uint8)
        packed += (c[:, 0] | (c[:, 1] << 2) | (c[:, 2] << 4) | (c[:, 3] << 6)).astype(np.uint8).tobytes()
        tails.append(s[4 * nb:])
        lens.append(len(s))
    return np.array(lens, np.uint64), bytes(packed), tails


def unpack_seq(packed_by_tid, tails):
    out = []
    for p, t in zip(packed_by_tid, tails):
        b = np.frombuffer(p, np.uint8)
        c = (b[:, None] >> (2 * np.arange(4, dtype=np.uint8))) & 3
        out.append(np.frombuffer(b"ACGT", np.uint8)[c.reshape(-1)].tobytes().decode() + t)
    return "".join(out)


def decoded(ds, pe):
    return ds.reads(0) + (ds.reads(1) if pe else [])


def downloads(ss, pe):
    return {s: ss.download(s) for s in sm.stream_names(pe)}


def window(streams, b0, nb):
    """{stream: (bytes, offsets)} -> the same restricted to blocks [b0, b0 + nb), offsets from 0."""
    out = {}
    for s, (d, o) in streams.items():
        lo, hi = int(o[b0]), int(o[b0 + nb])
        out[s] = (d[lo:hi], np.asarray(o[b0:b0 + nb + 1], np.uint64) - np.uint64(lo))
    return out


# ---------------------------------------------------------------- 1. corner cases
@pytest.mark.parametrize("pe", [False, True])
@pytest.mark.parametrize("preserve_order", [False, True])
@pytest.mark.parametrize("B", [1, 2, 3, 4, 8, 1 << 30])
def test_corner_cases(pe, preserve_order, B):
    from spring_amd import DecodeStage, StreamsStage
    from spring_amd.reorder import ReorderError
    enc, seq, N, reads = sm.corner_case(pe, shuffle=pe or preserve_order)
    st = sm.write_streams(enc, N, pe, preserve_order, B)
    try:
        want = sm.read_all(st, seq, N, pe, preserve_order, B)
    except AssertionError:
        want = None   # the reader's quirk: a block that opens with an unaligned read 1 and has an aligned one after
    with StreamsStage() as ss, DecodeStage() as ds:
        ss.from_host(enc["pos"], enc["rc"], enc["noise"], enc["noisepos"], enc["order"], enc["rlen"], enc["unaligned"],
                     N, pe, preserve_order, B)
        ds.seq_from_host(*pack_seq(seq, 3))
        for how in ("streams", "host"):
            if want is None:
                with pytest.raises(ReorderError, match="code -1"):
                    ds.from_streams(ss) if how == "streams" else ds.from_host(downloads(ss, pe), N, pe,
                                                                               preserve_order, B)
                with pytest.raises(ReorderError, match="code -4"):
                    ds.download(0)
                continue
            info = ds.from_streams(ss) if how == "streams" else ds.from_host(downloads(ss, pe), N, pe, preserve_order, B)
            got = decoded(ds, pe)
            assert got == want == reads, (how, B)
            assert info["num_units"] == (N // 2 if pe else N) and info["pos_escapes"] == ss.info["pos_escapes"]
            assert info["n_aligned"] + info["n_unaligned"] == N
    assert want is not None or (pe and not preserve_order and B == 3)


# ---------------------------------------------------------------- 1b. blocks the reference's own writer wrote
QUIRK = {"pe_corner_B3": 3, "pe_flags_B3": 0}   # case -> units that decode from the blocks before the first refused one


@pytest.mark.parametrize("case", sorted(rc.STREAM_FIXTURES))
def test_decodes_reference_written_blocks(case):
    """The blocks the real reorder_compress_streams wrote (tests/golden/ref_streams_<case>.npz), with the case's
    consensus, decode to the case's original reads: the decoder against the real WRITER, no reader model in between.
    Where a block opens with an unaligned read 1 and holds an aligned one later, the real writer stores that position
    as a u16 delta against 0 (reorder_compress_streams.cpp:312-328) and the real reader takes the block's first
    position as a u64 (decompress.cpp:229-247): the decoder refuses such a block, as test_corner_cases says of the
    model-written one, and decodes the blocks before it."""
    from spring_amd import DecodeStage
    from spring_amd.reorder import ReorderError
    g = rc.load_stream_fixture(case)
    N, pe, po_, B = g["N"], g["pe"], g["preserve_order"], g["B"]
    U = N // 2 if pe else N
    with DecodeStage() as ds:
        ds.seq_from_host(*pack_seq(g["seq"], 3))
        if case not in QUIRK:
            info = ds.from_host(g["streams"], N, pe, po_, B)
            assert decoded(ds, pe) == g["reads"]
            assert info["num_units"] == U and info["n_aligned"] + info["n_unaligned"] == N
            assert info["n_aligned"] == len(g["enc"]["pos"])
            return
        with pytest.raises(ReorderError, match="code -1"):
            ds.from_host(g["streams"], N, pe, po_, B)
        with pytest.raises(ReorderError, match="code -4"):
            ds.download(0)
        k = QUIRK[case] // B   # whole blocks before the refused one
        if k:
            ds.from_host(window(g["streams"], 0, k), N, pe, po_, B)
            assert ds.reads(0) == g["reads"][:k * B] and ds.reads(1) == g["reads"][U:U + k * B]


# ---------------------------------------------------------------- 2. encoder output
@functools.lru_cache(maxsize=None)
def _set(name, nN=80, seed=5):
    dna, n, L = named_set(name)
    read, ln = po.load_dna(dna, n, L)
    strs = read_strings(read, ln)
    Nreads = make_N_reads(strs, nN + (n + nN) % 2, seed)
    order_N = interleave_order_N(n, len(Nreads), seed + 7)
    isN = np.zeros(n + len(Nreads), bool)
    isN[order_N] = True
    orig = [None] * (n + len(Nreads))
    for i, p in enumerate(np.flatnonzero(~isN)):
        orig[p] = strs[i]
    for i, p in enumerate(order_N):
        orig[p] = Nreads[i]
    return dna, n, L, po.pack_dnaN(Nreads), order_N, orig


def slot_contents(order, slot, orig):
    """slot slot[k] holds record k, i.e. original read order[k]."""
    want = [None] * len(order)
    for k in range(len(order)):
        want[int(slot[k])] = orig[int(order[k])]
    return want


@pytest.mark.parametrize("name,pe,T", [("syn5k_150", False, 3), ("var2k", False, 2), ("test_1+2", True, 3),
                                       ("syn2k_100", True, 2)])
def test_encoder_output(name, pe, T):
    import spring_amd
    from spring_amd import DecodeStage, StreamsStage
    from spring_amd.encoder import EncoderStage
    dna, n, L, dnaN, order_N, orig = _set(name)
    N = n + len(order_N)
    with spring_amd.ReorderStage(spring_amd.ReorderOpts(num_chains=8, num_thr=T)) as st:
        st.load_dna(dna, n, L)
        st.run()
        with EncoderStage() as enc, StreamsStage() as ss, DecodeStage() as a, DecodeStage() as b:
            enc.encode(st, dnaN, order_N)
            e = enc.streams()
            assert len(e["seq_len_tid"]) == T
            a.seq_from_encoder(enc)
            b.seq_from_host(e["seq_len_tid"], *enc.seq_packed())
            for preserve_order in (False, True):
                slot = e["order"] if preserve_order else (po.pe_encode(e["order"]) if pe else np.arange(N))
                ew = dict(e, order=slot if (pe or preserve_order) else e["order"])
                want_slots = slot_contents(e["order"], slot, orig)
                for B in (1, 7, 256000):
                    ss.from_encoder(enc, N, pe, preserve_order, B)
                    want = sm.read_all(sm.write_streams(ew, N, pe, preserve_order, B), e["seq"].decode(), N, pe,
                                       preserve_order, B)
                    assert want == want_slots
                    a.from_streams(ss)
                    got = decoded(a, pe)
                    assert got == want, (name, preserve_order, B)
                    b.from_streams(ss)
                    for m in range(2 if pe else 1):
                        assert a.download(m)[0] == b.download(m)[0] and np.array_equal(a.download(m)[1], b.download(m)[1])
                    if preserve_order:
                        assert got == orig


# ---------------------------------------------------------------- 3. FASTQ round trip
def _synth_fastq(seed, n, lmin, lmax, pn=0.1):
    rng = np.random.default_rng(seed)
    genome = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, 30000)]
    out, seqs = [], []
    for i in range(n):
        L = int(rng.integers(lmin, lmax + 1))
        p = int(rng.integers(0, len(genome) - L))
        r = genome[p:p + L].copy()
        if rng.random() < 0.5 and L:
            r = np.frombuffer(r.tobytes()[::-1].translate(bytes.maketrans(b"ACGT", b"TGCA")), np.uint8).copy()
        if rng.random() < pn and L:
            r[rng.integers(0, L, max(1, L // 20))] = ord("N")
        out += [b"@r%d" % i, r.tobytes(), b"+", b"I" * L]
        seqs.append(r.tobytes().decode())
    return b"\n".join(out) + b"\n", seqs


def _fastq_seqs(path):
    lines = open(path, "rb").read().split(b"\n")
    return [lines[i].strip().decode() for i in range(1, len(lines) - 1, 4)]


@pytest.mark.parametrize("case", ["synthetic", "golden_pe"])
@pytest.mark.parametrize("preserve_order", [False, True])
def test_fastq_round_trip(case, preserve_order):
    import spring_amd
    from spring_amd import DecodeStage, StreamsStage
    from spring_amd.encoder import EncoderStage
    if case == "synthetic":
        f1, s1 = _synth_fastq(11, 4000, 0, 160)
        f2, s2 = None, []
    else:
        f1, f2 = (open(os.path.join(GOLDEN, "test_%d.fastq" % j), "rb").read() for j in (1, 2))
        s1, s2 = _fastq_seqs(os.path.join(GOLDEN, "test_1.fastq")), _fastq_seqs(os.path.join(GOLDEN, "test_2.fastq"))
    pe = f2 is not None
    fq = s1 + s2
    N = len(fq)
    with spring_amd.ReorderStage(spring_amd.ReorderOpts(num_chains=8, num_thr=2)) as st:
        info = st.load_fastq(f1, f2)
        assert sum(info["num_reads"]) == N
        st.run()
        dnaN, order_N = st.fastq_N(0)
        if pe:   # preprocess.cpp:363-381: the two files' N reads merged, file-2 indices after file 1's
            d2, o2 = st.fastq_N(1)
            dnaN, order_N = dnaN + d2, np.concatenate([order_N, o2 + info["num_reads"][0]]).astype(np.uint32)
        with EncoderStage() as enc, StreamsStage() as ss, DecodeStage() as ds:
            enc.encode(st, dnaN, order_N)
            order = enc.streams()["order"]
            ss.from_encoder(enc, N, pe, preserve_order, 97)
            ds.seq_from_encoder(enc)
            ds.from_streams(ss)
            r1 = ds.reads(0)
            r2 = ds.reads(1) if pe else []
    if preserve_order:
        assert r1 == s1 and r2 == s2
    else:
        assert sorted(r1 + r2) == sorted(fq)
        slot = po.pe_encode(order) if pe else np.arange(N)
        assert r1 + r2 == slot_contents(order, slot, fq)


# ---------------------------------------------------------------- 4. adversarial escapes
@pytest.mark.parametrize("name", sorted(dc.escape_cases()))
@pytest.mark.parametrize("B", [1, 3, 7, 1 << 30])
def test_adversarial_escapes(name, B):
    from spring_amd import DecodeStage, StreamsStage
    enc, seq, N, reads = dc.custom_case(dc.escape_cases()[name], unaligned=("ACGTN" * 3, ""))
    want = sm.read_all(sm.write_streams(enc, N, False, False, B), seq, N, False, False, B)
    assert want == reads
    with StreamsStage() as ss, DecodeStage() as ds:
        si = ss.from_host(enc["pos"], enc["rc"], enc["noise"], enc["noisepos"], None, enc["rlen"], enc["unaligned"],
                          N, False, False, B)
        assert si["pos_escapes"] == dc.writer_escapes(enc, N, B)
        ds.seq_from_host(*pack_seq(seq, 2))
        info = ds.from_streams(ss)
        assert ds.reads(0) == want
        assert info["pos_escapes"] == si["pos_escapes"]
        info = ds.from_host(downloads(ss, False), N, False, False, B)
        assert ds.reads(0) == want and info["pos_escapes"] == si["pos_escapes"]


# ---------------------------------------------------------------- 5. block windows
@pytest.mark.parametrize("name,pe,preserve_order,B", [("syn2k_100", False, False, 300), ("test_1+2", True, False, 7),
                                                      ("var2k", False, True, 333)])
def test_block_windows(name, pe, preserve_order, B):
    import spring_amd
    from spring_amd import DecodeStage, StreamsStage
    from spring_amd.encoder import EncoderStage
    dna, n, L, dnaN, order_N, orig = _set(name)
    N = n + len(order_N)
    U = N // 2 if pe else N
    with spring_amd.ReorderStage(spring_amd.ReorderOpts(num_chains=8, num_thr=2)) as st:
        st.load_dna(dna, n, L)
        st.run()
        with EncoderStage() as enc, StreamsStage() as ss, DecodeStage() as ds:
            enc.encode(st, dnaN, order_N)
            ss.from_encoder(enc, N, pe, preserve_order, B)
            ds.seq_from_encoder(enc)
            ds.from_streams(ss)
            full = [ds.reads(m) for m in range(2 if pe else 1)]
            nb = ss.info["num_blocks"]
            assert U % B != 0   # the last block is partial
            streams = downloads(ss, pe)
            for b0, k in ((0, 1), (nb // 2 - 1, 3), (nb - 1, 1), (0, nb)):
                info = ds.from_host(window(streams, b0, k), N, pe, preserve_order, B, first_block=b0)
                lo, hi = b0 * B, min((b0 + k) * B, U)
                assert info["num_units"] == hi - lo and info["first_block"] == b0
                for m in range(2 if pe else 1):
                    assert ds.reads(m) == full[m][lo:hi], (b0, k, m)


# ---------------------------------------------------------------- 6. refusals
def _mutable(streams):
    return {s: (bytearray(d), np.array(o, np.uint64)) for s, (d, o) in streams.items()}


def _refuse(ds, streams, N, pe, po_, B, code="code -1", **kw):
    from spring_amd.reorder import ReorderError
    with pytest.raises(ReorderError, match=code):
        ds.from_host({s: (bytes(d), o) for s, (d, o) in streams.items()}, N, pe, po_, B, **kw)
    with pytest.raises(ReorderError, match="code -4"):
        ds.download(0)


def _se_case(name="gaps", B=1 << 30):
    from spring_amd import StreamsStage
    enc, seq, N, reads = dc.custom_case(dc.escape_cases()[name], unaligned=("ACGTN" * 3, "TTAGN"))
    with StreamsStage() as ss:
        ss.from_host(enc["pos"], enc["rc"], enc["noise"], enc["noisepos"], None, enc["rlen"], enc["unaligned"], N,
                     False, False, B)
        return downloads(ss, False), seq, N, reads


def _pe_case(B=8):
    from spring_amd import StreamsStage
    enc, seq, N, reads = sm.corner_case(True)
    with StreamsStage() as ss:
        ss.from_host(enc["pos"], enc["rc"], enc["noise"], enc["noisepos"], enc["order"], enc["rlen"], enc["unaligned"],
                     N, True, False, B)
        return downloads(ss, True), seq, N, reads


def test_refuses_flags_orientations_noise_and_unaligned_bytes():
    from spring_amd import DecodeStage
    se, seq, N, reads = _se_case()
    pe, pseq, PN, preads = _pe_case()
    B = 1 << 30
    with DecodeStage() as ds:
        ds.seq_from_host(*pack_seq(seq, 2))
        ds.from_host(se, N, False, False, B)
        assert ds.reads(0) == reads   # the valid input decodes
        for stream, at, val in (("read_flag.txt", 2, b"1"),                 # a paired-end flag in single-end data
                                ("read_rev.txt", 3, b"x"),
                                ("read_noise.txt", 0, b"4"),                 # line 0 holds noise
                                ("read_unaligned.txt", 5, b"X")):
            s = _mutable(se)
            assert s["read_noise.txt"][0][0] != ord("\n")
            s[stream][0][at:at + 1] = val
            _refuse(ds, s, N, False, False, B)
        s = _mutable(se)   # a noise position past the read's length (24)
        s["read_noisepos.bin"][0][0:2] = (30).to_bytes(2, "little")
        _refuse(ds, s, N, False, False, B)
        ds.seq_from_host(*pack_seq(pseq, 1))
        ds.from_host(pe, PN, True, False, 8)
        assert ds.reads(0) + ds.reads(1) == preads
        for stream, at, val in (("read_flag.txt", 1, b"5"), ("read_rev_pair.txt", 0, b"2"), ("read_rev.txt", 0, b"D")):
            s = _mutable(pe)
            s[stream][0][at:at + 1] = val
            _refuse(ds, s, PN, True, False, 8)


def test_refuses_reads_past_the_consensus():
    from spring_amd import DecodeStage
    se, seq, N, reads = _se_case()   # gaps: 100 (u64), then 100 + 65534 by a u16 delta
    with DecodeStage() as ds:
        ds.seq_from_host(*pack_seq(seq[:110], 1))    # the u64 read at 100 (24 bases) ends past 110
        _refuse(ds, _mutable(_se_case(B=1)[0]), N, False, False, 1, num_blocks=1)
        ds.seq_from_host(*pack_seq(seq[:65650], 1))  # block 0 of B = 2: 100 by u64 fits, 65634 by a delta does not
        w = window(_se_case(B=2)[0], 0, 1)
        _refuse(ds, _mutable(w), N, False, False, 2)
        ds.seq_from_host(*pack_seq(seq[:65700], 1))
        ds.from_host(w, N, False, False, 2)
        assert ds.reads(0) == reads[:2]
    pe, pseq, PN, preads = _pe_case()
    with DecodeStage() as ds:
        ds.seq_from_host(*pack_seq(pseq[:150000], 1))   # every read of the corner case ends before 132100
        ds.from_host(pe, PN, True, False, 8)
        assert ds.reads(0) + ds.reads(1) == preads
        s = _mutable(pe)   # unit 2 (flag 0): pos_pair -32766 -> +32767, read 2 at 164836
        assert s["read_pos_pair.bin"][0][2:4] == (-32766).to_bytes(2, "little", signed=True)
        s["read_pos_pair.bin"][0][2:4] = (32767).to_bytes(2, "little", signed=True)
        _refuse(ds, s, PN, True, False, 8)


def _shrink_last(s, stream, k):
    d, o = s[stream]
    del d[len(d) - k:]
    o[-1] -= np.uint64(k)


def test_refuses_under_and_over_consumed_streams_and_bad_tables():
    from spring_amd import DecodeStage
    se, seq, N, reads = _se_case("decreasing")
    B = 1 << 30
    with DecodeStage() as ds:
        ds.seq_from_host(*pack_seq(seq, 1))
        ds.from_host(se, N, False, False, B)
        assert ds.reads(0) == reads
        s = _mutable(se)   # a truncated escape: the last u64 payload cut short
        _shrink_last(s, "read_pos.bin", 4)
        _refuse(ds, s, N, False, False, B)
        s = _mutable(se)   # trailing bytes
        s["read_pos.bin"][0].extend(b"\0\0")
        s["read_pos.bin"][1][-1] += np.uint64(2)
        _refuse(ds, s, N, False, False, B)
        for stream in ("read_rev.txt", "read_noisepos.bin", "read_unaligned.txt", "read_noise.txt"):
            s = _mutable(se)   # one stream a byte (entry) short, or one too long
            _shrink_last(s, stream, 2 if stream == "read_noisepos.bin" else 1)
            _refuse(ds, s, N, False, False, B)
            s = _mutable(se)
            s[stream][0].extend(b"\n\n" if stream != "read_unaligned.txt" else b"A")
            s[stream][1][-1] += np.uint64(2 if stream != "read_unaligned.txt" else 1)
            _refuse(ds, s, N, False, False, B)
        se3, *_ = _se_case("decreasing", B=3)
        ds.from_host(se3, N, False, False, 3)
        assert ds.reads(0) == reads
        s = _mutable(se3)   # a table that is not monotone
        s["read_rev.txt"][1][1], s["read_rev.txt"][1][2] = s["read_rev.txt"][1][2], s["read_rev.txt"][1][1]
        _refuse(ds, s, N, False, False, 3)
        s = _mutable(se3)   # a block boundary moved: the counts of the units no longer match the table
        s["read_rev.txt"][1][1] += np.uint64(1)
        _refuse(ds, s, N, False, False, 3)
        s = _mutable(se3)
        s["read_noise.txt"][1][1] += np.uint64(1)
        _refuse(ds, s, N, False, False, 3)
        s = _mutable(se3)   # the flag table does not match the block sizes
        s["read_flag.txt"][1][1] -= np.uint64(1)
        _refuse(ds, s, N, False, False, 3)
    # the reader's quirk (decompress.cpp:229-247 against reorder_compress_streams.cpp:254-270)
    pe, pseq, PN, preads = _pe_case(B=3)
    with DecodeStage() as ds:
        ds.seq_from_host(*pack_seq(pseq, 1))
        _refuse(ds, _mutable(pe), PN, True, False, 3)
        ds.from_host(window(pe, 0, 1), PN, True, False, 3)   # block 0 alone is fine
        assert ds.reads(0) == preads[:3]


def test_refuses_without_a_consensus():
    from spring_amd import DecodeStage
    se, seq, N, reads = _se_case()
    with DecodeStage() as ds:
        _refuse(ds, _mutable(se), N, False, False, 1 << 30, code="code -4")


# ---------------------------------------------------------------- 7. file forms
def _files(d):
    return {f: open(os.path.join(d, f), "rb").read() for f in sorted(os.listdir(d))}


@pytest.mark.parametrize("pe,preserve_order", [(False, False), (False, True), (True, False)])
def test_file_forms(tmp_path, pe, preserve_order):
    import spring_amd
    from spring_amd import DecodeStage
    from spring_amd.encoder import call_reorder_encoder
    from spring_amd.order_ops import pe_encode
    from spring_amd.reorder import CompressionParams, ReorderError
    from spring_amd.streams import call_reorder_compress_streams
    from readsets import pack_var
    dna, n, L = named_set("test_1+2" if pe else "syn2k_100")
    d = str(tmp_path)
    B, T = 100 if not pe else 9, 2
    if pe:
        read, ln = po.load_dna(dna, n, L)
        strs = read_strings(read, ln)
        half = n // 2
        n = 2 * half
        open(os.path.join(d, "input_clean_1.dna"), "wb").write(pack_var([x.encode() for x in strs[:half]]))
        open(os.path.join(d, "input_clean_2.dna"), "wb").write(pack_var([x.encode() for x in strs[half:n]]))
        cp = CompressionParams(L, [half, half], num_thr=T, paired_end=True)
    else:
        open(os.path.join(d, "input_clean_1.dna"), "wb").write(dna)
        cp = CompressionParams(L, [n, 0], num_thr=T)
    call_reorder_encoder(d, cp, n, spring_amd.ReorderOpts(num_chains=8, num_thr=T))
    for t in range(T):   # what BSC_decompress leaves
        os.rename(os.path.join(d, "read_seq.bin.%d.tmp" % t), os.path.join(d, "read_seq.bin.%d" % t))
    if pe and not preserve_order:
        order = np.frombuffer(open(os.path.join(d, "read_order.bin"), "rb").read(), np.uint32)
        open(os.path.join(d, "read_order.bin"), "wb").write(pe_encode(order)[0].tobytes())
    seqf = {t: (open(os.path.join(d, "read_seq.bin.%d" % t), "rb").read(),
                open(os.path.join(d, "read_seq.bin.%d.tail" % t), "rb").read().decode()) for t in range(T)}
    seq = unpack_seq([seqf[t][0] for t in range(T)], [seqf[t][1] for t in range(T)])
    info = call_reorder_compress_streams(d, cp, preserve_order, B, num_reads=n)
    nb = info["num_blocks"]
    names = sm.stream_names(pe)
    streams = {}
    for s in names:   # the in-memory image of every block, for the reader and the in-memory decode
        blocks = [open(os.path.join(d, "%s.%d" % (s, b)), "rb").read() for b in range(nb)]
        streams[s] = (b"".join(blocks), np.concatenate([[0], np.cumsum([len(x) for x in blocks])]).astype(np.uint64))
    want = sm.read_all(streams, seq, n, pe, preserve_order, B)
    U = n // 2 if pe else n
    with DecodeStage() as ds, DecodeStage() as mem:
        mem.seq_from_host(*pack_seq(seq, 1))
        mem.from_host(streams, n, pe, preserve_order, B)
        full = decoded(mem, pe)
        assert full == want
        ds.seq_from_files(d, T)
        assert not [f for f in os.listdir(d) if f.startswith("read_seq.bin")]
        # a refused window (a flag file one byte too long) leaves every file in place
        bad = os.path.join(d, "read_flag.txt.%d" % (nb - 1))
        good = open(bad, "rb").read()
        open(bad, "ab").write(b"0")
        before = _files(d)
        with pytest.raises(ReorderError, match="code -1"):
            ds.from_files(d, nb - 2, 2, n, pe, preserve_order, B)
        assert _files(d) == before
        open(bad, "wb").write(good)
        got = [[], []]
        for b0, k in ((0, nb - 2), (nb - 2, 2)):
            fi = ds.from_files(d, b0, k, n, pe, preserve_order, B)
            assert fi["ms_file"] > 0 and fi["num_units"] == min((b0 + k) * B, U) - b0 * B
            for m in range(2 if pe else 1):
                got[m] += ds.reads(m)
            assert not [f for f in os.listdir(d) if any(f == "%s.%d" % (s, b) for s in names for b in range(b0, b0 + k))]
        assert got[0] + got[1] == full
    assert not [f for f in os.listdir(d) if any(f.startswith(s + ".") for s in names)]


# ---------------------------------------------------------------- 8. at size
@pytest.mark.parametrize("pe", [False, True])
def test_ten_million_reads_at_size(pe):
    """10 M synthetic reads of 150 bp through reorder -> encoder -> streams -> decode on the device; the decoded reads
    equal the synthetic originals (vectorised numpy) in both order modes (single-end) or after pe_encode (pairs)."""
    import spring_amd
    from spring_amd import DecodeStage, StreamsStage
    from spring_amd.encoder import EncoderStage
    from spring_amd.order_ops import pe_encode
    n, L, B = 10_000_000, 150, 256000
    G = n * L // 40
    flags = 10000 | (spring_amd.SYNTH_PAIRED if pe else 0)
    body = np.frombuffer(spring_amd.synth_dna_host(n, L, G, 33, flags), np.uint8).reshape(n, 2 + (L + 3) // 4)[:, 2:]
    j = np.arange(L)
    with spring_amd.ReorderStage(spring_amd.ReorderOpts(num_chains=0, num_thr=4)) as st:
        st.load_synth(n, L, G, 33, flags)
        st.run()
        with EncoderStage() as enc, StreamsStage() as ss, DecodeStage() as ds:
            enc.encode(st)
            order = enc.streams()["order"]
            ds.seq_from_encoder(enc)
            for preserve_order in ((False,) if pe else (False, True)):
                ss.from_encoder(enc, n, pe, preserve_order, B)
                info = ds.from_streams(ss)
                assert info["num_blocks"] == ss.info["num_blocks"] and info["pos_escapes"] == ss.info["pos_escapes"]
                if preserve_order:
                    ids = np.arange(n)
                else:
                    slot = pe_encode(order)[0] if pe else np.arange(n)
                    ids = np.empty(n, np.int64)
                    ids[slot] = order
                U = n // 2 if pe else n
                for m in range(2 if pe else 1):
                    data, off = ds.download(m)
                    assert np.array_equal(off, np.arange(U + 1, dtype=np.uint64) * L)
                    got = np.frombuffer(data, np.uint8).reshape(U, L)
                    part = ids[m * U:(m + 1) * U]
                    for lo in range(0, U, 1_000_000):   # in slices: a few hundred MB at a time
                        sel = part[lo:lo + 1_000_000]
                        codes = (body[sel][:, j >> 2] >> (2 * (j & 3)).astype(np.uint8)) & 3
                        assert np.array_equal(got[lo:lo + 1_000_000], np.frombuffer(b"AGCT", np.uint8)[codes]), (m, lo)
