"""GPU tests of the per-block read streams (include/spring_streams.h) against the checker tests/streams_model.py:
every stream and the block table byte for byte, the device pe_encode, the file contract, one run at size."""
import functools
import os

import numpy as np
import pytest

import ref_cases as rc
import streams_model as sm
from helpers import interleave_order_N, make_N_reads, named_set, read_strings
from oracle import pyoracle as po

pytestmark = pytest.mark.gpu


def _same(stage, want, what=""):
    info = stage.info
    assert info["num_blocks"] + 1 == len(next(iter(want.values()))[1]), what
    for s, (data, off) in want.items():
        got, goff = stage.download(s)
        assert np.array_equal(goff, off), (what, s, "block table")
        assert got == data, (what, s)
    for s in sm.STREAMS:
        if s not in want:
            assert info["bytes"][sm.STREAMS.index(s)] == 0, (what, s)


@functools.lru_cache(maxsize=None)
def _set(name, nN=80, seed=5):
    dna, n, L = named_set(name)
    read, ln = po.load_dna(dna, n, L)
    Nreads = make_N_reads(read_strings(read, ln), nN + (n + nN) % 2, seed)
    return dna, n, L, po.pack_dnaN(Nreads), interleave_order_N(n, len(Nreads), seed + 7)


@pytest.mark.parametrize("name,pe", [("syn5k_150", False), ("var2k", False), ("test_1+2", True), ("syn2k_100", True)])
def test_gpu_equals_checker_from_encoder_and_host(name, pe):
    import spring_amd
    from spring_amd.encoder import EncoderStage
    from spring_amd.streams import StreamsStage
    dna, n, L, dnaN, order_N = _set(name)
    N = n + len(order_N)
    with spring_amd.ReorderStage(spring_amd.ReorderOpts(num_chains=8, num_thr=2)) as st:
        st.load_dna(dna, n, L)
        st.run()
        with EncoderStage() as enc, StreamsStage() as ss:
            enc.encode(st, dnaN, order_N)
            e = enc.streams()
            for preserve_order in (False, True):
                order = po.pe_encode(e["order"]) if (pe and not preserve_order) else e["order"]
                ew = dict(e, order=order)
                for B in (1, 7, 256000):
                    want = sm.write_streams(ew, N, pe, preserve_order, B)
                    info = ss.from_encoder(enc, N, pe, preserve_order, B)
                    assert info["n_aligned"] == len(e["pos"])
                    _same(ss, want, (name, preserve_order, B, "encoder"))
                    ss.from_host(e["pos"], e["rc"], e["noise"], e["noisepos"],
                                 order if (pe or preserve_order) else None, e["rlen"], e["unaligned"], N, pe,
                                 preserve_order, B)
                    _same(ss, want, (name, preserve_order, B, "host"))
                    fl = np.frombuffer(ss.download("flag")[0], np.uint8) - ord("0")
                    assert np.array_equal(np.bincount(fl, minlength=5), info["flag_count"])
            # the encoder's own order is untouched by the device pe_encode
            assert np.array_equal(enc.streams()["order"], e["order"])


@pytest.mark.parametrize("pe", [False, True])
@pytest.mark.parametrize("preserve_order", [False, True])
@pytest.mark.parametrize("B", [1, 3, 4, 1000])
def test_gpu_corner_cases_from_host(pe, preserve_order, B):
    from spring_amd.streams import StreamsStage
    enc, seq, N, reads = sm.corner_case(pe, shuffle=pe or preserve_order)
    want = sm.write_streams(enc, N, pe, preserve_order, B)
    with StreamsStage() as ss:
        info = ss.from_host(enc["pos"], enc["rc"], enc["noise"], enc["noisepos"], enc["order"], enc["rlen"],
                            enc["unaligned"], N, pe, preserve_order, B)
        _same(ss, want, (pe, preserve_order, B))
        if not preserve_order and pe and B == 3:
            assert info["pos_escapes"] == 2 and info["flag_count"] == [3, 2, 1, 1, 1]


@pytest.mark.parametrize("case", sorted(rc.STREAM_FIXTURES))
def test_gpu_equals_reference_written_blocks(case):
    """Every stream and block table against what the reference's own reorder_compress_streams wrote for the case
    (tests/golden/ref_streams_<case>.npz, recorded by tests/golden/make_ref_golden.py): no model in between."""
    from spring_amd.streams import StreamsStage
    g = rc.load_stream_fixture(case)
    enc = g["enc"]
    with StreamsStage() as ss:
        info = ss.from_host(enc["pos"], enc["rc"], enc["noise"], enc["noisepos"], enc["order"], enc["rlen"],
                            enc["unaligned"], g["N"], g["pe"], g["preserve_order"], g["B"])
        _same(ss, g["streams"], case)
        flags = np.frombuffer(g["streams"]["read_flag.txt"][0], np.uint8) - ord("0")
        assert np.array_equal(np.bincount(flags, minlength=5), info["flag_count"])
        assert info["num_blocks"] == ((g["N"] // 2 if g["pe"] else g["N"]) + g["B"] - 1) // g["B"]


def test_gpu_refuses_bad_input():
    from spring_amd.reorder import ReorderError
    from spring_amd.streams import StreamsStage
    enc, seq, N, reads = sm.corner_case(True)
    args = lambda **kw: [kw.get(k, enc[k]) for k in ("pos", "rc", "noise", "noisepos", "order", "rlen", "unaligned")]  # noqa: E731
    dup = enc["order"].copy()
    dup[1] = dup[0]
    big = enc["order"].copy()
    big[2] = N
    un_bad = bytearray(enc["unaligned"])
    un_bad[2] = 0x77   # base codes 7: not A G C T N
    with StreamsStage() as ss:
        for a, n, pe, B in ((args(order=dup), N, True, 3), (args(order=big), N, True, 3), (args(), N + 2, True, 3),
                            (args(), N, True, 0), (args(noise=enc["noise"][:-1]), N, True, 3),
                            (args(noise=b"1" + enc["noise"]), N, True, 3), (args(unaligned=bytes(un_bad)), N, True, 3),
                            (args(unaligned=enc["unaligned"][:-1]), N, True, 3)):
            with pytest.raises(ReorderError, match="code -1"):
                ss.from_host(*a, n, pe, True, B)
        e1, *_ = sm.corner_case(False)
        odd = {k: e1[k] for k in e1}
        with pytest.raises(ReorderError, match="even"):
            ss.from_host(odd["pos"], odd["rc"], odd["noise"], odd["noisepos"], odd["order"][:7],
                         odd["rlen"][:7], b"", 7, True, False, 3)
        with pytest.raises(ReorderError):
            ss.download(0)   # nothing computed by a failed call


def test_device_pe_encode_equals_host_pe_encode():
    import spring_amd
    from spring_amd.encoder import EncoderStage
    from spring_amd.order_ops import pe_encode
    from spring_amd.streams import StreamsStage
    dna, n, L, dnaN, order_N = _set("test_1+2")
    N = n + len(order_N)
    with spring_amd.ReorderStage(spring_amd.ReorderOpts(num_chains=4, num_thr=1)) as st:
        st.load_dna(dna, n, L)
        st.run()
        with EncoderStage() as enc, StreamsStage() as a, StreamsStage() as b:
            enc.encode(st, dnaN, order_N)
            e = enc.streams()
            a.from_encoder(enc, N, True, False, 100)
            host_order, _ = pe_encode(e["order"])
            b.from_host(e["pos"], e["rc"], e["noise"], e["noisepos"], host_order, e["rlen"], e["unaligned"], N, True,
                        False, 100)
            for s in sm.STREAMS:
                assert a.download(s)[0] == b.download(s)[0], s
            assert np.array_equal(enc.streams()["order"], e["order"])


def _files(d):
    return {f: open(os.path.join(d, f), "rb").read() for f in sorted(os.listdir(d))}


@pytest.mark.parametrize("pe,preserve_order", [(False, False), (False, True), (True, False), (True, True)])
def test_file_contract(tmp_path, pe, preserve_order):
    from spring_amd.encoder import call_reorder_encoder
    from spring_amd.order_ops import pe_encode
    from spring_amd.reorder import CompressionParams, ReorderError
    from spring_amd.streams import call_reorder_compress_streams
    import spring_amd
    from readsets import pack_var
    dna, n, L = named_set("test_1+2" if pe else "syn2k_100")
    d = str(tmp_path)
    B = 100
    if pe:  # two files of equal length: the pool's reads split in halves
        read, ln = po.load_dna(dna, n, L)
        strs = read_strings(read, ln)
        half = n // 2
        n = 2 * half
        open(os.path.join(d, "input_clean_1.dna"), "wb").write(pack_var([x.encode() for x in strs[:half]]))
        open(os.path.join(d, "input_clean_2.dna"), "wb").write(pack_var([x.encode() for x in strs[half:n]]))
        cp = CompressionParams(L, [half, half], num_thr=2, paired_end=True)
    else:
        open(os.path.join(d, "input_clean_1.dna"), "wb").write(dna)
        cp = CompressionParams(L, [n, 0], num_thr=2)
    call_reorder_encoder(d, cp, n, spring_amd.ReorderOpts(num_chains=8, num_thr=2))
    enc_files = _files(d)
    enc = dict(pos=np.frombuffer(enc_files["read_pos.bin"], np.uint64), rc=enc_files["read_rev.txt"],
               noise=enc_files["read_noise.txt"], noisepos=np.frombuffer(enc_files["read_noisepos.bin"], np.uint16),
               order=np.frombuffer(enc_files["read_order.bin"], np.uint32),
               rlen=np.frombuffer(enc_files["read_lengths.bin"], np.uint16), unaligned=enc_files["read_unaligned.txt"])
    if pe and not preserve_order:   # spring.cpp:190-206: pe_encode rewrites read_order.bin first
        enc["order"], _ = pe_encode(enc["order"])
        open(os.path.join(d, "read_order.bin"), "wb").write(enc["order"].tobytes())
    # a duplicate entry in read_order.bin: refused, the directory untouched (for the modes that read the file)
    if pe or preserve_order:
        good = open(os.path.join(d, "read_order.bin"), "rb").read()
        bad = np.frombuffer(good, np.uint32).copy()
        bad[3] = bad[4]
        open(os.path.join(d, "read_order.bin"), "wb").write(bad.tobytes())
        before = _files(d)
        with pytest.raises(ReorderError, match="code -1"):
            call_reorder_compress_streams(d, cp, preserve_order, B, num_reads=n)
        assert _files(d) == before
        open(os.path.join(d, "read_order.bin"), "wb").write(good)
    seq_files = {f: v for f, v in _files(d).items() if f.startswith("read_seq.bin")}
    info = call_reorder_compress_streams(d, cp, preserve_order, B, num_reads=n)
    want = sm.blocks_of(sm.write_streams(enc, n, pe, preserve_order, B))
    nb = info["num_blocks"]
    expect = {"%s.%d" % (s, b): want[s][b] for s in sm.stream_names(pe) for b in range(nb)}
    expect.update(seq_files)   # the encoder's packed consensus stays for its own BSC loop
    assert nb == ((n // 2 if pe else n) + B - 1) // B
    assert _files(d) == expect
    assert info["ms_file"] > 0


def test_ten_million_reads_at_size():
    """>= 10 M synthetic single-end reads, both order modes: per-stream totals and the block tables equal the checker's
    closed-form sizes; first, middle and last blocks byte for byte, and the reader restores their reads."""
    import time

    import spring_amd
    from spring_amd.encoder import EncoderStage
    from spring_amd.streams import StreamsStage
    t0 = time.time()
    n, L, B = 10_000_000, 100, 256000
    G = n * L // 40
    with spring_amd.ReorderStage(spring_amd.ReorderOpts(num_chains=0, num_thr=4)) as st:
        st.load_synth(n, L, G, 33)
        st.run()
        with EncoderStage() as enc, StreamsStage() as ss:
            enc.encode(st)
            e = enc.streams()
            body = np.frombuffer(spring_amd.synth_dna_host(n, L, G, 33), np.uint8).reshape(n, 2 + (L + 3) // 4)[:, 2:]
            for preserve_order in (False, True):
                info = ss.from_encoder(enc, n, False, preserve_order, B)
                want = sm.write_streams(e, n, False, preserve_order, B)
                nb = info["num_blocks"]
                assert nb == (n + B - 1) // B
                for s, (data, off) in want.items():
                    got, goff = ss.download(s)
                    assert np.array_equal(goff, off), s
                    assert info["bytes"][sm.STREAMS.index(s)] == len(data), s
                    for b in (0, nb // 2, nb - 1):
                        assert got[int(goff[b]):int(goff[b + 1])] == data[int(off[b]):int(off[b + 1])], (s, b)
                wb = sm.blocks_of(want)
                j = np.arange(L)
                for b in (0, nb // 2, nb - 1):
                    nu = min(B, n - b * B)
                    reads = sm.read_block({s: v[b] for s, v in wb.items()}, e["seq"].decode(), nu, False,
                                          preserve_order)
                    slots = np.arange(b * B, b * B + nu)
                    orig_ids = slots if preserve_order else e["order"][slots]
                    codes = (body[orig_ids][:, j >> 2] >> (2 * (j & 3)).astype(np.uint8)) & 3
                    orig = np.frombuffer(b"AGCT", np.uint8)[codes]
                    assert np.array_equal(np.frombuffer("".join(reads).encode(), np.uint8).reshape(nu, L), orig), b
    assert time.time() - t0 <= 60
