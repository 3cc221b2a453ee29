"""CPU tests of the per-block read streams: the checker (tests/streams_model.py) against the decompressor's reader on
the encoder oracle's output and on hand-built corner cases, and the C ABI surface that needs no device."""
import ctypes as C
import functools
import os
import re
import subprocess

import numpy as np
import pytest

import streams_model as sm
from helpers import interleave_order_N, make_N_reads, named_set, read_strings
from oracle import pyoracle as po

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@functools.lru_cache(maxsize=None)
def encoded(name, nN=60, seed=4):
    """-> (encoder streams, original reads by original index, num_reads) of a named set with N reads."""
    dna, n, L = named_set(name)
    read, ln = po.load_dna(dna, n, L)
    strs = read_strings(read, ln)
    Nreads = make_N_reads(strs, nN + (n + nN) % 2, seed)   # an even total: the paired-end runs take every set
    order_N = interleave_order_N(n, len(Nreads), seed + 7)
    enc = po.encode(read, ln, L, po.reorder_rounds(read, ln, L, 6, 3), num_thr=3, dnaN=po.pack_dnaN(Nreads),
                    order_N=order_N)
    isN = np.zeros(n + len(Nreads), bool)
    isN[order_N] = True
    orig = [None] * (n + len(Nreads))
    for i, p in enumerate(np.flatnonzero(~isN)):
        orig[p] = strs[i]
    for i, p in enumerate(order_N):
        orig[p] = Nreads[i]
    return enc, orig, n + len(Nreads)


def slot_order(enc, paired_end, preserve_order):
    """record k -> slot; for paired-end data without preserve_order through pe_encode (spring.cpp:190-206)."""
    if preserve_order:
        return enc["order"]
    if paired_end:
        return po.pe_encode(enc["order"])
    return np.arange(len(enc["order"]), dtype=np.uint32)


def with_order(enc, order):
    e = dict(enc)
    e["order"] = np.asarray(order, np.uint32)
    return e


@pytest.mark.parametrize("name,pe", [("syn2k_100", False), ("var2k", False), ("test_1+2", True), ("syn5k_150", True)])
@pytest.mark.parametrize("preserve_order", [False, True])
@pytest.mark.parametrize("B", [1, 7, 1000, 1 << 30])
def test_checker_round_trip(name, pe, preserve_order, B):
    enc, orig, N = encoded(name)
    e = with_order(enc, slot_order(enc, pe, preserve_order))
    st = sm.write_streams(e, N, pe, preserve_order, B)
    U = N // 2 if pe else N
    assert len(st["read_flag.txt"][1]) == (U + B - 1) // B + 1
    got = sm.read_all(st, enc["seq"].decode(), N, pe, preserve_order, B)
    slot = np.asarray(e["order"]) if (pe or preserve_order) else np.arange(N)
    want = [None] * N
    for k in range(N):   # slot slot[k] holds record k, i.e. original read enc["order"][k]
        want[int(slot[k])] = orig[int(enc["order"][k])]
    assert got == want
    if preserve_order:
        assert got == orig   # the original order itself


def _blocks(pe, po_, B, shuffle=True):
    enc, seq, N, reads = sm.corner_case(pe, shuffle=shuffle)
    st = sm.write_streams(enc, N, pe, po_, B)
    return sm.blocks_of(st), st, enc, seq, N, reads


def _u64(v):
    return int(v).to_bytes(8, "little")


def _u16(v):
    return int(v).to_bytes(2, "little", signed=v < 0)


def test_corner_single_end_positions():
    bl, *_ = _blocks(False, False, 4, shuffle=False)
    # gap 65534 -> u16; gap 65535 -> escape; decreasing -> escape (uint64 wrap); block start -> absolute
    assert bl["read_pos.bin"][0] == (_u64(100) + _u16(65534) + _u16(65535) + _u64(100 + 65534 + 65535) + _u16(65535)
                                     + _u64(50))
    assert bl["read_pos.bin"][1] == _u64(7) + _u16(65535) + _u64(70000)
    assert bl["read_flag.txt"] == [b"0000", b"0022"]
    assert bl["read_unaligned.txt"][1] == b"ACGTNACGTNACGTNACGT" + b"NNACGTTGCAACGTTGCAAC"
    assert bl["read_lengths.bin"][1] == np.array([20, 20, 19, 20], np.uint16).tobytes()
    assert bl["read_noise.txt"] == [b"\n" * 4, b"\n" * 2]


def test_corner_paired_end_every_flag():
    bl, *_ = _blocks(True, False, 3)
    assert bl["read_flag.txt"] == [b"010", b"432", b"01"]
    # |pos_pair| = 32766 -> flag 0 (int16 pos2 - pos1), 32767 -> flag 1
    assert bl["read_pos_pair.bin"][0] == _u16(32766) + _u16(-32766)
    assert bl["read_rev_pair.txt"][0] == b"01"
    assert bl["read_pos.bin"][0] == (_u64(1000) + _u16(65534) + _u64(66534 + 32767) + _u16(65535) + _u64(132069))
    # block 1 starts with an unaligned read 1: the aligned read 1 after it is a delta against 0
    assert bl["read_pos.bin"][1] == _u64(500) + _u16(40)
    assert bl["read_rev.txt"][1] == b"dr"
    assert bl["read_unaligned.txt"][1] == (b"ACGTNACGTNACGTNACGTA" + b"TTTTTNNNNNAAAAACCCC" + b"GGGGGCCCCCAAAAATTTTT"
                                           + b"ACGTN")
    # block 2: absolute, then a decreasing position takes the escape; read 2 of flag 1 appends its absolute position
    assert bl["read_pos.bin"][2] == _u64(10) + _u16(65535) + _u64(5) + _u64(40005)
    assert bl["read_rev.txt"][2] == b"ddd"
    assert bl["read_pos_pair.bin"][2] == _u16(2) and bl["read_rev_pair.txt"][2] == b"0"
    assert bl["read_lengths.bin"][1] == np.array([20, 20, 20, 19, 20, 5], np.uint16).tobytes()


@pytest.mark.parametrize("pe", [False, True])
def test_corner_preserve_order_round_trip(pe):
    bl, st, enc, seq, N, reads = _blocks(pe, True, 3)
    assert sm.read_all(st, seq, N, pe, True, 3) == reads
    flags = b"".join(bl["read_flag.txt"])
    assert flags == (b"010432" + b"01" if pe else b"00000022")


def test_header_declarations_equal_streams_exports():
    from spring_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "spring_streams.h")).read()
    declared = set(re.findall(r"\b(spring_streams_\w+)\s*\(", hdr))
    assert declared == set(_lib.STREAMS_EXPORTS)
    assert not set(_lib.STREAMS_EXPORTS) & set(_lib.EXPORTS)
    L = _lib.lib()
    for name in sorted(declared):
        assert hasattr(L, name), name


def test_info_mirror_matches_the_c_layout(tmp_path):
    from spring_amd import _lib
    fields = [f for f, _ in _lib.StreamsInfo._fields_]
    src = tmp_path / "off.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "spring_streams.h"\nint main(void){\n'
                   'printf("%zu\\n", sizeof(spring_streams_info));\n'
                   + "".join('printf("%%zu\\n", offsetof(spring_streams_info, %s));\n' % f for f in fields)
                   + "return 0;}\n")
    exe = tmp_path / "off"
    subprocess.run(["gcc", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert got[0] == C.sizeof(_lib.StreamsInfo)
    assert got[1:] == [getattr(_lib.StreamsInfo, f).offset for f in fields]


def test_refusals_without_a_device(tmp_path):
    from spring_amd import _lib
    L = _lib.lib()
    info = _lib.StreamsInfo()
    assert L.spring_streams_create(0, None) == -1
    assert L.spring_streams_from_encoder(None, None, 0, 0, 0, 1, 0, C.byref(info)) == -1
    assert L.spring_streams_from_host(None, None, None, 0, None, 0, None, 0, None, None, 0, None, 0, 0, 0, 0, 1,
                                      C.byref(info)) == -1
    assert L.spring_streams_download(None, 0, None, None) == -1
    assert L.spring_streams_get_info(None, C.byref(info)) == -1
    assert L.spring_streams_run(None, 0, 0, 0, 1, -1, C.byref(info)) == -1
    L.spring_streams_destroy(None)
    # a directory without the encoder's files: an I/O error before any device is touched, nothing created
    d = str(tmp_path)
    assert L.spring_streams_run(d.encode(), 10, 0, 0, 1, -1, C.byref(info)) == -2
    assert os.listdir(d) == []
