"""The checker of the BSC framing stage (include/spring_bsc.h): a plain-Python restatement (struct + zlib.adler32) of
libbsc's block header and store rule (reference src/libbsc/libbsc/libbsc/libbsc.cpp:77-90, :201-305) and of the two file
framings (libbsc/bsc.cpp:149-156, :306-379; libbsc/bsc_str_array.cpp:183-250, :451-458) under SPRING's settings: no LZP,
BWT, static QLFC, recordSize 1, contexts following.  The transform and the coded bytes are inputs: the model frames
what the block sort and the coder gave.  Below it, the real bsc_compress / bsc_store / bsc_adler32 /
bsc_compress-in-place of oracle/_ref/libref_units.so and the ref_bsc program, where they are built; and the cases the
GPU tests and the CPU tests share."""
import ctypes as C
import os
import struct
import subprocess
import tempfile
import zlib

import numpy as np

import bwt_model as bm

HEADER = 28
MODE = 1 | (1 << 5)
INDEX_MIN = 65536
FOLLOWING = 1                      # LIBBSC_CONTEXTS_FOLLOWING
NOT_COMPRESSIBLE = -3              # LIBBSC_NOT_COMPRESSIBLE
CODED, STORED_SMALL, STORED_CODER, STORED_NO_GAIN = range(4)
BLOCKS, BSC_FILE, STR_ARRAY = range(3)


def adler(b):
    return zlib.adler32(bytes(b)) & 0xffffffff


def store(data):
    """bsc_store."""
    a = adler(data)
    head = struct.pack("<iiiiII", len(data) + HEADER, len(data), 0, 0, a, a)
    return head + struct.pack("<I", adler(head)) + bytes(data)


def outcome(n, rc, num_indexes):
    """rc: what bsc_coder_compress returned (the size, or a negative value)."""
    k = 0 if n < INDEX_MIN else num_indexes
    if n <= HEADER:
        return STORED_SMALL
    if rc < 0:
        return STORED_CODER
    if rc + 1 + 4 * k >= n:
        return STORED_NO_GAIN
    return CODED


def block(data, primary, indexes, coded, rc):
    """bsc_compress(., ., n, 0, 0, 1, 1, features) with bsc_store where it (or its in-place form) answers not
    compressible -> (the block, the outcome).  indexes: the secondary indexes the block sort reports."""
    n = len(data)
    kind = outcome(n, rc, len(indexes))
    if kind != CODED:
        return store(data), kind
    k = 0 if n < INDEX_MIN else len(indexes)
    body = bytes(coded) + struct.pack("<%di" % k, *[int(x) for x in indexes[:k]]) + bytes([k])
    head = struct.pack("<iiiiII", len(body) + HEADER, n, MODE, int(primary), adler(data), adler(body))
    return head + struct.pack("<I", adler(head)) + body, kind


def cuts(n, block_bytes):
    """Compression()'s cut of n bytes -> [(lo, hi)]; none for n = 0."""
    return [(lo, min(lo + block_bytes, n)) for lo in range(0, n, block_bytes)]


def bsc_file(blocks):
    """BSC_compress's file: blocks = [(offset of the cut in the input, block bytes)]."""
    return struct.pack("<i", len(blocks)) + b"".join(struct.pack("<qbb", off, 1, FOLLOWING) + b for off, b in blocks)


def str_array_file(blocks):
    """BSC_str_array_compress's file: blocks = [block bytes]."""
    return struct.pack("<i", len(blocks)) + b"".join(struct.pack("<bb", 1, FOLLOWING) + b for b in blocks)


def frame(framing, blocks):
    """blocks = [(offset, block bytes)] of one file."""
    if framing == BLOCKS:
        return b"".join(b for _, b in blocks)
    return bsc_file(blocks) if framing == BSC_FILE else str_array_file([b for _, b in blocks])


def parse_block(blk):
    """-> dict of the header fields and the body; checks the three sums."""
    size, n, mode, primary, a_in, a_body, a_head = struct.unpack_from("<iiiiIII", blk)
    assert size == len(blk) and a_head == adler(blk[:24]) and a_body == adler(blk[HEADER:])
    return dict(size=size, n=n, mode=mode, primary=primary, adler_in=a_in, body=blk[HEADER:])


# ---------------------------------------------------------------------------------------------- the real functions
def ref_lib():
    U = bm.ref_lib()
    if U is not None and not getattr(U, "_frame_typed", False):
        U.bsc_store.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int]
        U._frame_typed = True
    return U


FEATURES = bm.FASTMODE | bm.MULTITHREADING


def ref_adler(data):
    a = np.frombuffer(bytes(data), np.uint8).copy()
    return int(ref_lib().bsc_adler32(a.ctypes.data if len(a) else None, len(a), FEATURES))


def ref_store(data):
    a = np.frombuffer(bytes(data), np.uint8).copy()
    out = np.zeros(len(a) + HEADER, np.uint8)
    size = ref_lib().bsc_store(a.ctypes.data if len(a) else None, out.ctypes.data, len(a), FEATURES)
    return out[:size].tobytes()


def ref_block(data):
    """The real bsc_compress(in, out, n, 0, 0, 1, 1, 3), then the real bsc_store where it says not compressible."""
    a = np.frombuffer(bytes(data), np.uint8).copy()
    out = np.zeros(len(a) + HEADER + 4096, np.uint8)
    size = ref_lib().bsc_compress(a.ctypes.data if len(a) else None, out.ctypes.data, len(a), 0, 0, 1, 1, FEATURES)
    if size == NOT_COMPRESSIBLE:
        return ref_store(data)
    assert size >= HEADER, size
    return out[:size].tobytes()


def ref_inplace_rc(data):
    """What the in-place bsc_compress, the one Compression() calls, returns: the size or LIBBSC_NOT_COMPRESSIBLE."""
    a = np.zeros(len(data) + HEADER + 4096, np.uint8)
    a[:len(data)] = np.frombuffer(bytes(data), np.uint8)
    return int(ref_lib().bsc_compress(a.ctypes.data, a.ctypes.data, len(data), 0, 0, 1, 1, FEATURES))


def ref_decompress(blk, n):
    a = np.frombuffer(bytes(blk), np.uint8).copy()
    back = np.zeros(max(n, 1), np.uint8)
    rc = ref_lib().bsc_decompress(a.ctypes.data, len(a), back.ctypes.data, n, FEATURES)
    return back[:n].tobytes(), rc


def ref_bsc_bin():
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle", "_ref", "ref_bsc")
    return path if os.path.exists(path) else None


def ref_bsc_file(data):
    """The ref_bsc program (the real BSC_compress, 64 MiB blocks) on a file holding data -> the file it writes."""
    with tempfile.TemporaryDirectory() as d:
        src, dst = os.path.join(d, "in"), os.path.join(d, "out")
        with open(src, "wb") as f:
            f.write(data)
        subprocess.run([ref_bsc_bin(), src, dst], check=True, stdout=subprocess.DEVNULL)
        return open(dst, "rb").read()


# ---------------------------------------------------------------------------------------------- cases
# Stored although the coder succeeds: NO_GAIN_N random bytes (seed NO_GAIN_SEED), then a run of zero bytes.  Found
# with the real functions by scanning the run's length (tests/test_bsc_cpu.py pins the branches where they are built):
# the coder gives r = 66799 bytes from a run of 810 bytes on (below that it reports not compressible) and the block
# sort 8 indexes, so r + 1 + 4 * 8 = 66832.  NO_GAIN_RUN (n = 66820) is stored with 12 bytes to spare, NO_GAIN_EQ_RUN
# is r + 1 + 4 k' = n, still stored, and GAIN_RUN is r + 1 + 4 k' = n - 1, the first length that is coded.
NO_GAIN_N, NO_GAIN_SEED = 66000, 7
NO_GAIN_RUN, NO_GAIN_EQ_RUN, GAIN_RUN = 820, 832, 833
NO_GAIN_CODED = 66799


def no_gain_case(run=NO_GAIN_RUN):
    return np.random.default_rng(NO_GAIN_SEED).integers(0, 256, NO_GAIN_N).astype(np.uint8).tobytes() + bytes(run)


def text(n, seed=3):
    """Compressible text of n bytes: words of a small vocabulary."""
    rng = np.random.default_rng(seed)
    words = [bytes(rng.integers(97, 123, int(k)).astype(np.uint8)) for k in rng.integers(2, 9, 200)]
    out, size = [], 0
    while size < n:
        w = words[int(rng.integers(0, len(words)))] + b" "
        out.append(w)
        size += len(w)
    return b"".join(out)[:n]


SUM_TILE = 4096   # bsc_frame_plan.h: TILE
SUM_LENGTHS = (0, 1, 15, 16, 17, SUM_TILE - 1, SUM_TILE, SUM_TILE + 1, 2 * SUM_TILE + 3, 5552, 5553, 65520, 65521, 65522)


def sum_batch():
    """-> (bytes, offsets): SUM_LENGTHS of random bytes, then 16 segments of 100 bytes with a filler in front of each
    that puts their starts at every residue mod 16, then 1 MiB + 1 and 64 MiB + 1 bytes of 0xFF."""
    rng = np.random.default_rng(12)
    segs = [rng.integers(0, 256, n).astype(np.uint8).tobytes() for n in SUM_LENGTHS]
    at = sum(len(s) for s in segs)
    for res in range(16):
        fill = (res - at) % 16
        segs += [rng.integers(0, 256, fill).astype(np.uint8).tobytes(), rng.integers(0, 256, 100).astype(np.uint8).tobytes()]
        at += fill + 100
    segs += [b"\xff" * ((1 << 20) + 1), b"\xff" * ((64 << 20) + 1)]
    off = np.cumsum([0] + [len(s) for s in segs]).astype(np.uint64)
    return b"".join(segs), off
