"""The checker of the block-sort stage (include/spring_bwt.h): libbsc's bsc_bwt_encode restated in numpy from its
definition -- suffix order with the end of the string below every byte, the byte in front of every suffix but the
first around the primary index, the sampled ranks (divsufsort.c:1704-1727) -- plus the real function from
oracle/_ref/libref_units.so where that is built (tests/test_bwt_cpu.py pins the one to the other)."""
import ctypes as C

import numpy as np

from oracle import pyoracle as po

FASTMODE, MULTITHREADING = 1, 2
LENGTHS = [0, 1, 2, 3, 7, 8, 9, 15, 16, 17, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4097]


def suffix_ranks(T):
    """rank[i] of suffix T[i:] among all suffixes (a proper prefix sorts first), by prefix doubling."""
    T = np.frombuffer(bytes(T), np.uint8) if not isinstance(T, np.ndarray) else T
    n = len(T)
    r = T.astype(np.int64) + 1          # 0 is "past the end"
    mult = max(n, 256) + 2
    h = 1
    while True:
        r2 = np.zeros(n, np.int64)
        if h < n:
            r2[:n - h] = r[h:]
        key = r * mult + r2
        order = np.argsort(key, kind="stable")
        ks = key[order]
        newr = np.cumsum(np.concatenate(([1], (ks[1:] != ks[:-1]).astype(np.int64))))
        r = np.empty(n, np.int64)
        r[order] = newr
        if newr[-1] == n:
            return r - 1
        h *= 2


def index_step(n):
    mod = n // 8
    for s in (1, 2, 4, 8, 16):
        mod |= mod >> s
    return (mod >> 1) + 1


def bwt(T):
    """-> (the n output bytes, primary index, the secondary indexes as an int32 array)."""
    T = np.frombuffer(bytes(T), np.uint8) if not isinstance(T, np.ndarray) else T
    n = len(T)
    if n == 0:
        return b"", 0, np.zeros(0, np.int32)
    rank = suffix_ranks(T)
    sa = np.empty(n, np.int64)
    sa[rank] = np.arange(n)
    out = np.empty(n, np.uint8)
    out[0] = T[n - 1]
    out[1:] = T[sa[sa > 0] - 1]
    step = index_step(n)
    num = ((n - 1) // step) & 0xff
    idx = rank[(np.arange(num) + 1) * step].astype(np.int32)
    return out.tobytes(), int(rank[0]) + 1, idx


def ref_lib():
    """oracle/_ref/libref_units.so with libbsc's entry points typed, or None when it is not built."""
    U = po.ref_units()
    if U is None:
        return None
    if not getattr(U, "_bsc_typed", False):
        U.bsc_init.argtypes = [C.c_int]
        U.bsc_bwt_encode.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_ubyte), C.c_void_p, C.c_int]
        U.bsc_coder_compress.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int]
        U.bsc_compress.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]
        U.bsc_decompress.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int]
        U.bsc_adler32.argtypes = [C.c_void_p, C.c_int, C.c_int]
        U.bsc_adler32.restype = C.c_uint
        assert U.bsc_init(FASTMODE | MULTITHREADING) == 0
        U._bsc_typed = True
    return U


def ref_bwt(T, features=0):
    """The real bsc_bwt_encode -> (bytes, primary index, indexes)."""
    U = ref_lib()
    buf = np.frombuffer(bytes(T), np.uint8).copy()
    num = C.c_ubyte(0)
    idx = np.zeros(256, np.int32)
    primary = U.bsc_bwt_encode(buf.ctypes.data, len(buf), C.byref(num), idx.ctypes.data, features)
    assert primary >= 0, primary
    return buf.tobytes(), primary, idx[:num.value].copy()


def contents(kind, n, seed=0):
    """The test contents by name."""
    rng = np.random.default_rng(seed * 1000003 + n)
    if kind == "acgt":
        return np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, n)].tobytes()
    if kind == "bytes":
        return rng.integers(0, 256, n, dtype=np.uint8).tobytes()
    if kind == "const":
        return b"A" * n
    if kind == "cac":
        return (b"CAC" * (n // 3 + 1))[:n]
    if kind in ("tail00", "tailff"):
        body = rng.integers(0, 256, n - n // 3, dtype=np.uint8).tobytes()
        return body + (b"\x00" if kind == "tail00" else b"\xff") * (n // 3)
    raise ValueError(kind)


POOL_LENGTHS = {"acgt": (1, 7, 31, 64, 90, 150, 210, 256, 299, 300), "bytes": (2, 8, 15, 65, 100, 180, 255, 300),
                "const": (1, 2, 3, 63, 150, 257, 300), "cac": (3, 9, 100, 300), "tail00": (3, 17, 128, 300),
                "tailff": (3, 16, 64, 129, 300)}


def segment_pool():
    """38 distinct texts of 1 .. 300 bytes of every kind, and the empty one."""
    pool = [b""] + [contents(kind, n, seed=5) for kind, lens in POOL_LENGTHS.items() for n in lens]
    assert len(set(pool)) == len(pool) == 39 and max(len(t) for t in pool) == 300
    return pool


def pool_batch(S, seed=17):
    """S segments drawn from segment_pool() (a model result per distinct text serves the whole batch): one segment in
    nine is empty, one in eight repeats its neighbour, three empties stand in a row, and segments 40 and 8000 (where
    the batch has them) are the 300 random bytes of ACGT and the 255 random bytes."""
    pool = segment_pool()
    rng = np.random.default_rng(seed * 1000003 + S)
    idx = rng.integers(1, len(pool), S)
    idx[rng.random(S) < 1 / 9] = 0
    rep = np.flatnonzero(rng.random(S) < 1 / 8)
    rep = rep[rep > 0]
    idx[rep] = idx[rep - 1]
    idx[5:8] = 0
    for s, text in ((40, contents("acgt", 300, seed=5)), (8000, contents("bytes", 255, seed=5))):
        if s < S:
            idx[s] = pool.index(text)
    return [pool[i] for i in idx]


def dna_with_repeats(n, seed=3):
    """DNA-like text with planted repeats of 300 and 5000 bytes."""
    rng = np.random.default_rng(seed)
    t = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, n)].copy()
    for length, copies in ((300, 40), (5000, 6)):
        src = int(rng.integers(0, n - length))
        piece = t[src:src + length].copy()
        for _ in range(copies):
            dst = int(rng.integers(0, n - length))
            t[dst:dst + length] = piece
    return t.tobytes()
