"""The checker of the inverse block-sort stage (include/spring_unbwt.h): libbsc's bsc_bwt_decode restated in numpy from
its definition -- the n + 1 rows around the primary index, LF from a stable sort of the bytes, the walk from row 0 --
plus the real function from oracle/_ref/libref_units.so where that is built (tests/test_unbwt_cpu.py pins the one to
the other)."""
import ctypes as C

import numpy as np

import bwt_model as bm


def _lf(L, primary):
    """-> (LF over the n + 1 rows, -1 at the primary row; the byte of every row, 0 at the primary row)."""
    L = np.frombuffer(bytes(L), np.uint8) if not isinstance(L, np.ndarray) else L
    n = len(L)
    if not 1 <= primary <= n:
        raise ValueError("primary index %d out of range for %d bytes" % (primary, n))
    q = np.arange(n)
    row = np.where(q < primary, q, q + 1)
    order = np.argsort(L, kind="stable")          # place t holds the byte of row row[order[t]]
    lf = np.full(n + 1, -1, np.int64)
    lf[row[order]] = np.arange(n) + 1
    byte = np.zeros(n + 1, np.uint8)
    byte[row] = L
    return lf, byte


def path_length(L, primary):
    """Steps from row 0 to the primary row; n for the transform of a text."""
    n = len(L)
    if n == 0:
        return 0
    lf = _lf(L, primary)[0].tolist()
    r, steps = 0, 0
    while r != primary and steps <= n:
        r = lf[r]
        steps += 1
    return steps


def unbwt(L, primary):
    """-> the text (bytes).  ValueError when the primary index is out of range or the path from row 0 is short."""
    n = len(L)
    if n == 0:
        if primary != 0:
            raise ValueError("primary index %d for an empty segment" % primary)
        return b""
    lf, byte = _lf(L, primary)
    lf, byte = lf.tolist(), byte.tolist()
    T = bytearray(n)
    r = 0
    for i in range(n - 1, -1, -1):
        if r == primary:
            raise ValueError("the path from row 0 has %d of %d steps" % (n - 1 - i, n))
        T[i] = byte[r]
        r = lf[r]
    assert r == primary
    return bytes(T)


def ref_lib():
    """oracle/_ref/libref_units.so with bsc_bwt_decode typed as well, or None when it is not built."""
    U = bm.ref_lib()
    if U is not None and not getattr(U, "_unbwt_typed", False):
        U.bsc_bwt_decode.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_ubyte, C.c_void_p, C.c_int]
        U._unbwt_typed = True
    return U


def ref_unbwt(L, primary, features=0, indexes=None):
    """The real bsc_bwt_decode -> (return code, bytes)."""
    U = ref_lib()
    buf = np.frombuffer(bytes(L), np.uint8).copy()
    idx = None if indexes is None else np.ascontiguousarray(indexes, np.int32)
    rc = U.bsc_bwt_decode(buf.ctypes.data if len(buf) else None, len(buf), primary, 0 if idx is None else len(idx),
                          None if idx is None else idx.ctypes.data, features)
    return rc, buf.tobytes()
