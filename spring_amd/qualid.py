"""Host-side mirror of the quality and id stage (the quality / id side of reference src/preprocess.cpp:200-250 and
src/reorder_compress_quality_id.cpp:34-235, up to their codec calls) on top of the C ABI in
include/spring_qualid.h.  All compute is in the HIP library; no CPU fallback."""
import ctypes as C

import numpy as np

from . import _lib
from ._stage import ReorderError, Stage, chk

QUALITY, ID = 0, 1
KIND = {"quality": QUALITY, "id": ID, QUALITY: QUALITY, ID: ID}


def _u8(b):
    """bytes-like or array -> (contiguous uint8 array, pointer or None)."""
    a = b if isinstance(b, np.ndarray) else np.frombuffer(b, np.uint8)
    a = np.ascontiguousarray(a, np.uint8)
    return a, (a.ctypes.data if len(a) else None)


def quality_table(mode, thr=0, high=0, low=0):
    """The 128-byte quantization table of preprocess: mode "illumina" (8-level binning, util.cpp:166-180) or "binary"
    (byte < 33 + thr -> 33 + low, else 33 + high; util.cpp:182-188).  Host only."""
    m = {"illumina": 1, "ill_bin": 1, "binary": 2}.get(mode, mode)
    t = np.zeros(128, np.uint8)
    chk(_lib.lib().spring_quality_table(int(m), thr, high, low, t.ctypes.data))
    return t


def id_pattern(fastq_1, fastq_2, device=-1):
    """paired_id_code 0..3 of two FASTQ texts (find_id_pattern on the first pair, check_id_pattern on every pair on
    the device; util.cpp:196-253)."""
    a, pa = _u8(fastq_1)
    b, pb = _u8(fastq_2)
    code, ms = C.c_uint8(0), C.c_double(0)
    chk(_lib.lib().spring_id_pattern(pa, len(a), pb, len(b), device, C.byref(code), C.byref(ms)))
    return int(code.value)


class QualIdStage(Stage):
    """set_order() / set_order_from_encoder(), then from_fastq() / from_lines(): the quality lines and id lines of one
    input file in the final read order, cut into blocks of num_reads_per_block reads (pairs), on the device.
    download(kind) / blocks(kind) fetch a result."""

    quality_table = staticmethod(quality_table)
    id_pattern = staticmethod(id_pattern)

    _prefix, _Info = "spring_qualid", _lib.QualIdInfo

    def __init__(self, device: int = -1):
        super().__init__(device)
        self._B = 0

    def set_order(self, order, num_reads, paired_end=False):
        """order: the image of read_order.bin before pe_encode (num_reads entries), or None for the identity
        (preserve_order)."""
        self.info = None
        if order is not None:
            order = np.ascontiguousarray(order, dtype=np.uint32)
            if len(order) != num_reads:
                raise ReorderError("order holds %d entries, num_reads is %d" % (len(order), num_reads))
        chk(self._L.spring_qualid_order_from_host(self._h, None if order is None or not len(order) else order.ctypes.data,
                                                  num_reads, int(paired_end)))

    def set_order_from_encoder(self, enc, num_reads, paired_end=False):
        """enc: an EncoderStage after encode(); its order stays in HBM and is left as it was."""
        self.info = None
        chk(self._L.spring_qualid_order_from_encoder(self._h, enc._h, num_reads, int(paired_end)))

    def from_fastq(self, fastq, want=("quality", "id"), table=None, num_reads_per_block=256000):
        """fastq: the text (or gzip image) of one input file.  want: the kinds to build.  table: 128 bytes or None."""
        bits = sum(1 << KIND[k] for k in ((want,) if isinstance(want, (str, int)) else want))
        a, pa = _u8(fastq)
        t, pt = (None, None) if table is None else _u8(table)
        if t is not None and len(t) != 128:
            raise ReorderError("the quality table has 128 entries")
        self._run("from_fastq", pa, len(a), bits, pt, num_reads_per_block)
        self._B = num_reads_per_block
        return self.info

    def from_lines(self, kind, lines, table=None, num_reads_per_block=256000):
        """lines: the image of quality_j / id_j as preprocess writes them, one '\\n'-terminated line per read."""
        a, pa = _u8(lines)
        t, pt = (None, None) if table is None else _u8(table)
        if t is not None and len(t) != 128:
            raise ReorderError("the quality table has 128 entries")
        self._run("from_lines", KIND[kind], pa, len(a), pt, num_reads_per_block)
        self._B = num_reads_per_block
        return self.info

    def download(self, kind):
        """-> (bytes of all blocks back to back, line lengths in slot order: uint32, block offsets: uint64)."""
        k = KIND[kind]
        if self.info is None:   # nothing computed (or the last call failed): the library says so
            chk(self._L.spring_qualid_download(self._h, k, None, None, None))
        n = self.info["bytes"][k]
        buf = np.zeros(max(n, 1), np.uint8)
        ln = np.zeros(max(self.info["num_units"], 1), np.uint32)
        off = np.zeros(self.info["num_blocks"] + 1, np.uint64)
        chk(self._L.spring_qualid_download(self._h, k, buf.ctypes.data, ln.ctypes.data, off.ctypes.data))
        return buf[:n].tobytes(), ln[:self.info["num_units"]], off

    def blocks(self, kind):
        """-> per block the list of its lines (bytes, without the id's '\\n'): the string array a codec call takes."""
        data, ln, off = self.download(kind)
        nl = 1 if KIND[kind] == ID else 0
        B, U = self._B, len(ln)
        start = np.concatenate([[0], np.cumsum(ln.astype(np.int64) + nl)])
        return [[data[int(start[s]):int(start[s]) + int(ln[s])] for s in range(b * B, min((b + 1) * B, U))]
                for b in range(len(off) - 1)]
