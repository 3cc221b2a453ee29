"""Host-side mirror of the block-sort stage (libbsc's bsc_bwt_encode, reference src/libbsc/libbsc/libbsc/libbsc.cpp:158)
on top of the C ABI in include/spring_bwt.h.  All compute is in the HIP library; no CPU fallback."""
import ctypes as C

import numpy as np

from . import _lib
from ._stage import Stage, chk
from .qualid import KIND, QualIdStage
from .streams import STREAM_ID, StreamsStage

DEFAULT_BLOCK_BYTES = 25 * 1024 * 1024   # BSC's paramBlockSize (bsc.cpp:80)


def workspace_need(nbytes, segments=1):
    """What a sub-batch of nbytes bytes in `segments` segments takes of the workspace budget."""
    return int(_lib.lib().spring_bwt_workspace_need(nbytes, segments))


class BwtStage(Stage):
    """transform(): the Burrows-Wheeler transform, primary index and libbsc's secondary indexes of every segment of a
    batch, on the device.  The batch is host bytes with offsets, or the (stream, block) slices of a StreamsStage or the
    quality / id blocks of a QualIdStage, read in place in HBM.  download() / segments() fetch the result."""

    _prefix, _Info = "spring_bwt", _lib.BwtInfo

    def set_block_bytes(self, block_bytes):
        """The cut inside a stream slice for the calls that follow (default: 25 MiB, BSC's block size)."""
        chk(self._L.spring_bwt_set_block_bytes(self._h, block_bytes))

    def set_workspace_bytes(self, workspace_bytes):
        """The device workspace a sub-batch may use (0: from the free HBM)."""
        chk(self._L.spring_bwt_set_workspace_bytes(self._h, workspace_bytes))

    def set_run_keys(self, on, cap_bits=0):
        """Run-aware first keys for the calls that follow (default: off): same results, fewer rounds on content with
        few symbols and long runs.  cap_bits: 0 (the layout's own width) or 2 .. that width."""
        chk(self._L.spring_bwt_set_run_keys(self._h, int(bool(on)), cap_bits))

    def transform(self, src, seg_off=None, streams=None, kind="quality", block_bytes=0):
        """src: a StreamsStage holding a run; streams: the streams to take (ids, file names or short names; None: all
        nine).  Or a QualIdStage holding a result; kind: "quality" or "id"; block_bytes: the cut inside a block (0: the
        64 MiB SPRING passes).  Or bytes / a uint8 array; seg_off: num_segments + 1 offsets from 0 to len(src) that do
        not decrease (None: one segment).  -> info."""
        self.info = None
        if isinstance(src, QualIdStage):
            if seg_off is not None or streams is not None:
                raise ValueError("seg_off and streams are not for a QualIdStage: it is cut by its blocks and block_bytes")
            return self._run("from_qualid", src._h, KIND.get(kind, kind), block_bytes)
        if isinstance(src, StreamsStage):
            if seg_off is not None:
                raise ValueError("seg_off is for host buffers; a StreamsStage is cut by its blocks and block_bytes")
            ids = range(_lib.STREAMS_NUM) if streams is None else [s if isinstance(s, int) else STREAM_ID[s] for s in streams]
            mask = 0
            for s in ids:
                mask |= 1 << s
            return self._run("from_streams", src._h, mask)
        if streams is not None:
            raise ValueError("streams is for a StreamsStage")
        a = src if isinstance(src, np.ndarray) else np.frombuffer(src, np.uint8)
        a = np.ascontiguousarray(a, np.uint8)
        off = None if seg_off is None else np.ascontiguousarray(seg_off, dtype=np.uint64)
        if off is not None and len(off) < 1:
            raise ValueError("seg_off needs at least one offset")
        return self._run("from_host", a.ctypes.data if len(a) else None, len(a), None if off is None else off.ctypes.data,
                         0 if off is None else len(off) - 1)

    def download(self):
        """-> dict: bwt (all segments back to back: bytes), seg_off (num_segments + 1 uint64), primary and num_indexes
        (int32 per segment), indexes (num_segments x 256 int32; the first num_indexes of a row are set)."""
        if self.info is None:   # nothing transformed (or the last call failed): the library says so
            chk(self._L.spring_bwt_download(self._h, None, None, None, None, None))
        n, S = self.info["bytes"], self.info["num_segments"]
        buf = np.zeros(max(n, 1), np.uint8)
        off = np.zeros(S + 1, np.uint64)
        primary = np.zeros(max(S, 1), np.int32)
        num = np.zeros(max(S, 1), np.int32)
        idx = np.zeros((max(S, 1), _lib.BWT_MAX_INDEXES), np.int32)
        chk(self._L.spring_bwt_download(self._h, buf.ctypes.data, off.ctypes.data, primary.ctypes.data, num.ctypes.data,
                                        idx.ctypes.data))
        return dict(bwt=buf[:n].tobytes(), seg_off=off, primary=primary[:S], num_indexes=num[:S], indexes=idx[:S])

    def segments(self):
        """-> (stream id (-1: host input, -2 / -3: quality / id blocks), block, cut) of every segment: three arrays."""
        if self.info is None:
            chk(self._L.spring_bwt_segments(self._h, None, None, None))
        S = self.info["num_segments"]
        st, bl, cu = np.zeros(max(S, 1), np.int32), np.zeros(max(S, 1), np.uint32), np.zeros(max(S, 1), np.uint32)
        chk(self._L.spring_bwt_segments(self._h, st.ctypes.data, bl.ctypes.data, cu.ctypes.data))
        return st[:S], bl[:S], cu[:S]

    def round_entries(self):
        """-> the entries every sort round of the last call sorted (round 0: every position), summed over the
        sub-batches: uint64 array of info["rounds"] entries."""
        if self.info is None:
            chk(self._L.spring_bwt_round_entries(self._h, None, 0))
        e = np.zeros(max(self.info["rounds"], 1), np.uint64)
        chk(self._L.spring_bwt_round_entries(self._h, e.ctypes.data, len(e)))
        return e[:self.info["rounds"]]

    def encode_inplace(self, T):
        """bsc_bwt_encode's contract on a writable uint8 array (None or empty: n = 0): T is transformed in place.
        -> (primary index, the secondary indexes: int32 array)."""
        n = 0 if T is None else len(T)
        if n and not (isinstance(T, np.ndarray) and T.dtype == np.uint8 and T.flags.c_contiguous and T.flags.writeable):
            raise ValueError("T must be a writable contiguous uint8 array")
        num = C.c_uint8(0)
        idx = np.zeros(_lib.BWT_MAX_INDEXES, np.int32)
        self.info = None
        rc = self._L.spring_bwt_encode_inplace(self._h, T.ctypes.data if n else None, n, C.byref(num), idx.ctypes.data)
        if rc < 0:
            chk(rc)
        self.info = self.get_info()
        return rc, idx[:num.value].copy()
