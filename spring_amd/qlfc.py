"""Host-side mirror of the QLFC stage (libbsc's bsc_coder_compress with LIBBSC_CODER_QLFC_STATIC in fast mode,
reference src/libbsc/libbsc/coder/coder.cpp:110-160) on top of the C ABI in include/spring_qlfc.h.  All compute is in the
HIP library; no CPU fallback."""
import ctypes as C

import numpy as np

from . import _lib
from ._stage import Stage, chk
from .bwt import BwtStage

NOT_COMPRESSIBLE = -3   # LIBBSC_NOT_COMPRESSIBLE, what compress() returns where bsc_coder_compress does


class QlfcInfo(_lib.Info):
    """spring_qlfc_info."""
    _fields_ = ([(k, C.c_uint64) for k in ("num_segments", "bytes_in", "bytes_out", "chunks", "runs", "events",
                                           "not_compressible", "chunks_raw", "sub_batches", "workspace_bytes")]
                + [("ms_device", C.c_double), ("ms_pass", C.c_double * _lib.QLFC_PASSES)])


def workspace_need(nbytes, segments=1):
    """What a sub-batch of nbytes bytes in `segments` segments takes of the workspace budget before its events are
    counted; every event takes _lib.QLFC_EVENT_BYTES more."""
    return int(_lib.lib().spring_qlfc_workspace_need(nbytes, segments))


class QlfcStage(Stage):
    """code(): every segment of a batch coded on the device as bsc_coder_compress codes it.  The batch is host bytes
    with offsets, or the transformed segments of a BwtStage, read in place in HBM.  download() fetches the result.  The
    two state tables of the coder come from the caller: set_state_tables() first."""

    _prefix, _Info = "spring_qlfc", QlfcInfo

    def set_state_tables(self, rank_table, run_table):
        """libbsc's model_rank_state_table (32768 bytes) and model_run_state_table (8192 bytes)."""
        rank = np.ascontiguousarray(np.frombuffer(bytes(rank_table), np.uint8))
        run = np.ascontiguousarray(np.frombuffer(bytes(run_table), np.uint8))
        if len(rank) != _lib.QLFC_RANK_TABLE or len(run) != _lib.QLFC_RUN_TABLE:
            raise ValueError("the state tables are %d and %d bytes" % (_lib.QLFC_RANK_TABLE, _lib.QLFC_RUN_TABLE))
        chk(self._L.spring_qlfc_set_state_tables(self._h, rank.ctypes.data, run.ctypes.data))

    def set_workspace_bytes(self, workspace_bytes):
        """The device workspace a sub-batch may use (0: from the free HBM)."""
        chk(self._L.spring_qlfc_set_workspace_bytes(self._h, workspace_bytes))

    def code(self, src, seg_off=None):
        """src: a BwtStage holding a result (its segments, in its order), or bytes / a uint8 array; seg_off:
        num_segments + 1 offsets from 0 to len(src) that do not decrease (None: one segment).  -> info."""
        self.info = None
        if isinstance(src, BwtStage):
            if seg_off is not None:
                raise ValueError("seg_off is for host buffers; a BwtStage brings its own segments")
            return self._run("from_bwt", src._h)
        a = src if isinstance(src, np.ndarray) else np.frombuffer(src, np.uint8)
        a = np.ascontiguousarray(a, np.uint8)
        off = None if seg_off is None else np.ascontiguousarray(seg_off, dtype=np.uint64)
        if off is not None and len(off) < 1:
            raise ValueError("seg_off needs at least one offset")
        return self._run("from_host", a.ctypes.data if len(a) else None, len(a), None if off is None else off.ctypes.data,
                         0 if off is None else len(off) - 1)

    def download(self):
        """-> dict: coded (the coded segments back to back: bytes), coded_off (num_segments + 1 uint64), status (int32
        per segment: 0 coded, 1 not compressible -- no bytes)."""
        if self.info is None:   # nothing coded (or the last call failed): the library says so
            chk(self._L.spring_qlfc_download(self._h, None, None, None))
        n, S = self.info["bytes_out"], self.info["num_segments"]
        buf = np.zeros(max(n, 1), np.uint8)
        off = np.zeros(S + 1, np.uint64)
        status = np.zeros(max(S, 1), np.int32)
        chk(self._L.spring_qlfc_download(self._h, buf.ctypes.data, off.ctypes.data, status.ctypes.data))
        return dict(coded=buf[:n].tobytes(), coded_off=off, status=status[:S])

    def segments(self):
        """-> per segment (coded bytes, return value as bsc_coder_compress gives it: the size or NOT_COMPRESSIBLE)."""
        res = self.download()
        off = res["coded_off"]
        return [(res["coded"][int(off[s]):int(off[s + 1])], int(off[s + 1] - off[s]) if st == 0 else NOT_COMPRESSIBLE)
                for s, st in enumerate(res["status"])]

    def compress(self, buf):
        """bsc_coder_compress's contract on a host buffer -> (coded bytes, return value)."""
        a = np.ascontiguousarray(np.frombuffer(bytes(buf), np.uint8))
        out = np.zeros(max(len(a), 1), np.uint8)
        self.info = None
        rc = self._L.spring_qlfc_compress(self._h, a.ctypes.data if len(a) else None, out.ctypes.data, len(a))
        if rc == _lib.QLFC_NOT_COMPRESSIBLE:
            rc = NOT_COMPRESSIBLE
        elif rc < 0:
            chk(rc)
        self.info = self.get_info()
        return (out[:rc].tobytes() if rc > 0 else b""), rc
