"""Host-side mirror of the QLFC decoder stage (libbsc's bsc_coder_decompress with LIBBSC_CODER_QLFC_STATIC in fast mode,
reference src/libbsc/libbsc/coder/coder.cpp:171-217) on top of the C ABI in include/spring_unqlfc.h.  All compute is in
the HIP library; no CPU fallback."""
import ctypes as C

import numpy as np

from . import _lib
from ._stage import Stage, chk
from .qlfc import QlfcStage

PASSES = ("plan", "decode", "raw")   # info["ms_pass"]


class UnqlfcInfo(_lib.Info):
    """spring_unqlfc_info."""
    _fields_ = ([(k, C.c_uint64) for k in ("num_segments", "bytes_in", "bytes_out", "chunks", "chunks_raw", "runs", "events",
                                           "skipped", "sub_batches", "workspace_bytes")]
                + [("ms_device", C.c_double), ("ms_pass", C.c_double * _lib.UNQLFC_PASSES)])


def workspace_need(bytes_out, chunks=1):
    """What a sub-batch that decodes bytes_out bytes in `chunks` coded chunks takes of the workspace budget."""
    return int(_lib.lib().spring_unqlfc_workspace_need(bytes_out, chunks))


class UnqlfcStage(Stage):
    """decode(): every coded segment of a batch decoded on the device as bsc_coder_decompress decodes it.  The batch is
    host bytes with offsets and output sizes, or the coded segments of a QlfcStage, read in place in HBM.  download()
    fetches the result; UnbwtStage.invert() takes it where it lies.  The two state tables of the coder come from the
    caller: set_state_tables() first."""

    _prefix, _Info = "spring_unqlfc", UnqlfcInfo

    def set_state_tables(self, rank_table, run_table):
        """libbsc's model_rank_state_table (32768 bytes) and model_run_state_table (8192 bytes)."""
        rank = np.ascontiguousarray(np.frombuffer(bytes(rank_table), np.uint8))
        run = np.ascontiguousarray(np.frombuffer(bytes(run_table), np.uint8))
        if len(rank) != _lib.QLFC_RANK_TABLE or len(run) != _lib.QLFC_RUN_TABLE:
            raise ValueError("the state tables are %d and %d bytes" % (_lib.QLFC_RANK_TABLE, _lib.QLFC_RUN_TABLE))
        chk(self._L.spring_unqlfc_set_state_tables(self._h, rank.ctypes.data, run.ctypes.data))

    def set_workspace_bytes(self, workspace_bytes):
        """The device workspace a sub-batch may use (0: from the free HBM)."""
        chk(self._L.spring_unqlfc_set_workspace_bytes(self._h, workspace_bytes))

    def decode(self, src, coded_off=None, out_size=None):
        """src: a QlfcStage holding a result (its segments, in its order; the output sizes are its input sizes).  Or
        bytes / a uint8 array with out_size: the decoded size of every segment (an int for one segment) and coded_off:
        num_segments + 1 offsets from 0 to len(src) that do not decrease (None: one segment).  -> info."""
        self.info = None
        if isinstance(src, QlfcStage):
            if coded_off is not None or out_size is not None:
                raise ValueError("coded_off and out_size are for host buffers; a QlfcStage brings its own")
            return self._run("from_qlfc", src._h)
        a = src if isinstance(src, np.ndarray) else np.frombuffer(src, np.uint8)
        a = np.ascontiguousarray(a, np.uint8)
        off = np.ascontiguousarray([0, len(a)] if coded_off is None else coded_off, dtype=np.uint64)
        if len(off) < 1:
            raise ValueError("coded_off needs at least one offset")
        if out_size is None:
            raise ValueError("a host buffer needs its output sizes")
        size = np.ascontiguousarray(np.atleast_1d(out_size), dtype=np.uint64)
        if len(size) != len(off) - 1:
            raise ValueError("%d output sizes for %d segments" % (len(size), len(off) - 1))
        return self._run("from_host", a.ctypes.data if len(a) else None, len(a), off.ctypes.data,
                         size.ctypes.data if len(size) else None, len(size))

    def download(self):
        """-> dict: bytes (the decoded segments back to back), seg_off (num_segments + 1 uint64)."""
        if self.info is None:   # nothing decoded (or the last call failed): the library says so
            chk(self._L.spring_unqlfc_download(self._h, None, None))
        n, S = self.info["bytes_out"], self.info["num_segments"]
        buf = np.zeros(max(n, 1), np.uint8)
        off = np.zeros(S + 1, np.uint64)
        chk(self._L.spring_unqlfc_download(self._h, buf.ctypes.data, off.ctypes.data))
        return dict(bytes=buf[:n].tobytes(), seg_off=off)

    def segments(self):
        """-> the decoded segments, one bytes object each."""
        res = self.download()
        off = res["seg_off"]
        return [res["bytes"][int(off[s]):int(off[s + 1])] for s in range(len(off) - 1)]

    def decompress(self, coded, out_size):
        """bsc_coder_decompress's contract on a host buffer, with the decoded size -> the decoded bytes."""
        a = np.ascontiguousarray(np.frombuffer(bytes(coded), np.uint8))
        out = np.zeros(max(int(out_size), 1), np.uint8)
        self.info = None
        rc = self._L.spring_unqlfc_decompress(self._h, a.ctypes.data if len(a) else None, len(a), out.ctypes.data, int(out_size))
        if rc < 0:
            chk(rc)
        self.info = self.get_info()
        return out[:rc].tobytes()
