"""Host-side mirror of the gzip stage (the gzip_flag branch of write_fastq_block, reference src/util.cpp:70-110) on top
of the C ABI in include/spring_gzip.h.  All compute is in the HIP library; no CPU fallback."""
import ctypes as C

import numpy as np

from . import _lib
from ._stage import Stage, chk
from .fastq_out import FastqOutStage

STORED, DEFLATE = 0, 1


class GzipStage(Stage):
    """compress(): a FastqOutStage's text (read in place in HBM) or host bytes -> gzip members on the device;
    download() / write() fetch them."""

    _prefix, _Info = "spring_gzip", _lib.GzipInfo

    def set_chunk_bytes(self, chunk_bytes):
        """The cut inside a member for the calls that follow (for measurements; the default is the measured choice)."""
        chk(self._L.spring_gzip_set_chunk_bytes(self._h, chunk_bytes))

    def set_token_bytes(self, nbytes):
        """Token scratch of one batch of chunks for the calls that follow (0: the default of 1 GiB).  For tests and
        measurements: the output does not depend on it."""
        chk(self._L.spring_gzip_set_token_bytes(self._h, nbytes))

    def compress(self, src, member_records=0, member_off=None, mode=DEFLATE):
        """src: a FastqOutStage holding a text; members are cut every member_records records (0: one member).  Or
        bytes / a uint8 array; member_off: num_members + 1 offsets from 0 to len(src), strictly increasing (None: one
        member).  mode 0: stored blocks only, 1: the compressor.  -> info."""
        self.info = None
        if isinstance(src, FastqOutStage):
            if member_off is not None:
                raise ValueError("member_off is for host buffers; a FastqOutStage is cut by member_records")
            return self._run("from_fastq_out", src._h, member_records, mode)
        if member_records:
            raise ValueError("member_records is for a FastqOutStage; a host buffer is cut by member_off")
        a = src if isinstance(src, np.ndarray) else np.frombuffer(src, np.uint8)
        a = np.ascontiguousarray(a, np.uint8)
        off = None if member_off is None else np.ascontiguousarray(member_off, dtype=np.uint64)
        if off is not None and len(off) < 1:
            raise ValueError("member_off needs at least one offset")
        return self._run("from_host", a.ctypes.data if len(a) else None, len(a), None if off is None else off.ctypes.data,
                         0 if off is None else len(off) - 1, mode)

    def download(self):
        """-> (the members back to back: bytes, member offsets: num_members + 1 uint64)."""
        if self.info is None:   # nothing compressed (or the last call failed): the library says so
            chk(self._L.spring_gzip_download(self._h, None, None))
        n = self.info["bytes_out"]
        buf = np.zeros(max(n, 1), np.uint8)
        off = np.zeros(self.info["num_members"] + 1, np.uint64)
        chk(self._L.spring_gzip_download(self._h, buf.ctypes.data, off.ctypes.data))
        return buf[:n].tobytes(), off

    def write(self, path, append=False):
        """The members to a file; -> info with ms_file."""
        info = _lib.GzipInfo()
        chk(self._L.spring_gzip_write(self._h, str(path).encode(), int(append), C.byref(info)))
        self.info = info.asdict()
        return self.info
