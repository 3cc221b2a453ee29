"""Host-side mirror of the FASTQ assembler (the tail of reference src/decompress.cpp decompress_short with
write_fastq_block and modify_id of src/util.cpp) on top of the C ABI in include/spring_fastq_out.h.  All compute is in
the HIP library; no CPU fallback."""
import ctypes as C

import numpy as np

from . import _lib
from ._stage import Stage, chk
from .decode import DecodeStage
from .qualid import QualIdStage

ID_STORED, ID_NUMBERED, ID_FROM_MATE_1 = 0, 1, 2
TO_END = (1 << 64) - 1


def _u8(b):
    """bytes-like or array -> (uint8 array that shares its memory where it can, pointer or None)."""
    a = b if isinstance(b, np.ndarray) else np.frombuffer(b, np.uint8)
    a = np.ascontiguousarray(a, np.uint8)
    return a, (a.ctypes.data if len(a) else None)


class FastqOutStage(Stage):
    """assemble(): the text `id\\nread\\n+\\nquality\\n` per unit of one mate over a window of blocks, in HBM;
    download() / write() fetch it."""

    _prefix, _Info = "spring_fastq_out", _lib.FastqOutInfo

    def assemble(self, reads, num_reads, quality=None, ids=None, paired_end=False, num_reads_per_block=256000,
                 first_block=0, num_blocks=None, mate=0, preserve_id=True, paired_id_code=None, unit_range=None):
        """reads: a DecodeStage after a decode of this window, (bases, read_off) as DecodeStage.download gives them,
        or None.  quality: None (two-line records), a QualIdStage holding the file's quality blocks, the window's
        quality bytes, or (bytes, block_off).  ids: a QualIdStage holding the file's id blocks, the window's id lines,
        or (bytes, block_off); with preserve_id=False none, the ids are numbered.  paired_id_code 1..3: ids are file
        1's, the text is file 2's (mate must be 1).  unit_range: (start, end) within the window."""
        U = num_reads // 2 if paired_end else num_reads
        if num_blocks is None:
            B = max(num_reads_per_block, 1)
            num_blocks = max((U + B - 1) // B - first_block, 0)
        P = _lib.FastqOutParams()
        P.first_block, P.num_blocks, P.num_reads, P.num_reads_per_block = first_block, num_blocks, num_reads, num_reads_per_block
        P.paired_end, P.mate, P.preserve_quality = int(paired_end), mate, int(quality is not None)
        P.id_mode = ID_FROM_MATE_1 if paired_id_code is not None else ID_STORED if preserve_id else ID_NUMBERED
        P.paired_id_code = paired_id_code or 0
        P.range_start, P.range_end = (0, TO_END) if unit_range is None else unit_range
        S = _lib.FastqOutSources()
        keep = []
        if isinstance(reads, DecodeStage):
            S.decode = reads._h
        elif reads is not None:
            a, pa = _u8(reads[0])
            off = np.ascontiguousarray(reads[1], dtype=np.uint64)
            keep += [a, off]
            S.bases, S.read_off = pa, off.ctypes.data
        for name, src in (("quality", quality), ("id", ids)):
            if src is None:
                continue
            if isinstance(src, QualIdStage):
                setattr(S, name + "_ctx", src._h)
                continue
            data, tab = src if isinstance(src, tuple) else (src, None)
            a, pa = _u8(data)
            keep.append(a)
            setattr(S, "quality" if name == "quality" else "ids", pa)
            setattr(S, name + "_bytes", len(a))
            if tab is not None:
                t = np.ascontiguousarray(tab, dtype=np.uint64)
                keep.append(t)
                setattr(S, name + "_block_off", t.ctypes.data)
            elif not len(a):   # an empty source is still a source: give it an (empty) table to be seen
                t = np.zeros(num_blocks + 1, np.uint64)
                keep.append(t)
                setattr(S, name + "_block_off", t.ctypes.data)
        return self._run("assemble", C.byref(P), C.byref(S))

    def download(self, text=True, rec_off=True):
        """-> (the text: bytes, record offsets: num_units + 1 uint64); a part not asked for is None."""
        if self.info is None:   # nothing assembled (or the last call failed): the library says so
            chk(self._L.spring_fastq_out_download(self._h, None, None))
        n = self.info["bytes"]
        buf = np.zeros(max(n, 1), np.uint8) if text else None
        off = np.zeros(self.info["num_units"] + 1, np.uint64) if rec_off else None
        chk(self._L.spring_fastq_out_download(self._h, buf.ctypes.data if text else None,
                                              off.ctypes.data if rec_off else None))
        return (buf[:n].tobytes() if text else None), off

    def download_array(self):
        """-> the text as a uint8 array (no second copy on the host)."""
        if self.info is None:
            chk(self._L.spring_fastq_out_download(self._h, None, None))
        n = self.info["bytes"]
        buf = np.zeros(max(n, 1), np.uint8)
        chk(self._L.spring_fastq_out_download(self._h, buf.ctypes.data, None))
        return buf[:n]

    def write(self, path, append=False):
        """The text to a plain file (gzip output: GzipStage.compress(this stage)); -> info with ms_file."""
        info = _lib.FastqOutInfo()
        chk(self._L.spring_fastq_out_write(self._h, str(path).encode(), int(append), C.byref(info)))
        self.info = info.asdict()
        return self.info
