"""Host-side mirror of the BSC framing stage (libbsc's bsc_compress blocks and the files BSC_compress and
BSC_str_array_compress write, reference src/libbsc/libbsc/libbsc/libbsc.cpp:77-305, libbsc/bsc.cpp:149-379,
libbsc/bsc_str_array.cpp:183-463) on top of the C ABI in include/spring_bsc.h.  All compute is in the HIP library; no CPU
fallback."""
import ctypes as C

import numpy as np

from . import _lib
from ._stage import Stage, chk
from .bwt import BwtStage
from .qlfc import QlfcStage
from .qualid import KIND, QualIdStage
from .streams import STREAM_ID, StreamsStage

FRAMING = {"blocks": _lib.BSC_BLOCKS, "file": _lib.BSC_FILE, "str_array": _lib.BSC_STR_ARRAY}
KINDS = ("coded", "stored_small", "stored_coder", "stored_no_gain")   # block_kind 0 .. 3


class BscInfo(_lib.Info):
    """spring_bsc_info."""
    _fields_ = ([(k, C.c_uint64) for k in ("num_files", "num_blocks", "bytes_in", "bytes_out", "coded", "stored_small",
                                           "stored_coder", "stored_no_gain")]
                + [("ms_device", C.c_double), ("ms_pass", C.c_double * _lib.BSC_PASSES)])


class BscStage(Stage):
    """frame(): runs the block sort and the QLFC coder on the two stages it is given and frames their results on the
    device into the bytes bsc_compress, BSC_compress (stream slices) or BSC_str_array_compress (quality / id blocks)
    write.  download() / files() fetch the result.  The BwtStage carries the cut (set_block_bytes), the run-key and
    workspace settings, the QlfcStage the state tables; both keep their own results."""

    _prefix, _Info = "spring_bsc", BscInfo

    def frame(self, bwt, qlfc, src, seg_off=None, framing="blocks", file_first=None, streams=None, kind="quality",
              block_bytes=0):
        """src: a StreamsStage holding a run (streams: ids, file names or short names; None: all nine) -> one BSC file
        per (stream, block) slice.  Or a QualIdStage holding a result (kind: "quality" or "id"; block_bytes: the cut
        inside a block, 0: 64 MiB) -> one string-array file per block.  Or bytes / a uint8 array with seg_off
        (num_segments + 1 offsets, None: one segment), framing "blocks", "file" or "str_array", and file_first
        (num_files + 1 segment numbers from 0 to num_segments; None: one file per segment).  -> info."""
        if not isinstance(bwt, BwtStage) or not isinstance(qlfc, QlfcStage):
            raise ValueError("frame() takes a BwtStage and a QlfcStage")
        self.info = None
        bwt.info = qlfc.info = None
        try:
            if isinstance(src, QualIdStage):
                if seg_off is not None or streams is not None or file_first is not None:
                    raise ValueError("seg_off, file_first and streams are not for a QualIdStage")
                return self._run("from_qualid", bwt._h, qlfc._h, src._h, KIND.get(kind, kind), block_bytes)
            if isinstance(src, StreamsStage):
                if seg_off is not None or file_first is not None:
                    raise ValueError("seg_off and file_first are for host buffers")
                ids = range(_lib.STREAMS_NUM) if streams is None else [s if isinstance(s, int) else STREAM_ID[s] for s in streams]
                mask = 0
                for s in ids:
                    mask |= 1 << s
                return self._run("from_streams", bwt._h, qlfc._h, src._h, mask)
            if streams is not None:
                raise ValueError("streams is for a StreamsStage")
            a = src if isinstance(src, np.ndarray) else np.frombuffer(src, np.uint8)
            a = np.ascontiguousarray(a, np.uint8)
            off = None if seg_off is None else np.ascontiguousarray(seg_off, dtype=np.uint64)
            ff = None if file_first is None else np.ascontiguousarray(file_first, dtype=np.uint64)
            if (off is not None and len(off) < 1) or (ff is not None and len(ff) < 1):
                raise ValueError("seg_off and file_first need at least one entry")
            return self._run("from_host", bwt._h, qlfc._h, a.ctypes.data if len(a) else None, len(a),
                             None if off is None else off.ctypes.data, 0 if off is None else len(off) - 1,
                             FRAMING.get(framing, framing), None if ff is None else ff.ctypes.data,
                             0 if ff is None else len(ff) - 1)
        finally:
            for st in (bwt, qlfc):   # what the inner stages hold now, if they hold anything
                try:
                    st.info = st.get_info()
                except Exception:
                    st.info = None

    def download(self):
        """-> dict: bytes (the files back to back), file_off (num_files + 1 uint64), block_off (per block the offset of
        its header in bytes), block_kind (int32 per block: 0 coded, 1 stored: at most 28 bytes, 2 stored: the coder
        gave up, 3 stored: no gain)."""
        if self.info is None:   # nothing framed (or the last call failed): the library says so
            chk(self._L.spring_bsc_download(self._h, None, None, None, None))
        n, F, S = self.info["bytes_out"], self.info["num_files"], self.info["num_blocks"]
        buf = np.zeros(max(n, 1), np.uint8)
        foff = np.zeros(F + 1, np.uint64)
        boff = np.zeros(max(S, 1), np.uint64)
        kind = np.zeros(max(S, 1), np.int32)
        chk(self._L.spring_bsc_download(self._h, buf.ctypes.data, foff.ctypes.data, boff.ctypes.data, kind.ctypes.data))
        return dict(bytes=buf[:n].tobytes(), file_off=foff, block_off=boff[:S], block_kind=kind[:S])

    def files(self):
        """-> list, per file: (stream id as BwtStage.segments() reports it, block, first segment, the file's bytes)."""
        res = self.download()
        F = self.info["num_files"]
        st, bl, fs = np.zeros(max(F, 1), np.int32), np.zeros(max(F, 1), np.uint32), np.zeros(max(F, 1), np.uint64)
        chk(self._L.spring_bsc_files(self._h, st.ctypes.data, bl.ctypes.data, fs.ctypes.data))
        off = res["file_off"]
        return [(int(st[f]), int(bl[f]), int(fs[f]), res["bytes"][int(off[f]):int(off[f + 1])]) for f in range(F)]

    def adler32(self, src, seg_off=None):
        """bsc_adler32 of every segment of a host batch -> uint32 array (1 for an empty segment)."""
        a = src if isinstance(src, np.ndarray) else np.frombuffer(src, np.uint8)
        a = np.ascontiguousarray(a, np.uint8)
        off = np.ascontiguousarray([0, len(a)] if seg_off is None else seg_off, dtype=np.uint64)
        if len(off) < 1:
            raise ValueError("seg_off needs at least one offset")
        sums = np.zeros(max(len(off) - 1, 1), np.uint32)
        chk(self._L.spring_bsc_adler32(self._h, a.ctypes.data if len(a) else None, len(a), off.ctypes.data, len(off) - 1,
                                       sums.ctypes.data))
        return sums[:len(off) - 1]

    def compress(self, bwt, qlfc, buf):
        """bsc_compress's contract on a host buffer -> the block (stored where bsc_compress or BSC_compress stores)."""
        a = np.ascontiguousarray(np.frombuffer(bytes(buf), np.uint8))
        out = np.zeros(len(a) + _lib.BSC_HEADER_BYTES, np.uint8)
        self.info = None
        rc = self._L.spring_bsc_compress(self._h, bwt._h, qlfc._h, a.ctypes.data if len(a) else None, out.ctypes.data, len(a))
        if rc < 0:
            chk(rc)
        self.info = self.get_info()
        return out[:rc].tobytes()
