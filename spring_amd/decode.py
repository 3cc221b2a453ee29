"""Host-side mirror of the decoder of the per-block read streams (the read part of reference src/decompress.cpp
decompress_short) on top of the C ABI in include/spring_decode.h.  All compute is in the HIP library; no CPU
fallback."""
import ctypes as C

import numpy as np

from . import _lib
from ._stage import Stage, chk
from .streams import STREAM_FILES


class DecodeStage(Stage):
    """seq_from_*() loads the consensus once; from_*() decodes a window of blocks into the reads of its units in slot
    order; download(mate) / reads(mate) fetch read 1 (mate 0) or read 2 (mate 1, paired-end)."""

    _prefix, _Info = "spring_decode", _lib.DecodeInfo

    # ---- the consensus
    def seq_from_encoder(self, enc):
        """enc: an EncoderStage after encode(); its consensus is copied on the device."""
        self.info = None
        chk(self._L.spring_decode_seq_from_encoder(self._h, enc._h))

    def seq_from_host(self, seq_len_tid, packed, tails):
        """The images EncoderStage.seq_packed() gives: seq_len_tid, packed bytes (tid-major), a tail string per tid."""
        self.info = None
        sl = np.ascontiguousarray(seq_len_tid, dtype=np.uint64)
        T = len(sl)
        tail = np.zeros(4 * max(T, 1), np.uint8)
        for t, s in enumerate(tails):
            b = s.encode() if isinstance(s, str) else bytes(s)
            tail[4 * t:4 * t + len(b)] = np.frombuffer(b, np.uint8)
        buf = np.frombuffer(bytes(packed), np.uint8)
        chk(self._L.spring_decode_seq_from_host(self._h, T, sl.ctypes.data if T else None,
                                                buf.ctypes.data if len(buf) else None, tail.ctypes.data))

    def seq_from_files(self, temp_dir: str, num_thr_e: int):
        """temp_dir/read_seq.bin.<tid> (+ .tail) for tid < num_thr_e; removed on success."""
        self.info = None
        chk(self._L.spring_decode_seq_from_files(self._h, temp_dir.encode(), num_thr_e))

    # ---- the blocks
    def from_streams(self, ss):
        """Every block of the last run of a StreamsStage, with that run's parameters."""
        return self._run("from_streams", ss._h)

    def from_host(self, streams, num_reads, paired_end=False, preserve_order=False, num_reads_per_block=256000,
                  first_block=0, num_blocks=None):
        """streams: {stream id or file name: (bytes of the window's blocks back to back, num_blocks + 1 offsets from
        0)}, as StreamsStage.download gives (sliced to the window).  Streams 7 and 8 only for paired-end data."""
        ns = 9 if paired_end else 7
        keep, ptrs, offs = [], (C.c_void_p * 9)(), (C.c_void_p * 9)()
        for k, v in streams.items():
            sid = k if isinstance(k, int) else STREAM_FILES.index(k)
            if sid >= ns:
                continue
            data, off = v
            d = np.frombuffer(bytes(data), np.uint8)
            o = np.ascontiguousarray(off, dtype=np.uint64)
            keep += [d, o]
            ptrs[sid] = d.ctypes.data if len(d) else None
            offs[sid] = o.ctypes.data
            if num_blocks is None:
                num_blocks = len(o) - 1
        return self._run("from_host", ptrs, offs, first_block, num_blocks or 0, num_reads, int(paired_end),
                         int(preserve_order), num_reads_per_block)

    def from_files(self, temp_dir: str, first_block, num_blocks, num_reads, paired_end=False, preserve_order=False,
                   num_reads_per_block=256000):
        """temp_dir/<stream>.<b> for the window's blocks; removed on success."""
        return self._run("from_files", temp_dir.encode(), first_block, num_blocks, num_reads, int(paired_end),
                         int(preserve_order), num_reads_per_block)

    def download(self, mate=0):
        """-> (bases of the mate's reads back to back, num_units + 1 uint64 offsets)."""
        if self.info is None:   # nothing decoded (or the last call failed): the library says so
            chk(self._L.spring_decode_download(self._h, mate, None, None))
        n = self.info["bases"][mate]
        buf = np.zeros(max(n, 1), np.uint8)
        off = np.zeros(self.info["num_units"] + 1, np.uint64)
        chk(self._L.spring_decode_download(self._h, mate, buf.ctypes.data, off.ctypes.data))
        return buf[:n].tobytes(), off

    def reads(self, mate=0):
        """-> list of the mate's reads (str) in slot order."""
        data, off = self.download(mate)
        s = data.decode()
        return [s[int(off[i]):int(off[i + 1])] for i in range(len(off) - 1)]
