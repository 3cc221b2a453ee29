"""Host-side mirror of the per-block read streams (reference src/reorder_compress_streams.cpp:31-441
reorder_compress_streams) on top of the C ABI in include/spring_streams.h.  All compute is in the HIP library;
no CPU fallback."""
import ctypes as C
import os

import numpy as np

from . import _lib
from ._stage import ReorderError, Stage, chk

# stream ids of include/spring_streams.h -> the file names of reorder_compress_streams.cpp:34-74
STREAM_FILES = ("read_flag.txt", "read_pos.bin", "read_noise.txt", "read_noisepos.bin", "read_rev.txt",
                "read_unaligned.txt", "read_lengths.bin", "read_pos_pair.bin", "read_rev_pair.txt")
STREAM_ID = {f: i for i, f in enumerate(STREAM_FILES)}
STREAM_ID.update({f.split(".")[0][len("read_"):]: i for i, f in enumerate(STREAM_FILES)})  # "flag", "pos", ...


def _ptr(a):
    return a.ctypes.data if a is not None and len(a) else None


def stream_names(paired_end: bool):
    """The streams reorder_compress_streams writes per block, in id order."""
    return STREAM_FILES if paired_end else STREAM_FILES[:7]


class StreamsStage(Stage):
    """from_encoder() / from_host(): the encoder's flat streams scattered into the final read order and cut into
    blocks of num_reads_per_block reads (pairs), on the device.  blocks(stream) fetches one stream's blocks."""

    _prefix, _Info = "spring_streams", _lib.StreamsInfo

    def from_encoder(self, enc, num_reads, paired_end=False, preserve_order=False, num_reads_per_block=256000,
                     apply_pe_encode=None):
        """enc: an EncoderStage after encode().  apply_pe_encode (default: paired-end without preserve_order) runs
        pe_encode on a private device copy of the encoder's order; the encoder's own order is left as it was."""
        if apply_pe_encode is None:
            apply_pe_encode = bool(paired_end and not preserve_order)
        return self._run("from_encoder", enc._h, num_reads, int(paired_end), int(preserve_order), num_reads_per_block,
                         int(apply_pe_encode))

    def from_host(self, pos, rc, noise, noisepos, order, rlen, unaligned, num_reads, paired_end=False,
                  preserve_order=False, num_reads_per_block=256000):
        """The images of read_pos.bin, read_rev.txt, read_noise.txt, read_noisepos.bin, read_order.bin (may be None
        unless paired_end or preserve_order), read_lengths.bin and read_unaligned.txt (arrays or bytes)."""
        pos = np.ascontiguousarray(pos, dtype=np.uint64)
        rc = np.frombuffer(bytes(rc), np.uint8) if isinstance(rc, (bytes, bytearray)) else np.ascontiguousarray(rc, np.uint8)
        noise = np.frombuffer(bytes(noise), np.uint8)
        noisepos = np.ascontiguousarray(noisepos, dtype=np.uint16)
        order = None if order is None else np.ascontiguousarray(order, dtype=np.uint32)
        rlen = np.ascontiguousarray(rlen, dtype=np.uint16)
        un = np.frombuffer(bytes(unaligned), np.uint8)
        if order is not None and len(order) != len(rlen):
            raise ReorderError("order and rlen differ in length")
        return self._run("from_host", _ptr(pos), _ptr(rc), len(rc), _ptr(noise), len(noise), _ptr(noisepos),
                         len(noisepos), _ptr(order), _ptr(rlen), len(rlen), _ptr(un), len(un), num_reads,
                         int(paired_end), int(preserve_order), num_reads_per_block)

    def download(self, stream):
        """-> (bytes of all blocks back to back, block offsets: num_blocks + 1 uint64)."""
        sid = stream if isinstance(stream, int) else STREAM_ID[stream]
        if self.info is None:   # nothing computed (or the last call failed): the library says so
            chk(self._L.spring_streams_download(self._h, sid, None, None))
        n = self.info["bytes"][sid]
        buf = np.zeros(max(n, 1), np.uint8)
        off = np.zeros(self.info["num_blocks"] + 1, np.uint64)
        chk(self._L.spring_streams_download(self._h, sid, buf.ctypes.data, off.ctypes.data))
        return buf[:n].tobytes(), off

    def blocks(self, stream):
        """-> list of the per-block byte images of `stream` (a stream id, file name or short name like "pos")."""
        data, off = self.download(stream)
        return [data[int(off[b]):int(off[b + 1])] for b in range(len(off) - 1)]


def call_reorder_compress_streams(temp_dir: str, cp, preserve_order: bool, num_reads_per_block: int = 256000,
                                  num_reads: int = None, device: int = -1):
    """spring::reorder_compress_streams(temp_dir, cp) (reference reorder_compress_streams.cpp:31-441) MINUS its BSC
    calls: consumes the encoder's files in temp_dir (read_order.bin already through pe_encode for paired-end data
    without preserve_order) and leaves <stream>.<b> for every stream and block; the caller runs
    BSC_compress(f, f + ".bsc") and removes f.  cp is a reorder.CompressionParams;
    num_reads = cp.num_reads of the reference (clean + N reads), by default cp.num_reads if it has one, else the
    record count of read_lengths.bin.  -> info dict."""
    if num_reads is None:
        num_reads = getattr(cp, "num_reads", None)
    if num_reads is None:
        num_reads = os.path.getsize(os.path.join(temp_dir, "read_lengths.bin")) // 2
    info = _lib.StreamsInfo()
    chk(_lib.lib().spring_streams_run(temp_dir.encode(), num_reads, int(cp.paired_end), int(preserve_order),
                                      num_reads_per_block, device, C.byref(info)))
    return info.asdict()
