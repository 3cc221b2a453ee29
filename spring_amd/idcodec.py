"""Host-side mirror of the id codec stage (compress_id_block, reference src/util.cpp:113-126 and src/id_compression/)
on top of the C ABI in include/spring_idcodec.h.  All compute is in the HIP library; no CPU fallback."""
import ctypes as C

import numpy as np

from . import _lib
from ._stage import Stage, chk
from .qualid import QualIdStage

KINDS = ("type", "alpha_len", "alpha_byte", "char", "delta", "zero_run", "integer")   # bits 8-10 of a symbol word
TOKEN_TYPES = ("ALPHA", "DIGIT", "CHAR", "MATCH", "ZEROS", "DELTA", "END")            # the values of kind "type"


def workspace_need(blocks, max_tokens):
    """What the model tables of `blocks` blocks take of the workspace at a largest token count of max_tokens."""
    return int(_lib.lib().spring_idcodec_workspace_need(blocks, max_tokens))


class IdCodecStage(Stage):
    """from_qualid() / from_lines(): the id blocks of a run compressed on the device into the bytes compress_id_block
    writes to id_N.<block>.  blocks() fetches them, symbols() the token symbols the coder ran on."""

    _prefix, _Info = "spring_idcodec", _lib.IdCodecInfo

    def set_workspace_bytes(self, workspace_bytes):
        """The device memory the model tables of a sub-batch may use (0: from the free HBM)."""
        chk(self._L.spring_idcodec_set_workspace_bytes(self._h, workspace_bytes))

    def from_qualid(self, qualid):
        """qualid: a QualIdStage holding an id result; it stays in HBM and is left as it was.  -> info."""
        if not isinstance(qualid, QualIdStage):
            raise TypeError("from_qualid takes a QualIdStage")
        return self._run("from_qualid", qualid._h)

    def from_lines(self, lines, num_reads_per_block=256000):
        """lines: a list of ids (bytes, without '\\n') in slot order, or their image with every id '\\n'-terminated.
        -> info."""
        if isinstance(lines, (list, tuple)):
            n, lines = len(lines), b"".join(bytes(x) + b"\n" for x in lines)
        else:
            lines = lines.tobytes() if isinstance(lines, np.ndarray) else bytes(lines)
            n = lines.count(b"\n")
        a = np.frombuffer(lines, np.uint8)
        return self._run("from_host", a.ctypes.data if len(a) else None, len(a), n, num_reads_per_block)

    def download(self):
        """-> (bytes of all blocks back to back, block offsets: uint64)."""
        if self.info is None:   # nothing compressed (or the last call failed): the library says so
            chk(self._L.spring_idcodec_download(self._h, None, None))
        n = self.info["bytes"]
        buf = np.zeros(max(n, 1), np.uint8)
        off = np.zeros(self.info["num_blocks"] + 1, np.uint64)
        chk(self._L.spring_idcodec_download(self._h, buf.ctypes.data, off.ctypes.data))
        return buf[:n].tobytes(), off

    def blocks(self):
        """-> per block the bytes of its id_N.<block> file."""
        data, off = self.download()
        return [data[int(off[b]):int(off[b + 1])] for b in range(len(off) - 1)]

    def symbols(self):
        """-> (symbol words: uint32, value | kind << 8 | context << 11; per-block offsets: uint64)."""
        if self.info is None:
            chk(self._L.spring_idcodec_symbols(self._h, None, None))
        n = self.info["num_symbols"]
        words = np.zeros(max(n, 1), np.uint32)
        off = np.zeros(self.info["num_blocks"] + 1, np.uint64)
        chk(self._L.spring_idcodec_symbols(self._h, words.ctypes.data, off.ctypes.data))
        return words[:n], off
