"""Host-side mirror of the inverse block-sort stage (libbsc's bsc_bwt_decode, reference
src/libbsc/libbsc/bwt/bwt.cpp:180) on top of the C ABI in include/spring_unbwt.h.  All compute is in the HIP library; no
CPU fallback."""
import ctypes as C

import numpy as np

from . import _lib
from ._stage import Stage, chk
from .bwt import BwtStage
from .unqlfc import UnqlfcStage

PASSES = ("keys", "sort", "scatter", "walk", "rank", "write")   # info["ms_pass"]


def workspace_need(nbytes, segments=1):
    """What a sub-batch of nbytes bytes in `segments` segments takes of the workspace budget."""
    return int(_lib.lib().spring_unbwt_workspace_need(nbytes, segments))


class UnbwtStage(Stage):
    """invert(): the text of every transformed segment of a batch, on the device.  The batch is host bytes with offsets
    and primary indexes, or the result of a BwtStage, read in place in HBM.  download() fetches the texts."""

    _prefix, _Info = "spring_unbwt", _lib.UnbwtInfo

    def set_workspace_bytes(self, workspace_bytes):
        """The device workspace a sub-batch may use (0: from the free HBM)."""
        chk(self._L.spring_unbwt_set_workspace_bytes(self._h, workspace_bytes))

    def set_head_spacing(self, head_spacing):
        """K: one regular sublist head in every K rows (a power of two in 16 .. 1024; 0: the default, 64)."""
        chk(self._L.spring_unbwt_set_head_spacing(self._h, head_spacing))

    def invert(self, src, seg_off=None, primary=None):
        """src: a BwtStage holding a result.  Or an UnqlfcStage holding a result, with primary: one primary index per
        segment.  Or bytes / a uint8 array with primary: one primary index per segment (an
        int for one segment) and seg_off: num_segments + 1 offsets from 0 to len(src) that do not decrease (None: one
        segment).  -> info."""
        self.info = None
        if isinstance(src, BwtStage):
            if seg_off is not None or primary is not None:
                raise ValueError("seg_off and primary are for host buffers; a BwtStage brings its own")
            return self._run("from_bwt", src._h)
        if isinstance(src, UnqlfcStage):   # the decoded segments where they lie; the primary indexes from the caller
            if seg_off is not None:
                raise ValueError("seg_off is for host buffers; an UnqlfcStage brings its own segments")
            if primary is None:
                raise ValueError("decoded segments need their primary indexes")
            prim = np.ascontiguousarray(np.atleast_1d(primary), dtype=np.int32)
            if src.info is None or len(prim) != src.info["num_segments"]:
                raise ValueError("one primary index per decoded segment")
            return self._run("from_unqlfc", src._h, prim.ctypes.data if len(prim) else None)
        a = src if isinstance(src, np.ndarray) else np.frombuffer(src, np.uint8)
        a = np.ascontiguousarray(a, np.uint8)
        off = None if seg_off is None else np.ascontiguousarray(seg_off, dtype=np.uint64)
        if off is not None and len(off) < 1:
            raise ValueError("seg_off needs at least one offset")
        S = 1 if off is None else len(off) - 1
        if primary is None:
            raise ValueError("a host buffer needs its primary indexes")
        prim = np.ascontiguousarray(np.atleast_1d(primary), dtype=np.int32)
        if len(prim) != S:
            raise ValueError("%d primary indexes for %d segments" % (len(prim), S))
        return self._run("from_host", a.ctypes.data if len(a) else None, len(a), None if off is None else off.ctypes.data,
                         prim.ctypes.data if S else None, S if off is not None else 0)

    def download(self):
        """-> dict: text (all segments back to back: bytes), seg_off (num_segments + 1 uint64)."""
        if self.info is None:   # nothing inverted (or the last call failed): the library says so
            chk(self._L.spring_unbwt_download(self._h, None, None))
        n, S = self.info["bytes"], self.info["num_segments"]
        buf = np.zeros(max(n, 1), np.uint8)
        off = np.zeros(S + 1, np.uint64)
        chk(self._L.spring_unbwt_download(self._h, buf.ctypes.data, off.ctypes.data))
        return dict(text=buf[:n].tobytes(), seg_off=off)

    def decode_inplace(self, T, index, indexes=None):
        """bsc_bwt_decode's contract on a writable uint8 array (None or empty: n = 0): T, a transform with primary index
        `index`, is replaced by its text.  indexes: the secondary indexes, accepted and not needed."""
        n = 0 if T is None else len(T)
        if n and not (isinstance(T, np.ndarray) and T.dtype == np.uint8 and T.flags.c_contiguous and T.flags.writeable):
            raise ValueError("T must be a writable contiguous uint8 array")
        idx = None if indexes is None else np.ascontiguousarray(indexes, dtype=np.int32)
        self.info = None
        chk(self._L.spring_unbwt_decode_inplace(self._h, T.ctypes.data if n else None, n, int(index),
                                                0 if idx is None else len(idx) & 0xff,
                                                None if idx is None or not len(idx) else idx.ctypes.data))
        self.info = self.get_info()
