"""Writes tests/golden/ref_idcodec_<case>.npz: the files the REFERENCE'S OWN compress_id_block writes for the id lists
of tests/idcodec_cases.py, so that the id codec tests can compare with reference-written bytes where oracle/_ref is not
built.  Reads only oracle/_ref/libref_qualid.so (`make -C oracle`): ref_q_write is the real
reorder_compress_quality_id, run single-end, ids only, with an identity read_order.bin; id_1.<b> is read raw
(idcodec_cases.ref_blocks).  Data only.  Run: python tests/golden/make_ref_idcodec_golden.py

ref_idcodec_<case>.npz   `ids` = the id lines, each with its '\n'; `B` = num_reads_per_block; `blocks` = id_1.0,
                         id_1.1, ... back to back; `block_off` = their offsets.
ref_idcodec_rescale.npz  `id` and `count` in place of `ids`: the block is `count` copies of `id`.
ref_idcodec_rescale256.npz  `counter` in place of `ids`: the block is the ids 1, 2, ..., `counter`.

Every recorded file but the two rescale ones is read back by the real decompress_id_block and compared with the ids before
it is stored."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import idcodec_cases as ic  # noqa: E402
from oracle import pyoracle as po  # noqa: E402

assert po.ref_qualid_lib(), "oracle/_ref is not built"
u8 = lambda b: np.frombuffer(bytes(b), np.uint8)  # noqa: E731


def store(name, blocks, **kw):
    off = np.concatenate([[0], np.cumsum([len(x) for x in blocks])]).astype(np.uint64)
    path = os.path.join(HERE, "ref_idcodec_%s.npz" % name)
    np.savez_compressed(path, blocks=u8(b"".join(blocks)), block_off=off, **kw)
    print("%s: %d blocks, %d bytes" % (os.path.basename(path), len(blocks), int(off[-1])))


if __name__ == "__main__":
    for name, (ids, B) in sorted(ic.FIXTURES.items()):
        store(name, ic.ref_blocks(ids, B), ids=u8(ic.lines_image(ids)), B=np.uint32(B))
    ids = [ic.RESCALE_ID] * ic.RESCALE_COUNT
    store("rescale", ic.ref_blocks(ids, ic.RESCALE_COUNT, readback=False), id=u8(ic.RESCALE_ID),
          count=np.uint32(ic.RESCALE_COUNT), B=np.uint32(ic.RESCALE_COUNT))
    ids = ic.counter_ids(ic.COUNTER_COUNT)
    store("rescale256", ic.ref_blocks(ids, ic.COUNTER_COUNT, readback=False), counter=np.uint32(ic.COUNTER_COUNT),
          B=np.uint32(ic.COUNTER_COUNT))
