"""The id lists behind tests/golden/ref_idcodec_*.npz (tests/golden/make_ref_idcodec_golden.py records them through
the reference's own compress_id_block) and the loader the id codec tests share.  Each case is the smallest that reaches a
rule of the format."""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

# A prefix that is not a match, more tokens than the previous id, zero runs, delta 1 / 255, a negative difference, the
# 2^28 split, a previous token that is not a number; the last two ids add the delta of 256 the list lacked.
CORNER = [b"@AB", b"@AB.AB", b"@ABC", b"@AB", b"@", b"@x001", b"@x001", b"@x0001", b"@x01", b"@x10", b"@x11", b"@x266",
          b"@x267", b"@x9", b"@x4294967295", b"@x268435456123", b"@x268435455999", b"@x05", b"@x5", b"@x260", b"@x5",
          b"@a-b", b"@a+b", b"@a+b+c+d", b"@a", b"@12 34", b"@12 35 9", b"@13 290 9", b"@13 034 9", b"@13 34 9",
          b"@x4", b"@x260"]
# tokens beyond the previous id's count compare against its start
BEYOND = [b"@AB", b"@AB.AB", b"@AB.AB", b"@AB.AB.AB", b"@AB"]
EMPTY = [b"", b"@a 1", b"", b"", b"@a 2", b"@a 2", b""]
RESCALE_ID, RESCALE_COUNT = b"A", 104870   # one block: the type model of token 0 reaches n >= 2^20
COUNTER_COUNT = 105000   # one block of the ids 1, 2, 3, ...: a delta of 1 each, the 256-symbol delta model reaches n >= 2^20


def long_ids():
    """An id of 1 022 bytes with a 255-letter run, a 255-zero run and 410 digits; the same id twice; '@' + 254 letters;
    '@q'."""
    digits = "".join(str((7 * i + 3) % 10) for i in range(410))
    a = ("@" + "L" * 255 + ":" + "0" * 255 + ":" + digits + ":" + "z" * 98).encode()
    assert len(a) == 1022
    return [a, a, b"@" + b"Q" * 254, b"@q"]


def illumina_ids(n, seed=20240611):
    """Illumina-style ids: instrument, run, flowcell, lane, tile, x, y and a comment; tile / x / y advance as a sequencer's
    do, so that most tokens match or differ by a small delta."""
    rng = np.random.default_rng(seed)
    out, tile, x, y = [], 1101, 1000, 1000
    for i in range(n):
        x += int(rng.integers(0, 300))
        if x > 30000:
            x = 1000 + int(rng.integers(0, 200))
            y += int(rng.integers(1, 400))
        if y > 200000 or rng.random() < 0.002:
            y = 1000 + int(rng.integers(0, 500))
            tile += 1 if tile % 100 < 78 else 923
        out.append(("@A00123:45:HXXXXDSXX:%d:%d:%d:%d 1:N:0:%s" % (1 + tile // 2000 % 4, tile, x, y,
                                                                 "ACGT"[int(rng.integers(0, 4))] + "TTAGGC")).encode())
    return out


# name -> (ids, B); the reference needs num_reads >= 4
FIXTURES = {
    "corner_B1": (CORNER, 1), "corner_B7": (CORNER, 7), "corner_B64": (CORNER, 64),
    "beyond": (BEYOND, 5), "long": (long_ids(), 4), "empty": (EMPTY, 4),
    "illumina": (illumina_ids(3000), 1000),
}


def counter_ids(n):
    return [b"%d" % i for i in range(1, n + 1)]


def lines_image(ids):
    return b"".join(i + b"\n" for i in ids)


def ref_blocks(ids, B, num_thr=1, readback=True):
    """The raw id_1.<b> files of the real reorder_compress_quality_id (oracle/_ref/libref_qualid.so: it calls the real
    compress_id_block) for ids in slot order: single-end, ids only, an identity read_order.bin.  readback: every file
    goes through the real decompress_id_block and must give the ids back."""
    import tempfile
    from oracle import pyoracle as po
    n = len(ids)
    assert n >= 4, "the reference sizes an array from num_reads / 4 - 1"
    with tempfile.TemporaryDirectory() as d:
        with open(os.path.join(d, "id_1"), "wb") as f:
            f.write(lines_image(ids))
        with open(os.path.join(d, "read_order.bin"), "wb") as f:
            f.write(np.arange(n, dtype=np.uint32).tobytes())
        assert po.ref_qualid_lib().ref_q_write(d.encode(), n, 0, B, num_thr, 0, 1, 0) == 0
        out = []
        for b in range((n + B - 1) // B):
            path = os.path.join(d, "id_1.%d" % b)
            with open(path, "rb") as f:
                out.append(f.read())
            if readback:
                assert po.ref_read_ids(path, min(B, n - b * B)) == ids[b * B:(b + 1) * B], (b, "read back")
        return out


def load(name):
    """-> (ids, B, per-block bytes) of a recorded fixture; "rescale" and "rescale256" rebuild their ids from the stored parameters."""
    z = np.load(os.path.join(GOLDEN, "ref_idcodec_%s.npz" % name))
    if "count" in z.files:
        ids = [z["id"].tobytes()] * int(z["count"])
    elif "counter" in z.files:
        ids = counter_ids(int(z["counter"]))
    else:
        ids = z["ids"].tobytes().split(b"\n")[:-1]
    raw, off = z["blocks"].tobytes(), z["block_off"]
    return ids, int(z["B"]), [raw[int(off[b]):int(off[b + 1])] for b in range(len(off) - 1)]


ALL = sorted(FIXTURES) + ["rescale", "rescale256"]
