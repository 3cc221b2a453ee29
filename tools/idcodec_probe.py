"""The id codec stage on N Illumina-style ids against the real compress_id_block on 16 CPU
threads, same blocks, same box: ms_tokens / ms_coder of every repetition after a warm-up run, the wall time of the real
reorder_compress_quality_id (oracle/_ref/libref_qualid.so, ids only, identity order), and the byte-for-byte comparison
of every block with the file the reference wrote.  usage: python tools/idcodec_probe.py N [repeats] [reads per block]"""
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import pyoracle as po  # noqa: E402

N = int(sys.argv[1])
R = int(sys.argv[2]) if len(sys.argv) > 2 else 3
B = int(sys.argv[3]) if len(sys.argv) > 3 else 256000


def ids_image(n, seed=7, per_tile=250000):
    """instrument:run:flowcell:lane:tile:x:y and a comment; y climbs inside a tile, x is random, as a sequencer's do."""
    rng = np.random.default_rng(seed)
    tile_no = np.arange(n) // per_tile
    tile = 1101 + (tile_no % 78) + 1000 * ((tile_no // 78) % 2) + 100 * ((tile_no // 156) % 6)
    lane = 1 + (tile_no // 936) % 4
    cs = np.cumsum(rng.integers(0, 2, n))
    y = 1000 + cs - np.repeat(cs[::per_tile], per_tile)[:n]
    x = rng.integers(1000, 32000, n)
    parts = []
    for c in range(0, n, 5000000):   # in pieces: the lists of a piece are dropped before the next
        z = zip(lane[c:c + 5000000].tolist(), tile[c:c + 5000000].tolist(), x[c:c + 5000000].tolist(), y[c:c + 5000000].tolist())
        parts.append(b"".join([b"@A00123:45:HXXXXDSXX:%d:%d:%d:%d 1:N:0:ATTAGGCA\n" % t for t in z]))
    return b"".join(parts)


t0 = time.time()
image = ids_image(N)
print("ids: %d, %d bytes, generated in %.1f s; first %r" % (N, len(image), time.time() - t0, image[:54]), flush=True)
nb = (N + B - 1) // B

import spring_amd  # noqa: E402
ref, cpu = [], []
with tempfile.TemporaryDirectory() as d:
    with open(os.path.join(d, "read_order.bin"), "wb") as f:
        f.write(np.arange(N, dtype=np.uint32).tobytes())
    for r in range(R):
        with open(os.path.join(d, "id_1"), "wb") as f:   # the reference removes it when it is done
            f.write(image)
        t = time.time()
        assert po.ref_qualid_lib().ref_q_write(d.encode(), N, 0, B, 16, 0, 1, 0) == 0
        cpu.append(time.time() - t)
    for b in range(nb):
        with open(os.path.join(d, "id_1.%d" % b), "rb") as f:
            ref.append(f.read())
print("reference, 16 threads, reorder_compress_quality_id ids only (reads id_1 once per bin of num_reads / 4 lines, "
      "compress_id_block per block, writes id_1.<b>): s =", ["%.2f" % c for c in cpu], flush=True)

with spring_amd.IdCodecStage() as st:
    tok, cod, wall = [], [], []
    for r in range(R + 1):
        t = time.time()
        info = st.from_lines(image, B)
        wall.append(time.time() - t)
        tok.append(info["ms_tokens"])
        cod.append(info["ms_coder"])
    got = st.blocks()
print("info:", info)
print("device (first run = warm-up): ms_tokens =", ["%.1f" % v for v in tok], "ms_coder =", ["%.1f" % v for v in cod],
      "wall s (upload included) =", ["%.2f" % v for v in wall])
print("blocks: %d, compressed bytes %d (%.2f bytes an id), byte-identical to the reference's files: %s"
      % (nb, sum(map(len, got)), sum(map(len, got)) / N, got == ref))
assert got == ref
