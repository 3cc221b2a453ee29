"""Per-block read streams (include/spring_streams.h) at scale: synthetic reads -> reorder -> encoder -> streams on the
device, single-end in both order modes and the paired-end pool through the device pe_encode.  Prints the device time
of the streams stage (HIP events) and the wall time of its file contract (spring_streams_run on the encoder's files,
written to a temporary directory first; the output files are deleted afterwards).
usage: streams_probe.py [n_reads] [read_len] [reads_per_block] [tmp_dir]"""
import os
import shutil
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

import spring_amd  # noqa: E402
from spring_amd import _lib  # noqa: E402
from spring_amd.encoder import EncoderStage  # noqa: E402
from spring_amd.streams import STREAM_FILES, StreamsStage, stream_names  # noqa: E402

n = int(sys.argv[1]) if len(sys.argv) > 1 else 100_000_000
L = int(sys.argv[2]) if len(sys.argv) > 2 else 150
B = int(sys.argv[3]) if len(sys.argv) > 3 else 256000
tmp_root = sys.argv[4] if len(sys.argv) > 4 else None
G = n * L // 50


def file_contract(e, pe, po):
    """the encoder's files in a fresh directory -> spring_streams_run -> (info, output bytes on disk)."""
    d = tempfile.mkdtemp(prefix="streams_probe_", dir=tmp_root)
    try:
        order = e["order"]
        if pe and not po:
            from spring_amd.order_ops import pe_encode
            order, _ = pe_encode(order)
        for f, v in (("read_pos.bin", e["pos"]), ("read_noise.txt", e["noise"]), ("read_noisepos.bin", e["noisepos"]),
                     ("read_rev.txt", e["rc"]), ("read_order.bin", order), ("read_lengths.bin", e["rlen"]),
                     ("read_unaligned.txt", e["unaligned"]),
                     ("read_unaligned.txt.count", np.array([e["len_unaligned"]], np.uint64))):
            with open(os.path.join(d, f), "wb") as fh:
                fh.write(v if isinstance(v, bytes) else np.ascontiguousarray(v).tobytes())
        info = spring_amd.call_reorder_compress_streams(d, type("cp", (), {"paired_end": pe})(), po, B,
                                                        num_reads=len(e["rlen"]))
        files = os.listdir(d)
        on_disk = sum(os.path.getsize(os.path.join(d, f)) for f in files)
        assert len(files) == info["num_blocks"] * len(stream_names(pe)), len(files)
        return info, on_disk
    finally:
        shutil.rmtree(d, ignore_errors=True)


def run(pe):
    flags = 10000 | (spring_amd.SYNTH_PAIRED if pe else 0)
    with spring_amd.ReorderStage(spring_amd.ReorderOpts(num_chains=0, num_thr=8)) as st:
        st.load_synth(n, L, G, 7, flags)
        t0 = time.time()
        st.run()
        print("%s: reorder %d x %d bp  %.1f s" % ("paired-end" if pe else "single-end", n, L, time.time() - t0), flush=True)
        with EncoderStage() as enc, StreamsStage() as ss:
            ei = enc.encode(st)
            print("  encoder: device %.1f ms, aligned %d of %d, noise %d B, unaligned %d B"
                  % (ei["ms_device"], ei["n_aligned"], ei["n_total"], ei["noise_bytes"], ei["unaligned_bytes"]), flush=True)
            for po in ((False,) if pe else (False, True)):
                for rep in range(2):
                    t0 = time.time()
                    info = ss.from_encoder(enc, n, pe, po, B)
                    wall = (time.time() - t0) * 1e3
                    tot = sum(info["bytes"])
                    print("  streams %s preserve_order=%d pass %d: device %.1f ms (wall %.1f ms), %d blocks, %.2f GB out, "
                          "flags %s, escapes %d" % ("PE+pe_encode" if pe else "SE", po, rep, info["ms_device"], wall,
                                                    info["num_blocks"], tot / 1e9, info["flag_count"], info["pos_escapes"]),
                          flush=True)
                print("    bytes per stream: " + "  ".join("%s %d" % (s, b) for s, b in zip(STREAM_FILES, info["bytes"])))
            e = enc.streams()
    for po in ((False,) if pe else (False, True)):
        info, on_disk = file_contract(e, pe, po)
        print("  file contract %s preserve_order=%d: wall %.1f ms (device %.1f ms), %d files, %.2f GB written"
              % ("PE" if pe else "SE", po, info["ms_file"], info["ms_device"], info["num_blocks"] * len(stream_names(pe)),
                 on_disk / 1e9), flush=True)


if __name__ == "__main__":
    _lib.lib()
    print("streams_probe: n=%d L=%d reads_per_block=%d" % (n, L, B), flush=True)
    run(False)
    run(True)
