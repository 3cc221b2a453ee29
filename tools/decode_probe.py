"""Stream decoder (include/spring_decode.h) at scale: synthetic reads -> reorder -> encoder -> streams -> decode, all
on the device, single-end in both order modes and the paired-end pool through the device pe_encode.  Prints the
device time of the decoder (HIP events, two passes), its output bytes, the time to download the reads, the wall time
of its file contract (seq_from_files once, then from_files per step of num_thr blocks, on files written to a
temporary directory first) and checks every decoded read against the synthetic original.
usage: decode_probe.py [n_reads] [read_len] [reads_per_block] [tmp_dir] [--no-files]"""
import os
import shutil
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

import spring_amd  # noqa: E402
from spring_amd import _lib  # noqa: E402
from spring_amd.decode import DecodeStage  # noqa: E402
from spring_amd.encoder import EncoderStage  # noqa: E402
from spring_amd.order_ops import pe_encode  # noqa: E402
from spring_amd.streams import StreamsStage, stream_names  # noqa: E402

args = [a for a in sys.argv[1:] if not a.startswith("--")]
n = int(args[0]) if len(args) > 0 else 100_000_000
L = int(args[1]) if len(args) > 1 else 150
B = int(args[2]) if len(args) > 2 else 256000
tmp_root = args[3] if len(args) > 3 else None
files = "--no-files" not in sys.argv
G = n * L // 50
NUM_THR = 8   # reorder tids = consensus files; also the blocks per from_files step


def check(ds, pe, slot_ids, body):
    """every decoded read of every mate against the synthetic original it stands for -> (download ms, bytes)."""
    U = n // 2 if pe else n
    j = np.arange(L)
    lut = np.frombuffer(b"AGCT", np.uint8)
    ms, nbytes = 0.0, 0
    for m in range(2 if pe else 1):
        t0 = time.time()
        data, off = ds.download(m)
        ms += (time.time() - t0) * 1e3
        nbytes += len(data)
        assert np.array_equal(off, np.arange(U + 1, dtype=np.uint64) * L), "read offsets"
        got = np.frombuffer(data, np.uint8).reshape(U, L)
        ids = slot_ids[m * U:(m + 1) * U]
        for lo in range(0, U, 4_000_000):
            sel = ids[lo:lo + 4_000_000]
            codes = (body[sel][:, j >> 2] >> (2 * (j & 3)).astype(np.uint8)) & 3
            assert np.array_equal(got[lo:lo + 4_000_000], lut[codes]), (m, lo)
        del data, got
    return ms, nbytes


def file_contract(ss, pe, po, packed, tails, seq_len_tid, want):
    """the streams as <stream>.<b> and the consensus as read_seq.bin.<tid> (+ .tail) in a fresh directory ->
    seq_from_files, then from_files per step of NUM_THR blocks -> (wall ms of the decoder's calls, equal to want)."""
    d = tempfile.mkdtemp(prefix="decode_probe_", dir=tmp_root)
    try:
        nb = ss.info["num_blocks"]
        for s in stream_names(pe):
            data, off = ss.download(s)
            for b in range(nb):
                with open(os.path.join(d, "%s.%d" % (s, b)), "wb") as fh:
                    fh.write(data[int(off[b]):int(off[b + 1])])
        o = 0
        for t, ln in enumerate(seq_len_tid):
            with open(os.path.join(d, "read_seq.bin.%d" % t), "wb") as fh:
                fh.write(packed[o:o + int(ln) // 4])
            with open(os.path.join(d, "read_seq.bin.%d.tail" % t), "w") as fh:
                fh.write(tails[t])
            o += int(ln) // 4
        with DecodeStage() as ds:
            t0 = time.time()
            ds.seq_from_files(d, len(seq_len_tid))
            wall = (time.time() - t0) * 1e3
            same = True
            pos = [0, 0]
            for b0 in range(0, nb, NUM_THR):
                k = min(NUM_THR, nb - b0)
                info = ds.from_files(d, b0, k, n, pe, po, B)
                wall += info["ms_file"]
                for m in range(2 if pe else 1):
                    data, _ = ds.download(m)
                    same = same and data == want[m][pos[m]:pos[m] + len(data)]
                    pos[m] += len(data)
            assert not os.listdir(d), "inputs left behind"
        return wall, same and pos[0] == len(want[0])
    finally:
        shutil.rmtree(d, ignore_errors=True)


def run(pe):
    flags = 10000 | (spring_amd.SYNTH_PAIRED if pe else 0)
    t0 = time.time()
    body = None
    if files:   # the host copy of the synthetic reads, for the check
        body = np.frombuffer(spring_amd.synth_dna_host(n, L, G, 7, flags), np.uint8).reshape(n, 2 + (L + 3) // 4)[:, 2:]
    print("%s: %d x %d bp synthetic (host copy %.1f s)" % ("paired-end" if pe else "single-end", n, L, time.time() - t0),
          flush=True)
    with spring_amd.ReorderStage(spring_amd.ReorderOpts(num_chains=0, num_thr=NUM_THR)) as st:
        st.load_synth(n, L, G, 7, flags)
        st.run()
        with EncoderStage() as enc, StreamsStage() as ss, DecodeStage() as ds:
            enc.encode(st)
            e = enc.streams()
            order, seq_len_tid = e["order"], e["seq_len_tid"]
            del e
            packed, tails = enc.seq_packed()
            ds.seq_from_encoder(enc)
            print("  consensus %d bases in %d tids" % (int(sum(seq_len_tid)), len(seq_len_tid)), flush=True)
            for po in ((False,) if pe else (False, True)):
                si = ss.from_encoder(enc, n, pe, po, B)
                sbytes = sum(si["bytes"])
                for rep in range(2):
                    t0 = time.time()
                    info = ds.from_streams(ss)
                    wall = (time.time() - t0) * 1e3
                    print("  decode %s preserve_order=%d pass %d: device %.2f ms (wall %.1f ms), %d blocks, "
                          "%.2f GB streams in, %.2f GB bases out, aligned %d, unaligned %d, escapes %d"
                          % ("PE" if pe else "SE", po, rep, info["ms_device"], wall, info["num_blocks"], sbytes / 1e9,
                             sum(info["bases"]) / 1e9, info["n_aligned"], info["n_unaligned"], info["pos_escapes"]),
                          flush=True)
                if po:
                    ids = np.arange(n)
                else:
                    slot = pe_encode(order)[0] if pe else np.arange(n)
                    ids = np.empty(n, np.int64)
                    ids[slot] = order
                if files:
                    t0 = time.time()
                    ms_dl, nbytes = check(ds, pe, ids, body)
                    print("  download %.2f GB of bases: %.1f ms; every read equals its synthetic original (check %.1f s)"
                          % (nbytes / 1e9, ms_dl, time.time() - t0 - ms_dl / 1e3), flush=True)
                    want = [ds.download(m)[0] for m in range(2 if pe else 1)]
                    wall, same = file_contract(ss, pe, po, packed, tails, seq_len_tid, want)
                    del want
                    print("  file contract: seq_from_files + from_files per %d blocks: wall %.1f ms; output equals the "
                          "in-memory decode: %s" % (NUM_THR, wall, same), flush=True)
                    assert same


if __name__ == "__main__":
    _lib.lib()
    print("decode_probe: n=%d L=%d reads_per_block=%d" % (n, L, B), flush=True)
    run(False)
    run(True)
