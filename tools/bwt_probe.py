"""Measurement of the block-sort stage: the nine per-block read streams of a synthetic
single-end run, built in HBM as tools/streams_probe.py builds them, then BwtStage.transform over all of them at the
default 25 MiB cut.

  python tools/bwt_probe.py [n_reads] [read_len] [--reps R] [--threads T] [--out FILE]
  python tools/bwt_probe.py --golden [--out FILE]        (CPU only: the LZP table of the tests/golden stream fixtures)

One warm-up lap, then R laps: ms_device and every pass as median with min - max, bytes per second of input; rounds and
sub-batches per stream from one lap per stream.  Beside them the real bsc_bwt_encode of oracle/_ref/libref_units.so
over the same segments, one block per thread on T threads as SPRING's OpenMP loop runs them, its output compared with
the device's; and per stream the block sizes of the real bsc_compress with LZP (16, 128) and with LZP off: the price of
skipping LZP.  Without oracle/_ref the CPU columns are left out."""
import argparse
import ctypes as C
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

from oracle import pyoracle as po  # noqa: E402

PASSES = ("keys", "sort", "re-rank", "compaction", "gather + indexes")
FASTMODE = 1


def say(lines, s):
    lines.append(s)
    print(s, flush=True)


def stats(v):
    v = sorted(v)
    return v[len(v) // 2], v[0], v[-1]


def ref_lib():
    U = po.ref_units()
    if U is None:
        return None
    U.bsc_init.argtypes = [C.c_int]
    U.bsc_bwt_encode.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_ubyte), C.c_void_p, C.c_int]
    U.bsc_compress.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]
    assert U.bsc_init(FASTMODE) == 0
    return U


def ref_bwt(U, seg):
    buf = np.frombuffer(seg, np.uint8).copy()
    num = C.c_ubyte(0)
    idx = np.zeros(256, np.int32)
    primary = U.bsc_bwt_encode(buf.ctypes.data, len(buf), C.byref(num), idx.ctypes.data, FASTMODE)
    return buf.tobytes(), primary, idx[:num.value].copy()


def block_sizes(U, seg):
    """-> (bytes of bsc_compress with LZP (16, 128), with LZP off) for one block."""
    src = np.frombuffer(seg, np.uint8)
    out = np.zeros(len(seg) + 28 + 4096, np.uint8)
    a = U.bsc_compress(src.ctypes.data, out.ctypes.data, len(seg), 16, 128, 1, 1, FASTMODE)
    b = U.bsc_compress(src.ctypes.data, out.ctypes.data, len(seg), 0, 0, 1, 1, FASTMODE)
    assert a > 0 and b > 0
    return a, b


def lzp_table(lines, U, named_segments, threads):
    """named_segments: [(name, [segment bytes ...])] -> one line per name."""
    say(lines, "%-28s %8s %14s %14s %14s %9s" % ("blocks of", "blocks", "bytes in", "LZP (16, 128)", "LZP off", "change"))
    with ThreadPoolExecutor(threads) as ex:
        for name, segs in named_segments:
            segs = [s for s in segs if len(s)]
            if not segs:
                continue
            r = list(ex.map(lambda s: block_sizes(U, s), segs))
            a, b = sum(x[0] for x in r), sum(x[1] for x in r)
            say(lines, "%-28s %8d %14d %14d %14d %+8.3f%%" % (name, len(segs), sum(len(s) for s in segs), a, b, 100.0 * (b - a) / a))


def golden(lines, threads):
    U = ref_lib()
    assert U is not None, "oracle/_ref/libref_units.so is not built"
    gold = os.path.join(ROOT, "tests", "golden")
    named = []
    for f in sorted(os.listdir(gold)):
        if not (f.startswith("ref_streams_") and f.endswith(".npz")):
            continue
        z = np.load(os.path.join(gold, f))
        names = sorted(k[:-len(".off")] for k in z.files if k.endswith(".off"))
        segs = []
        for k in names:
            data, off = z[k].tobytes(), z[k + ".off"]
            segs += [data[int(off[b]):int(off[b + 1])] for b in range(len(off) - 1)]
        named.append((f[len("ref_streams_"):-4], segs))
    say(lines, "the stream blocks of tests/golden/ref_streams_*.npz (all streams of a fixture together):")
    lzp_table(lines, U, named, threads)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("n", type=int, nargs="?", default=20_000_000)
    ap.add_argument("L", type=int, nargs="?", default=150)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--golden", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = []
    if a.golden:
        golden(lines, a.threads)
    else:
        device(lines, a)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


def device(lines, a):
    import spring_amd
    from spring_amd.bwt import BwtStage
    from spring_amd.encoder import EncoderStage
    from spring_amd.streams import STREAM_FILES, StreamsStage
    n, L, B = a.n, a.L, 256000
    U = ref_lib()
    with spring_amd.ReorderStage(spring_amd.ReorderOpts(num_chains=0, num_thr=8)) as st:
        st.load_synth(n, L, n * L // 50, 7, 10000)
        t0 = time.time()
        st.run()
        say(lines, "bwt_probe: single-end %d x %d bp, %d reads per block; reorder %.1f s" % (n, L, B, time.time() - t0))
        with EncoderStage() as enc, StreamsStage() as ss, BwtStage() as bw:
            enc.encode(st)
            si = ss.from_encoder(enc, n, False, False, B)
            say(lines, "streams: %d blocks, %.3f GB; bytes per stream: %s"
                % (si["num_blocks"], sum(si["bytes"]) / 1e9, "  ".join("%s %d" % (s, b) for s, b in zip(STREAM_FILES, si["bytes"]))))
            runs = []
            for it in range(a.reps + 1):
                info = bw.transform(ss)
                if it:
                    runs.append(info)
            m, lo, hi = stats([r["ms_device"] for r in runs])
            say(lines, "all nine streams, 25 MiB cut: %d segments, %.3f GB, longest %d bytes, %d sub-batches (workspace budget %.1f GB), "
                "rounds %d (most of a sub-batch; %d summed)" % (info["num_segments"], info["bytes"] / 1e9, info["max_segment"],
                                                               info["sub_batches"], info["workspace_bytes"] / 1e9, info["rounds"],
                                                               info["rounds_total"]))
            say(lines, "ms_device median %.1f  min %.1f  max %.1f  (%d reps: %s); %.1f MB/s of input"
                % (m, lo, hi, len(runs), " ".join("%.1f" % r["ms_device"] for r in runs), info["bytes"] / m / 1e3))
            for k, name in enumerate(PASSES):
                pm, plo, phi = stats([r["ms_pass"][k] for r in runs])
                say(lines, "    %-18s median %9.2f ms  min %9.2f  max %9.2f" % (name, pm, plo, phi))
            res = bw.download()
            stream, block, cut = bw.segments()
            for s in range(len(STREAM_FILES)):
                if not si["bytes"][s]:
                    continue
                bw.transform(ss, streams=[s])
                i1 = bw.transform(ss, streams=[s])
                say(lines, "  %-20s %5d segments %12d bytes, longest %9d: %2d sub-batches, rounds %2d (%3d summed), ms_device %9.1f, %7.1f MB/s"
                    % (STREAM_FILES[s], i1["num_segments"], i1["bytes"], i1["max_segment"], i1["sub_batches"], i1["rounds"],
                       i1["rounds_total"], i1["ms_device"], i1["bytes"] / i1["ms_device"] / 1e3))
            if U is None:
                say(lines, "oracle/_ref/libref_units.so is not built: no CPU columns")
                return
            # the same segments on the host: the streams downloaded, cut as the stage cuts them
            data = {s: ss.download(s) for s in range(len(STREAM_FILES)) if si["bytes"][s]}
    segs = []
    for s, b, c in zip(stream.tolist(), block.tolist(), cut.tolist()):
        d, off = data[s]
        lo = int(off[b]) + c * (25 << 20)
        segs.append(d[lo:min(lo + (25 << 20), int(off[b + 1]))])
    t0 = time.perf_counter()
    with ThreadPoolExecutor(a.threads) as ex:
        ref = list(ex.map(lambda s: ref_bwt(U, s), segs))
    t_cpu = time.perf_counter() - t0
    off = res["seg_off"]
    same = all(res["bwt"][int(off[j]):int(off[j + 1])] == r[0] and res["primary"][j] == r[1]
               and np.array_equal(res["indexes"][j][:res["num_indexes"][j]], r[2]) for j, r in enumerate(ref))
    nbytes = sum(len(s) for s in segs)
    say(lines, "bsc_bwt_encode (features FASTMODE) over the same %d segments, one block per thread on %d threads: %.2f s wall, "
        "%.1f MB/s; bytes, primary index and indexes of every segment %s the device's; CPU / device: %.1fx"
        % (len(segs), a.threads, t_cpu, nbytes / t_cpu / 1e6, "EQUAL" if same else "DIFFER FROM", t_cpu * 1e3 / m))
    named = [(STREAM_FILES[s], [g for g, t in zip(segs, stream.tolist()) if t == s]) for s in sorted(data)]
    lzp_table(lines, U, named + [("all streams", segs)], a.threads)


if __name__ == "__main__":
    main()
