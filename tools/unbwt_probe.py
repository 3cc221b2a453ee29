"""Measurement of the inverse block-sort stage: the nine per-block read streams of a synthetic
single-end run, built in HBM as tools/streams_probe.py builds them, transformed by BwtStage at the default 25 MiB cut,
then UnbwtStage.invert over the transform where it lies.

  python tools/unbwt_probe.py [n_reads] [read_len] [--reps R] [--threads T] [--spacings 32,64,128] [--out FILE]

One warm-up lap, then R laps: ms_device and every pass as median with min - max, bytes per second; heads, the longest
walk and the ranking rounds; the same for every head spacing asked for, and per stream at the default one.  The result
is compared with the streams the transform was made from.  Beside it the real bsc_bwt_decode of
oracle/_ref/libref_units.so over the same segments, one segment per thread on T threads, with MULTITHREADING and the
secondary indexes from 64 KiB on as bsc_decompress passes them, its output compared too.  Without oracle/_ref the CPU
line is left out."""
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

FASTMODE, MULTITHREADING = 1, 2
CUT = 25 << 20


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
    U.bsc_bwt_decode.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_ubyte, C.c_void_p, C.c_int]
    assert U.bsc_init(FASTMODE | MULTITHREADING) == 0
    return U


def ref_unbwt(U, L, primary, idx):
    buf = np.frombuffer(L, np.uint8).copy()
    if len(buf) < 64 * 1024:   # bsc_compress stores no indexes below 64 KiB
        idx = idx[:0]
    idx = np.ascontiguousarray(idx, np.int32)
    rc = U.bsc_bwt_decode(buf.ctypes.data, len(buf), primary, len(idx), idx.ctypes.data if len(idx) else None,
                          FASTMODE | MULTITHREADING)
    assert rc == 0, rc
    return buf.tobytes()


def laps(ub, bw, reps):
    runs = []
    for it in range(reps + 1):
        info = ub.invert(bw)
        if it:
            runs.append(info)
    return runs


def report(lines, runs, passes, indent=""):
    info = runs[-1]
    m, lo, hi = stats([r["ms_device"] for r in runs])
    say(lines, indent + "ms_device median %.1f  min %.1f  max %.1f  (%d reps: %s); %.1f MB/s; heads %d, longest walk %d, "
        "ranking rounds %d" % (m, lo, hi, len(runs), " ".join("%.1f" % r["ms_device"] for r in runs), info["bytes"] / m / 1e3,
                               info["heads"], info["max_walk"], info["rank_rounds"]))
    for k, name in enumerate(passes):
        pm, plo, phi = stats([r["ms_pass"][k] for r in runs])
        say(lines, indent + "    %-10s median %9.2f ms  min %9.2f  max %9.2f" % (name, pm, plo, phi))
    return m


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("n", type=int, nargs="?", default=20_000_000)
    ap.add_argument("L", type=int, nargs="?", default=150)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--spacings", default="32,64,128")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = []
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
    from spring_amd.unbwt import PASSES, UnbwtStage
    n, L, B = a.n, a.L, 256000
    U = ref_lib()
    with spring_amd.ReorderStage(spring_amd.ReorderOpts(num_chains=0, num_thr=8)) as st:
        st.load_synth(n, L, n * L // 50, 7, 10000)
        st.run()
        say(lines, "unbwt_probe: single-end %d x %d bp, %d reads per block" % (n, L, B))
        with EncoderStage() as enc, StreamsStage() as ss, BwtStage() as bw, UnbwtStage() as ub:
            enc.encode(st)
            si = ss.from_encoder(enc, n, False, False, B)
            fi = bw.transform(ss)
            say(lines, "streams: %d blocks, %.3f GB; transformed at the 25 MiB cut: %d segments, longest %d bytes, forward ms_device %.1f"
                % (si["num_blocks"], sum(si["bytes"]) / 1e9, fi["num_segments"], fi["max_segment"], fi["ms_device"]))
            median = {}
            for K in [int(x) for x in a.spacings.split(",")]:
                ub.set_head_spacing(K)
                runs = laps(ub, bw, a.reps)
                info = runs[-1]
                say(lines, "head spacing %d: %d segments, %.3f GB, %d sub-batches (workspace budget %.1f GB)"
                    % (K, info["num_segments"], info["bytes"] / 1e9, info["sub_batches"], info["workspace_bytes"] / 1e9))
                median[K] = report(lines, runs, PASSES, "  ")
            ub.set_head_spacing(0)
            info = ub.invert(bw)
            K0 = info["head_spacing"]
            text = ub.download()
            fwd = bw.download()
            stream, block, cut = bw.segments()
            data = {s: ss.download(s) for s in range(len(STREAM_FILES)) if si["bytes"][s]}
            segs = []
            for s, b, c in zip(stream.tolist(), block.tolist(), cut.tolist()):
                d, off = data[s]
                lo = int(off[b]) + c * CUT
                segs.append(d[lo:min(lo + CUT, int(off[b + 1]))])
            same = text["text"] == b"".join(segs)
            say(lines, "the default spacing is %d; its result %s the streams the transform was made from"
                % (K0, "EQUALS" if same else "DIFFERS FROM"))
            for s in sorted(data):
                bw.transform(ss, streams=[s])
                runs = laps(ub, bw, 2)
                i1 = runs[-1]
                m1 = stats([r["ms_device"] for r in runs])[0]
                say(lines, "  %-20s %5d segments %12d bytes, longest %9d: heads %8d, longest walk %5d, ranking rounds %2d, ms_device %8.2f, "
                    "%7.1f MB/s  (%s)" % (STREAM_FILES[s], i1["num_segments"], i1["bytes"], i1["max_segment"], i1["heads"],
                                         i1["max_walk"], i1["rank_rounds"], m1, i1["bytes"] / m1 / 1e3,
                                         " ".join("%s %.2f" % (p, x) for p, x in zip(PASSES, i1["ms_pass"]))))
    if U is None:
        say(lines, "oracle/_ref/libref_units.so is not built: no CPU line")
        return
    off = fwd["seg_off"]
    jobs = [(fwd["bwt"][int(off[j]):int(off[j + 1])], int(fwd["primary"][j]), fwd["indexes"][j][:fwd["num_indexes"][j]])
            for j in range(len(segs))]
    t0 = time.perf_counter()
    with ThreadPoolExecutor(a.threads) as ex:
        ref = list(ex.map(lambda j: ref_unbwt(U, *j), jobs))
    t_cpu = time.perf_counter() - t0
    toff = text["seg_off"]
    same = all(text["text"][int(toff[j]):int(toff[j + 1])] == r == segs[j] for j, r in enumerate(ref))
    nbytes = sum(len(s) for s in segs)
    say(lines, "bsc_bwt_decode (features FASTMODE | MULTITHREADING, indexes from 64 KiB on) over the same %d segments, one segment per "
        "thread on %d threads: %.2f s wall, %.1f MB/s; every segment %s the device's and the stream's; CPU / device (spacing %d): %.1fx"
        % (len(segs), a.threads, t_cpu, nbytes / t_cpu / 1e6, "EQUALS" if same else "DIFFERS FROM", K0,
           t_cpu * 1e3 / median.get(K0, float("nan"))))


if __name__ == "__main__":
    main()
