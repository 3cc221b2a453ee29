"""Measurement of the FASTQ assembler: the text of a synthetic single-end FASTQ (the records of
tools/qualid_probe.py, the same random order) assembled from its reads, quality lines and id lines in the final order,
beside spring_fastq_reorder (whole 4-line records, one byte per lane), which writes the same bytes from the same text.

  python tools/fastq_out_probe.py N L [--reps R] [--no-yardstick] [--write DIR] [--out FILE]

Quality and id lines are in HBM (a QualIdStage that ran on the text with the order); the reads are given from the host
in slot order, as DecodeStage.download would give them: a decode context needs the whole compression chain in front
of it, and ms_device excludes the input copies either way.  Device times are the library's own HIP-event spans; the
two programs alternate inside one process, the first lap warms up, the report gives every repetition, the median and
the spread.  The assembled text is compared with the yardstick's, byte for byte.  --write DIR times write() into a
file under DIR (removed afterwards) and into /dev/null (the copy over PCIe alone)."""
import argparse
import ctypes as C
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

from spring_amd import FastqOutStage, _lib  # noqa: E402
from spring_amd.qualid import QualIdStage  # noqa: E402
from qualid_probe import make_text, stats  # noqa: E402

HBM_PEAK_GBS = 8000.0   # the peak bench.py --full states roofline.frac against


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("n", type=int)
    ap.add_argument("L", type=int)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-yardstick", action="store_true")
    ap.add_argument("--write", default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    n, L = a.n, a.L
    t0 = time.perf_counter()
    text, rec = make_text(n, L)
    order = np.random.default_rng(7).permutation(n).astype(np.uint32)
    bases = np.ascontiguousarray(text.reshape(n, rec)[order, 11:11 + L]).reshape(-1)   # slot i holds record order[i]
    read_off = np.arange(n + 1, dtype=np.uint64) * np.uint64(L)
    lines = ["n=%d L=%d text=%.3f GB (%d-byte records), random order, num_reads_per_block=256000; built in %.0f s"
             % (n, L, len(text) / 1e9, rec, time.perf_counter() - t0)]
    Lb = _lib.lib()
    yard_out = np.empty(len(text), np.uint8) if not a.no_yardstick else None
    need, ms = C.c_size_t(), C.c_double()
    runs, ys = [], []
    with QualIdStage() as qs, FastqOutStage() as fo:
        qs.set_order(order, n)
        qs.from_fastq(text)
        for it in range(a.reps + 1):   # the first lap warms up (code objects, the device pool)
            info = fo.assemble((bases, read_off), n, quality=qs, ids=qs)
            if it:
                runs.append(info["ms_device"])
            if yard_out is not None and it <= min(a.reps, 3):
                rc = Lb.spring_fastq_reorder(text.ctypes.data, len(text), order.ctypes.data, n, yard_out.ctypes.data,
                                             len(yard_out), C.byref(need), C.byref(ms))
                assert rc == 0 and need.value == len(text), (rc, need.value)
                if it:
                    ys.append(ms.value)
        out_b = info["bytes"]
        idb = qs.info["bytes"][1]
        # what the passes have to move, from the shapes: the newline passes read the ids twice and write the index;
        # k_lines reads the index and the read offsets and writes start / length / patch / size; the scan; the copy reads
        # those, the three sources and the record offsets, and writes the text
        side = n * (8 + 4 + 4 + 4)
        rd = 2 * idb + 8 * n + 8 * n + side + 8 * n + 8 * n + out_b - 4 * n
        wr = 8 * n + side + 8 * n + out_b
        m, lo, hi = stats(runs)
        lines.append("assemble (quality + ids in HBM, four-line records): %.3f GB out; ms_device median %.2f  min %.2f  "
                     "max %.2f  (%d reps: %s)  %.0f GB/s read+written, roofline.frac %.4f of %.0f GB/s; %.0f GB/s of output, "
                     "%.4f ns per output byte"
                     % (out_b / 1e9, m, lo, hi, len(runs), " ".join("%.2f" % x for x in runs), (rd + wr) / m / 1e6,
                        (rd + wr) / m / 1e6 / HBM_PEAK_GBS, HBM_PEAK_GBS, out_b / m / 1e6, m * 1e6 / out_b))
        if yard_out is not None:
            ym, ylo, yhi = stats(ys)
            nlines = 4 * n
            yrd = 2 * len(text) + 8 * nlines + n * (4 + 4 + 8) + len(text)
            ywr = 8 * nlines + n * (4 + 8) + len(text)
            lines.append("spring_fastq_reorder (same text and order): %.3f GB out; kernel_ms median %.2f  min %.2f  max %.2f  "
                         "(%d reps: %s)  %.0f GB/s read+written, roofline.frac %.4f; %.0f GB/s of output, %.4f ns per output byte"
                         % (len(text) / 1e9, ym, ylo, yhi, len(ys), " ".join("%.2f" % x for x in ys), (yrd + ywr) / ym / 1e6,
                            (yrd + ywr) / ym / 1e6 / HBM_PEAK_GBS, len(text) / ym / 1e6, ym * 1e6 / len(text)))
            lines.append("  assemble / spring_fastq_reorder: time %.3f (spread of assemble %.2f ms, of the yardstick %.2f ms)"
                         % (m / ym, hi - lo, yhi - ylo))
            got = fo.download_array()
            lines.append("  the assembled text %s the yardstick's (%d bytes)"
                         % ("EQUALS" if np.array_equal(got, yard_out) else "DIFFERS FROM", len(got)))
            del got
        if a.write:
            path = os.path.join(a.write, "fastq_out_probe.%d.fastq" % os.getpid())
            for target in (os.devnull, path, os.devnull, path):
                what = "/dev/null: the copy over PCIe alone" if target == os.devnull else "a file under " + a.write
                t1 = time.perf_counter()
                try:
                    wi = fo.write(target)
                except Exception as e:   # a full or read-only directory must not cost the measurements above
                    lines.append("write(%s) failed: %s" % (what, e))
                    continue
                wall = (time.perf_counter() - t1) * 1e3
                lines.append("write(%s): %.0f ms wall (ms_file %.0f), %.2f GB/s" % (what, wall, wi["ms_file"], out_b / wall / 1e6))
            if os.path.exists(path):
                os.remove(path)
    rep = "\n".join(lines) + "\n"
    sys.stdout.write(rep)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(rep)


if __name__ == "__main__":
    main()
