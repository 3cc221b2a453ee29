"""g3 measurement: quality + id lines of a synthetic single-end FASTQ (the fixed-width records of tools/fastq_probe.py,
qualities spread over 33..73) into a random final order, with and without the Illumina table, beside
spring_fastq_reorder (whole 4-line records, one byte per lane) on the same text and order.

  python tools/qualid_probe.py N L [--reps R] [--no-yardstick] [--out FILE]

Device times are the library's own HIP-event spans (input copy excluded).  The variants alternate inside one process;
the report gives every repetition, the median and the spread.  Bytes are algorithmic: what the passes have to read
and write, computed from the shapes, not counters."""
import argparse
import ctypes as C
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

import spring_amd  # noqa: E402
from spring_amd import _lib  # noqa: E402
from spring_amd.qualid import QualIdStage  # noqa: E402

HBM_PEAK_GBS = 8000.0   # the peak bench.py --full states roofline.frac against


def make_text(n, L, seed=3, unit=1 << 20):
    """n records "@rDDDDDDDD\\n" + read + "\\n+\\n" + quality + "\\n"; the bases and qualities of `unit` records, tiled."""
    rng = np.random.default_rng(seed)
    u = min(n, unit)
    rec = 11 + L + 3 + L + 1
    a = np.empty((u, rec), np.uint8)
    a[:, 0] = ord("@"); a[:, 1] = ord("r"); a[:, 10] = ord("\n")
    a[:, 11:11 + L] = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, (u, L))]
    a[:, 11 + L] = ord("\n"); a[:, 12 + L] = ord("+"); a[:, 13 + L] = ord("\n")
    a[:, 14 + L:14 + 2 * L] = rng.integers(33, 74, (u, L), dtype=np.uint8)
    a[:, 14 + 2 * L] = ord("\n")
    t = np.tile(a, ((n + u - 1) // u, 1))[:n]
    idx = np.arange(n)
    for d in range(8):
        t[:, 9 - d] = ord("0") + (idx // 10 ** d) % 10
    return t.reshape(-1), rec


def stats(ms):
    ms = sorted(ms)
    return ms[len(ms) // 2], ms[0], ms[-1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("n", type=int)
    ap.add_argument("L", type=int)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-yardstick", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    n, L = a.n, a.L
    t0 = time.perf_counter()
    text, rec = make_text(n, L)
    order = np.random.default_rng(7).permutation(n).astype(np.uint32)
    lines = ["n=%d L=%d text=%.3f GB (%d-byte records), random order, num_reads_per_block=256000; built in %.0f s"
             % (n, L, len(text) / 1e9, rec, time.perf_counter() - t0)]
    table = QualIdStage.quality_table("illumina")
    runs = {"plain": [], "illumina": []}
    info = None
    with QualIdStage() as qs:
        qs.set_order(order, n)
        for it in range(a.reps + 1):   # the first lap warms up (code objects, the device pool)
            for name, t in (("plain", None), ("illumina", table)):
                info = qs.from_fastq(text, table=t)
                if it:
                    runs[name].append(info["ms_device"])
                if name == "illumina":
                    changed = info["bytes_changed"]
    out_b = sum(info["bytes"])
    nlines = 4 * n
    side = 2 * n * (8 + 4 + 8)   # start, len, off per unit and kind
    rd = 2 * len(text) + 8 * nlines + side + out_b
    wr = 8 * nlines + side + out_b
    lines.append("from_fastq want=quality+id: quality %.3f GB + id %.3f GB out; algorithmic bytes read %.3f GB "
                 "(text twice for the newline index, the index, the per-line arrays, the lines) written %.3f GB"
                 % (info["bytes"][0] / 1e9, info["bytes"][1] / 1e9, rd / 1e9, wr / 1e9))
    med = {}
    for name in ("plain", "illumina"):
        m, lo, hi = stats(runs[name])
        med[name] = m
        lines.append("  %-8s ms_device median %.2f  min %.2f  max %.2f  (%d reps: %s)  %.0f GB/s read+written, "
                     "roofline.frac %.4f of %.0f GB/s; %.0f GB/s of output, %.4f ns per output byte"
                     % (name, m, lo, hi, len(runs[name]), " ".join("%.2f" % x for x in runs[name]), (rd + wr) / m / 1e6,
                        (rd + wr) / m / 1e6 / HBM_PEAK_GBS, HBM_PEAK_GBS, out_b / m / 1e6, m * 1e6 / out_b))
    lines.append("  table - plain = %+.2f ms (%+.1f %%); spread of plain %.2f ms; bytes_changed %d"
                 % (med["illumina"] - med["plain"], 100 * (med["illumina"] - med["plain"]) / med["plain"],
                    max(runs["plain"]) - min(runs["plain"]), changed))
    if not a.no_yardstick:
        Lb = _lib.lib()
        out = np.empty(len(text), np.uint8)
        need, ms = C.c_size_t(), C.c_double()
        ys = []
        for it in range(min(a.reps, 3) + 1):
            rc = Lb.spring_fastq_reorder(text.ctypes.data, len(text), order.ctypes.data, n, out.ctypes.data, len(out),
                                         C.byref(need), C.byref(ms))
            assert rc == 0 and need.value == len(text), (rc, need.value)
            if it:
                ys.append(ms.value)
        m, lo, hi = stats(ys)
        yrd = 2 * len(text) + 8 * nlines + n * (4 + 4 + 8) + len(text)
        ywr = 8 * nlines + n * (4 + 8) + len(text)
        lines.append("spring_fastq_reorder (same text and order): %.3f GB out; kernel_ms median %.2f  min %.2f  max %.2f  "
                     "(%d reps: %s)  %.0f GB/s read+written, roofline.frac %.4f; %.0f GB/s of output, %.4f ns per output byte"
                     % (len(text) / 1e9, m, lo, hi, len(ys), " ".join("%.2f" % x for x in ys), (yrd + ywr) / m / 1e6,
                        (yrd + ywr) / m / 1e6 / HBM_PEAK_GBS, len(text) / m / 1e6, m * 1e6 / len(text)))
        lines.append("  from_fastq / spring_fastq_reorder: time %.3f, output bytes %.3f, time per output byte %.3f"
                     % (med["plain"] / m, out_b / len(text), (med["plain"] / out_b) / (m / len(text))))
    rep = "\n".join(lines) + "\n"
    sys.stdout.write(rep)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(rep)


if __name__ == "__main__":
    main()
