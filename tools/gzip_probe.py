"""Measurement of the gzip stage on the workload of tools/fastq_out_probe.py: the text of a
synthetic single-end FASTQ assembled in HBM, then compressed there into gzip members.

  python tools/gzip_probe.py N L [--reps R] [--member-records M] [--sample-mib S] [--write DIR] [--out FILE]

For every chunk size tried: ms_device of the library's own HIP-event span and of every pass, bytes_out / bytes_in.  The
first lap of every size warms up; every repetition, the median and the spread are reported.  Beside them zlib level 1
and level 6 on the first S MiB of the same text (CPU, timed, one thread and 16 threads), the download of the compressed
result against the plain text's (write() to /dev/null: the copy over PCIe alone), and the whole way to a file under
DIR against the caller's alternative today: the plain download plus zlib level 1 on 16 threads, scaled from the sample.
The result of the default chunk size is inflated and compared with the text."""
import argparse
import os
import sys
import time
import zlib
from concurrent.futures import ThreadPoolExecutor

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

from spring_amd import FastqOutStage, GzipStage  # noqa: E402
from spring_amd.qualid import QualIdStage  # noqa: E402
from qualid_probe import make_text, stats  # noqa: E402

PASSES = ("chunk table", "match + parse", "codes", "emit", "crc32", "compaction")
SIZES = (16384, 32768, 49152, 65536)


def fastq_shaped(n=20000):
    """A text with what the probe's own has none of: counting ids, reads drawn with overlap from a 50 kb genome, quality
    lines from a table of 64 (the text of tests/test_gpu_gzip.py)."""
    rng = np.random.default_rng(5)
    genome = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, 50000)]
    qtab = [bytes(rng.choice(np.frombuffer(b"FFFFFFFF:,#IIJJ?A<", np.uint8), 100)) for _ in range(64)]
    starts = rng.integers(0, 50000 - 100, n)
    which = rng.integers(0, 64, n)
    return b"".join(b"@SRR1234567.%d %d length=100\n%s\n+\n%s\n" % (i + 1, i + 1, genome[s:s + 100].tobytes(), qtab[w])
                    for i, (s, w) in enumerate(zip(starts.tolist(), which.tolist())))


def say(lines, s):
    lines.append(s)
    print(s, flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("n", type=int)
    ap.add_argument("L", type=int)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--member-records", type=int, default=0)
    ap.add_argument("--sample-mib", type=int, default=256)
    ap.add_argument("--write", default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    n, L = a.n, a.L
    lines = []
    t0 = time.perf_counter()
    text, rec = make_text(n, L)
    order = np.random.default_rng(7).permutation(n).astype(np.uint32)
    bases = np.ascontiguousarray(text.reshape(n, rec)[order, 11:11 + L]).reshape(-1)
    read_off = np.arange(n + 1, dtype=np.uint64) * np.uint64(L)
    say(lines, "n=%d L=%d text=%.3f GB (%d-byte records), random order, member_records=%d; built in %.0f s"
        % (n, L, len(text) / 1e9, rec, a.member_records, time.perf_counter() - t0))
    with QualIdStage() as qs, FastqOutStage() as fo, GzipStage() as gs:
        qs.set_order(order, n)
        qs.from_fastq(text)
        del text
        fi = fo.assemble((bases, read_off), n, quality=qs, ids=qs)
        fi = fo.assemble((bases, read_off), n, quality=qs, ids=qs)
        nbytes = fi["bytes"]
        say(lines, "assemble: %.3f GB, ms_device %.2f" % (nbytes / 1e9, fi["ms_device"]))
        gs.compress(b"x")
        default = gs.info["chunk_bytes"]
        results = {}
        for cb in [s for s in SIZES if s != default] + [default]:   # the default last: its result stays in the context
            gs.set_chunk_bytes(cb)
            runs = []
            for it in range(a.reps + 1):
                info = gs.compress(fo, member_records=a.member_records)
                if it:
                    runs.append(info)
            m, lo, hi = stats([r["ms_device"] for r in runs])
            results[cb] = (m, info["bytes_out"] / nbytes)
            say(lines, "chunk_bytes %5d%s: %d members, %d chunks (%d stored), %.3f GB out, ratio %.4f; ms_device median %.1f  "
                "min %.1f  max %.1f  (%d reps: %s); %.2f GB/s of input"
                % (cb, " (default)" if cb == default else "", info["num_members"], info["num_chunks"], info["chunks_stored"],
                   info["bytes_out"] / 1e9, info["bytes_out"] / nbytes, m, lo, hi, len(runs),
                   " ".join("%.1f" % r["ms_device"] for r in runs), nbytes / m / 1e6))
            for k, name in enumerate(PASSES):
                pm, plo, phi = stats([r["ms_pass"][k] for r in runs])
                say(lines, "    %-14s median %8.2f ms  min %8.2f  max %8.2f" % (name, pm, plo, phi))
        info = gs.info
        # the window a chunk size leaves (min(32768, 65536 - chunk_bytes)) shows on a text that repeats
        shaped = fastq_shaped()
        with GzipStage() as g2:
            for cb in SIZES:
                g2.set_chunk_bytes(cb)
                si = g2.compress(shaped)
                say(lines, "repeating text (%d bytes: counting ids, overlapping reads, 64 quality lines), chunk_bytes %5d: ratio "
                    "%.4f (zlib level 1 %.4f, level 6 %.4f)" % (len(shaped), cb, si["bytes_out"] / len(shaped),
                                                               len(zlib.compress(shaped, 1)) / len(shaped),
                                                               len(zlib.compress(shaped, 6)) / len(shaped)))
        # zlib on the head of the same text
        t1 = time.perf_counter()
        plain = fo.download_array()
        say(lines, "download of the text to pageable memory: %.0f ms" % ((time.perf_counter() - t1) * 1e3))
        sample = plain[:a.sample_mib << 20].tobytes()
        z = {}
        for level in (1, 6):
            t1 = time.perf_counter()
            out = len(zlib.compress(sample, level))
            z[level] = (out / len(sample), time.perf_counter() - t1)
            say(lines, "zlib level %d on the first %d MiB, one thread: ratio %.4f, %.2f s (%.0f MB/s)"
                % (level, len(sample) >> 20, z[level][0], z[level][1], len(sample) / z[level][1] / 1e6))
        pieces = [sample[i:i + (4 << 20)] for i in range(0, len(sample), 4 << 20)]
        t1 = time.perf_counter()
        with ThreadPoolExecutor(16) as ex:
            out16 = sum(ex.map(lambda p: len(zlib.compress(p, 1)), pieces))
        t16 = time.perf_counter() - t1
        say(lines, "zlib level 1 on the same sample, 16 threads over 4 MiB pieces: ratio %.4f, %.2f s (%.0f MB/s); scaled to the "
            "text: %.1f s" % (out16 / len(sample), t16, len(sample) / t16 / 1e6, t16 * nbytes / len(sample)))
        say(lines, "ratio of the device coder (chunk_bytes %d) against zlib level 1: %.4f / %.4f = %.3f; against level 6: %.3f"
            % (default, results[default][1], z[1][0], results[default][1] / z[1][0], results[default][1] / z[6][0]))
        # the result of the default size inflates to the text
        t1 = time.perf_counter()
        gz, off = gs.download()
        t_dl = time.perf_counter() - t1
        d, pos, ok = zlib.decompressobj(31), 0, True
        view = memoryview(gz)
        members = 0
        for i in range(0, len(gz), 64 << 20):
            buf = view[i:i + (64 << 20)]
            while len(buf):
                out = d.decompress(buf)
                ok = ok and out == plain[pos:pos + len(out)].tobytes()
                pos += len(out)
                buf = d.unused_data
                if d.eof:
                    members += 1
                    d = zlib.decompressobj(31)
                elif len(buf):
                    break
        say(lines, "the members (%d) inflate to %d bytes that %s the text; download of the members to pageable memory %.0f ms"
            % (members, pos, "EQUAL" if ok and pos == len(plain) else "DIFFER FROM", t_dl * 1e3))
        del plain, gz
        targets = [os.devnull, os.devnull]
        path = None
        if a.write:
            path = os.path.join(a.write, "gzip_probe.%d.gz" % os.getpid())
            targets += [path, path]
        for stage, what, nb in ((gs, "members", info["bytes_out"]), (fo, "plain text", nbytes)):
            for target in targets:
                where = "/dev/null: the copy over PCIe alone" if target == os.devnull else "a file under " + a.write
                t1 = time.perf_counter()
                try:
                    wi = stage.write(target)
                except Exception as e:   # a full or read-only directory must not cost the measurements above
                    say(lines, "write(%s, %s) failed: %s" % (what, where, e))
                    continue
                wall = (time.perf_counter() - t1) * 1e3
                say(lines, "write(%s, %s): %.0f ms wall (ms_file %.0f), %.2f GB/s" % (what, where, wall, wi["ms_file"], nb / wall / 1e6))
        if path and os.path.exists(path):
            os.remove(path)
    rep = "\n".join(lines) + "\n"
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(rep)


if __name__ == "__main__":
    main()
