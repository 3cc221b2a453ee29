"""Measurement of the BSC framing stage: BscStage.frame over a StreamsStage and a QualIdStage,
which runs the block sort and the QLFC coder on the way, so one lap gives the three stages' times on the same batch.

  python tools/bsc_probe.py [n_reads] [read_len] [--quality-reads Q] [--reps R] [--threads T] [--skip LIST] [--out FILE]

Two inputs, as tools/qlfc_probe.py builds them:
  streams   the nine per-block read streams of a synthetic single-end run of n_reads, 25 MiB cut -> BSC files
  quality   the quality blocks of Q reads (four-level, illumina), 64 MiB cut, run keys off -> string-array files

For each: one warm-up lap, then R laps (R = 0: one lap, no warm-up): the framing's ms_device and passes as median with
min - max, beside the sort's and the coder's ms_device of the same laps; files, blocks, outcomes, bytes.  Then the
host route the stage replaces, on the same machine: the download of the uncompressed inputs (and of what the two inner
contexts hold), then zlib.adler32 of every input and body, the headers and the copies into files on T threads (one
block per task; tests/bsc_frame_model.py).  The host's files are compared with the device's.  The state tables are
read out of oracle/_ref/libref_units.so; without it there is nothing to run."""
import argparse
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tools"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

import bsc_frame_model as fm  # noqa: E402
import qlfc_model as qm  # noqa: E402
from bwt_probe import say, stats  # noqa: E402
from bwt_quality_probe import keep, with_qualities  # noqa: E402
from qualid_probe import make_text  # noqa: E402

PASSES = ("sums", "plan", "assembly")


def measure(lines, a, name, src, bw, ql, bs, inputs, framing, **kw):
    """inputs(): downloads the uncompressed input and returns per file the list of its cuts' bytes."""
    laps = []
    for it in range(a.reps + 1):
        info = bs.frame(bw, ql, src, **kw)
        if it or not a.reps:
            laps.append((info, bw.info, ql.info))
    m, lo, hi = stats([x[0]["ms_device"] for x in laps])
    sort_ms, coder_ms = stats([x[1]["ms_device"] for x in laps])[0], stats([x[2]["ms_device"] for x in laps])[0]
    say(lines, "%s: %d files, %d blocks, %.3f GB in, %.3f GB out; coded %d, stored: small %d, coder %d, no gain %d"
        % (name, info["num_files"], info["num_blocks"], info["bytes_in"] / 1e9, info["bytes_out"] / 1e9, info["coded"],
           info["stored_small"], info["stored_coder"], info["stored_no_gain"]))
    say(lines, "  framing ms_device median %.2f  min %.2f  max %.2f  (%d reps); %.1f GB/s of input"
        % (m, lo, hi, len(laps), info["bytes_in"] / m / 1e6))
    say(lines, "  " + "  ".join("%s %.2f" % (p, stats([x[0]["ms_pass"][k] for x in laps])[0]) for k, p in enumerate(PASSES)))
    say(lines, "  the same laps: block sort ms_device %.1f, QLFC coder ms_device %.1f; framing / sort = %.4f, framing / (sort + coder) = %.5f"
        % (sort_ms, coder_ms, m / sort_ms, m / (sort_ms + coder_ms)))
    keep(lines, a.out)
    t0 = time.perf_counter()
    files = bs.files()
    t_files = time.perf_counter() - t0
    t0 = time.perf_counter()
    cuts = inputs()
    t_in = time.perf_counter() - t0
    t0 = time.perf_counter()
    res, coded = bw.download(), ql.segments()
    t_parts = time.perf_counter() - t0
    flat = [c for f in cuts for c in f]
    parts = [(int(res["primary"][j]), res["indexes"][j][:int(res["num_indexes"][j])], coded[j][0], coded[j][1]) for j in range(len(flat))]
    t0 = time.perf_counter()
    with ThreadPoolExecutor(a.threads) as ex:
        blocks = list(ex.map(lambda sp: fm.block(sp[0], *sp[1])[0], zip(flat, parts)))
    host, j = [], 0
    for f in cuts:
        at, fb = 0, []
        for c in f:
            fb.append((at, blocks[j]))
            at += len(c)
            j += 1
        host.append(fm.frame(framing, fb))
    t_host = time.perf_counter() - t0
    same = [x[3] for x in files] == host
    say(lines, "  host route on %d threads: download of the %.3f GB of input %.1f ms (%.1f GB/s), of the sort's and the coder's results "
        "%.1f ms; sums, headers and copies %.1f ms: %.1f ms in all; its files %s the device's.  Download of the device's files: %.1f ms"
        % (a.threads, sum(map(len, flat)) / 1e9, t_in * 1e3, sum(map(len, flat)) / t_in / 1e9, t_parts * 1e3, t_host * 1e3,
           (t_in + t_parts + t_host) * 1e3, "EQUAL" if same else "DIFFER FROM", t_files * 1e3))
    say(lines, "  host route / (framing + download of the files) = %.1fx" % ((t_in + t_parts + t_host) * 1e3 / (m + t_files * 1e3)))
    keep(lines, a.out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("n", type=int, nargs="?", default=20_000_000)
    ap.add_argument("L", type=int, nargs="?", default=150)
    ap.add_argument("--quality-reads", type=int, default=4_000_000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--skip", default="", help="comma list of inputs to leave out: streams, illumina, four-level")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import spring_amd
    from spring_amd import BscStage, BwtStage, QlfcStage, QualIdStage, _lib
    from spring_amd.encoder import EncoderStage
    from spring_amd.streams import StreamsStage
    tables = qm.state_tables()
    assert tables is not None, "oracle/_ref/libref_units.so is not built"
    skip = set(a.skip.split(","))
    lines = []
    n, L, B = a.n, a.L, 256000
    if "streams" not in skip:
        with spring_amd.ReorderStage(spring_amd.ReorderOpts(num_chains=0, num_thr=8)) as st:
            st.load_synth(n, L, n * L // 50, 7, 10000)
            st.run()
            say(lines, "bsc_probe: single-end %d x %d bp, %d reads per block, all nine streams, 25 MiB cut" % (n, L, B))
            with EncoderStage() as enc, StreamsStage() as ss, BwtStage() as bw, QlfcStage() as ql, BscStage() as bs:
                ql.set_state_tables(*tables)
                enc.encode(st)
                ss.from_encoder(enc, n, False, False, B)

                def inputs():
                    out = []
                    for s in range(_lib.STREAMS_NUM):
                        for blk in ss.blocks(s):
                            out.append([blk[lo:hi] for lo, hi in fm.cuts(len(blk), 25 << 20)])
                    return out
                measure(lines, a, "streams", ss, bw, ql, bs, inputs, fm.BSC_FILE)
    n = a.quality_reads
    if skip >= {"illumina", "four-level"}:
        n = 0
    text, rec = make_text(n, L) if n else (None, 0)
    if n:
        say(lines, "")
        say(lines, "quality: single-end %d x %d bp, file order, %d reads per block, cut at 64 MiB, run keys off" % (n, L, B))
    for name, fq, table in (("four-level", None, None), ("illumina", text, QualIdStage.quality_table("illumina"))):
        if name in skip or not n:
            continue
        if fq is None:
            fq = with_qualities(text, rec, n, L)
        _lib.lib().spring_reorder_trim_pool()   # the budgets come from the free HBM: give the last content's blocks back
        with QualIdStage() as qs, BwtStage() as bw, QlfcStage() as ql, BscStage() as bs:
            ql.set_state_tables(*tables)
            qs.set_order(None, n)
            qs.from_fastq(fq, want="quality", table=table, num_reads_per_block=B)

            def inputs():
                data, _, off = qs.download("quality")
                return [[data[int(off[b]):int(off[b + 1])][lo:hi] for lo, hi in fm.cuts(int(off[b + 1] - off[b]), 64 << 20)]
                        for b in range(len(off) - 1)]
            measure(lines, a, name, qs, bw, ql, bs, inputs, fm.STR_ARRAY, kind="quality", block_bytes=0)
    keep(lines, a.out)


if __name__ == "__main__":
    main()
