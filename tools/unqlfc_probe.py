"""Measurement of the QLFC decoder stage: UnqlfcStage.decode over the coded segments a QlfcStage
leaves in HBM.

  python tools/unqlfc_probe.py [n_reads] [read_len] [--quality-reads Q] [--reps R] [--threads T] [--skip LIST] [--out FILE]

The inputs are those of tools/qlfc_probe.py (profiles/qlfc_20Mx150.txt): the nine per-block read streams of a synthetic
single-end run, block-sorted at the 25 MiB cut, and the quality blocks of Q reads in three contents (four-level,
illumina, raw), block-sorted at the 64 MiB cut with run keys off.  Each is coded once by QlfcStage.

For each: one warm-up lap, then R laps of UnqlfcStage.decode(qlfc stage): ms_device and every pass as median with
min - max, chunks, runs, events, ns per event of the longest chunk's share, sub-batches.  Every decoded segment is
compared with the block-sorted segment that was coded.  Beside them the real bsc_coder_decompress of
oracle/_ref/libref_units.so over the same coded segments, one segment per thread on T threads.  The state tables are read
out of that library (tests/qlfc_model.state_tables); without oracle/_ref there is nothing to run."""
import argparse
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tools"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

import qlfc_model as qm  # noqa: E402
from bwt_probe import say, stats  # noqa: E402
from bwt_quality_probe import keep, with_qualities  # noqa: E402
from qualid_probe import make_text  # noqa: E402

PASSES = ("plan", "decode", "raw copies")


def measure(lines, a, name, bw, ql, uq, out):
    """Codes what bw holds, then the laps of the decoder over the result ql holds, then the CPU column."""
    cinfo = ql.code(bw)
    runs = []
    for it in range(a.reps + 1):
        info = uq.decode(ql)
        if it or not a.reps:   # --reps 0: the first lap is the measurement
            runs.append(info)
    m, lo, hi = stats([r["ms_device"] for r in runs])
    say(lines, "%s: %d segments, %.3f GB coded, %.3f GB decoded, %d sub-batches (workspace budget %.1f GB); %d chunks (%d raw), "
        "%d runs, %d events = %.2f per decoded byte; %d segments skipped (the coder's not compressible: %d)"
        % (name, info["num_segments"], info["bytes_in"] / 1e9, info["bytes_out"] / 1e9, info["sub_batches"],
           info["workspace_bytes"] / 1e9, info["chunks"], info["chunks_raw"], info["runs"], info["events"],
           info["events"] / max(info["bytes_out"], 1), info["skipped"], cinfo["not_compressible"]))
    say(lines, "  ms_device median %.1f  min %.1f  max %.1f  (%d reps); %.1f MB/s of decoded bytes; %.1f ns per event with %d walks side by side"
        % (m, lo, hi, len(runs), info["bytes_out"] / m / 1e3, m * 1e6 / max(info["events"], 1) * (info["chunks"] - info["chunks_raw"]),
           info["chunks"] - info["chunks_raw"]))
    say(lines, "  " + "  ".join("%s %.1f" % (p, stats([r["ms_pass"][k] for r in runs])[0]) for k, p in enumerate(PASSES)))
    keep(lines, out)
    got = uq.segments()
    coded = ql.segments()
    res = bw.download()
    off = res["seg_off"]
    segs = [res["bwt"][int(off[j]):int(off[j + 1])] for j in range(len(off) - 1)]
    same = all(g == (s if rc > 0 else b"") for g, s, (_, rc) in zip(got, segs, coded))
    say(lines, "  every decoded segment %s the block-sorted segment that was coded" % ("EQUALS" if same else "DIFFERS FROM"))
    jobs = [(c, len(s)) for s, (c, rc) in zip(segs, coded) if rc > 0]
    t0 = time.perf_counter()
    with ThreadPoolExecutor(a.threads) as ex:
        ref = list(ex.map(lambda j: qm.ref_decompress(*j), jobs))
    t_cpu = time.perf_counter() - t0
    same = all(r[0] == s for r, s in zip(ref, [s for s, (_, rc) in zip(segs, coded) if rc > 0]))
    say(lines, "  bsc_coder_decompress (QLFC static, features 3) over the same %d coded segments, one segment per thread on %d threads: "
        "%.2f s wall, %.1f MB/s; every segment %s the input; device / CPU: %.2fx"
        % (len(jobs), a.threads, t_cpu, sum(n for _, n in jobs) / t_cpu / 1e6, "EQUALS" if same else "DIFFERS FROM", m / (t_cpu * 1e3)))
    keep(lines, out)
    return m, t_cpu * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("n", type=int, nargs="?", default=20_000_000)
    ap.add_argument("L", type=int, nargs="?", default=150)
    ap.add_argument("--quality-reads", type=int, default=4_000_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--skip", default="", help="comma list of inputs to leave out: streams, raw, illumina, four-level")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import spring_amd
    from spring_amd import BwtStage, QlfcStage, QualIdStage, UnqlfcStage, _lib
    from spring_amd.encoder import EncoderStage
    from spring_amd.streams import StreamsStage
    tables = qm.state_tables()
    assert tables is not None and qm.ref_lib() is not None, "oracle/_ref/libref_units.so is not built"
    skip = set(a.skip.split(","))
    lines, summary = [], []
    n, L, B = a.n, a.L, 256000
    if "streams" not in skip:
        with spring_amd.ReorderStage(spring_amd.ReorderOpts(num_chains=0, num_thr=8)) as st:
            st.load_synth(n, L, n * L // 50, 7, 10000)
            st.run()
            say(lines, "unqlfc_probe: single-end %d x %d bp, %d reads per block, all nine streams, 25 MiB cut" % (n, L, B))
            with EncoderStage() as enc, StreamsStage() as ss, BwtStage() as bw, QlfcStage() as ql, UnqlfcStage() as uq:
                ql.set_state_tables(*tables)
                uq.set_state_tables(*tables)
                enc.encode(st)
                ss.from_encoder(enc, n, False, False, B)
                bw.transform(ss)
                summary.append(("streams",) + measure(lines, a, "streams", bw, ql, uq, a.out))
    n = a.quality_reads
    if skip >= {"raw", "illumina", "four-level"}:
        n = 0
    text, rec = make_text(n, L) if n else (None, 0)
    if n:
        say(lines, "")
    say(lines, "quality: single-end %d x %d bp, file order, %d reads per block, cut at 64 MiB, run keys off" % (n, L, B))
    for name, fq, table in (("four-level", None, None), ("illumina", text, QualIdStage.quality_table("illumina")), ("raw", text, None)):
        if name in skip or not n:
            continue
        if fq is None:
            fq = with_qualities(text, rec, n, L)
        _lib.lib().spring_reorder_trim_pool()   # the budgets come from the free HBM: give the last content's blocks back
        with QualIdStage() as qs, BwtStage() as bw, QlfcStage() as ql, UnqlfcStage() as uq:
            ql.set_state_tables(*tables)
            uq.set_state_tables(*tables)
            qs.set_order(None, n)
            qs.from_fastq(fq, want="quality", table=table, num_reads_per_block=B)
            bw.transform(qs, kind="quality", block_bytes=0)
            summary.append((name,) + measure(lines, a, name, bw, ql, uq, a.out))
    say(lines, "")
    for name, dev, cpu in summary:
        say(lines, "%-10s device %9.1f ms, %d CPU threads %9.1f ms: %s by %.2fx"
            % (name, dev, a.threads, cpu, "the device wins" if dev < cpu else "the CPU wins", max(dev, cpu) / min(dev, cpu)))
    keep(lines, a.out)


if __name__ == "__main__":
    main()
