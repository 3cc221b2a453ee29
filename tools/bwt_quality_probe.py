"""Measurement of the block sort on quality text ("Run-aware first keys"): the quality blocks of
a synthetic single-end FASTQ (tools/qualid_probe.make_text), left in HBM by QualIdStage in file order, 256 000 reads a
block, then BwtStage.transform over them at the 64 MiB cut SPRING passes, with run keys off and on.

  python tools/bwt_quality_probe.py [n_reads] [read_len] [--reps R] [--threads T] [--out FILE]

Three contents:
  raw        make_text's qualities: every byte uniform in 33 .. 73, independent
  illumina   the same under the Illumina 8-level table (QualIdStage.quality_table("illumina"))
  four-level the generator below: few symbols, long runs, '#' tails

four_level(u, L, seed): a stream of u * L bytes is np.repeat(symbols, lengths) with symbols drawn uniformly from
"F:,#" and lengths uniformly from (1, 2, 3, 5, 8, 13, 21, 34, 55, 89), numpy default_rng(seed); it is cut into u lines
of L bytes, so runs cross line ends; then every fourth line (line % 4 == 3) gets a tail of '#' over its last
1 + (line * 7919) % 100 bytes.  As in make_text, the lines of 2^20 records are tiled over the file.

One warm-up lap, then R laps per case: ms_device as median with min - max, the passes, rounds, the entries every round
sorted and run_positions.  Beside them the real bsc_bwt_encode of oracle/_ref/libref_units.so over the same segments,
one block per thread on T threads, its output compared with the device's.  Without oracle/_ref the CPU column is left
out."""
import argparse
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np  # noqa: E402

from bwt_probe import PASSES, ref_bwt, ref_lib, say, stats  # noqa: E402
from qualid_probe import make_text  # noqa: E402

CUT = 64 << 20
RUN_LENGTHS = (1, 2, 3, 5, 8, 13, 21, 34, 55, 89)


def four_level(u, L, seed=4):
    rng = np.random.default_rng(seed)
    need = u * L
    k = need // 8 + 16   # the mean run is 23.1 bytes: far more runs than the stream takes
    sym = np.frombuffer(b"F:,#", np.uint8)[rng.integers(0, 4, k)]
    ln = np.array(RUN_LENGTHS)[rng.integers(0, len(RUN_LENGTHS), k)]
    a = np.repeat(sym, ln)[:need].reshape(u, L).copy()
    assert a.size == need
    lines = np.arange(3, u, 4)
    tail = 1 + (lines * 7919) % 100
    col = np.arange(L)[None, :]
    a[lines] = np.where(col >= L - np.minimum(tail, L)[:, None], ord("#"), a[lines])
    return a


def with_qualities(text, rec, n, L, unit=1 << 20):
    """make_text's text with the quality lines replaced by four_level's, tiled as make_text tiles."""
    u = min(n, unit)
    q = four_level(u, L)
    t = text.reshape(n, rec).copy()
    t[:, 14 + L:14 + 2 * L] = np.tile(q, ((n + u - 1) // u, 1))[:n]
    return t.reshape(-1)


def keep(lines, out):
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as f:
            f.write("\n".join(lines) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("n", type=int, nargs="?", default=4_000_000)
    ap.add_argument("L", type=int, nargs="?", default=150)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from spring_amd import BwtStage, QualIdStage
    lines = []
    n, L, B = a.n, a.L, 256000
    U = ref_lib()
    text, rec = make_text(n, L)
    say(lines, "bwt_quality_probe: single-end %d x %d bp, file order, %d reads per block, cut at 64 MiB" % (n, L, B))
    if U is None:
        say(lines, "oracle/_ref/libref_units.so is not built: no CPU column")
    summary = []
    for name, fq, table in (("raw", text, None), ("illumina", text, QualIdStage.quality_table("illumina")),
                            ("four-level", None, None)):
        if fq is None:
            fq = with_qualities(text, rec, n, L)
        with QualIdStage() as qs, BwtStage() as bw:
            qs.set_order(None, n)
            qi = qs.from_fastq(fq, want="quality", table=table, num_reads_per_block=B)
            say(lines, "")
            say(lines, "%s: %d blocks, %.3f GB of quality text" % (name, qi["num_blocks"], qi["bytes"][0] / 1e9))
            med = {}
            for on in (False, True):
                bw.set_run_keys(on)
                runs = []
                for it in range(a.reps + 1):
                    info = bw.transform(qs, kind="quality", block_bytes=0)
                    if it:
                        runs.append(info)
                m, lo, hi = stats([r["ms_device"] for r in runs])
                med[on] = m
                say(lines, "  run keys %-3s %d segments, longest %d bytes, %d sub-batches: ms_device median %.1f  min %.1f  max %.1f "
                    "(%d reps); %.1f MB/s; rounds %d (%d summed); run_positions %d"
                    % ("on:" if on else "off:", info["num_segments"], info["max_segment"], info["sub_batches"], m, lo, hi, len(runs),
                       info["bytes"] / m / 1e3, info["rounds"], info["rounds_total"], info["run_positions"]))
                say(lines, "      " + "  ".join("%s %.1f" % (p, stats([r["ms_pass"][k] for r in runs])[0]) for k, p in enumerate(PASSES)))
                say(lines, "      entries sorted per round: " + " ".join(str(int(x)) for x in bw.round_entries()))
                res = bw.download() if on else None
            summary.append((name, med[False], med[True]))
            keep(lines, a.out)
            if U is None:
                continue
            data, _, off = qs.download("quality")
        segs = []
        for b in range(len(off) - 1):
            for x in range(int(off[b]), int(off[b + 1]), CUT):
                segs.append(data[x:min(x + CUT, int(off[b + 1]))])
        t0 = time.perf_counter()
        with ThreadPoolExecutor(a.threads) as ex:
            ref = list(ex.map(lambda s: ref_bwt(U, s), segs))
        t_cpu = time.perf_counter() - t0
        so = res["seg_off"]
        same = all(res["bwt"][int(so[j]):int(so[j + 1])] == r[0] and res["primary"][j] == r[1]
                   and np.array_equal(res["indexes"][j][:res["num_indexes"][j]], r[2]) for j, r in enumerate(ref))
        say(lines, "  bsc_bwt_encode (features FASTMODE) over the same %d segments, one block per thread on %d threads: %.2f s wall, "
            "%.1f MB/s; bytes, primary index and indexes of every segment %s the device's (run keys on); CPU / device: off %.1fx, on %.1fx"
            % (len(segs), a.threads, t_cpu, sum(map(len, segs)) / t_cpu / 1e6, "EQUAL" if same else "DIFFER FROM",
               t_cpu * 1e3 / med[False], t_cpu * 1e3 / med[True]))
    say(lines, "")
    for name, off_ms, on_ms in summary:
        say(lines, "%-10s run keys off %9.1f ms, on %9.1f ms: %s by %.2fx" % (name, off_ms, on_ms, "on wins" if on_ms < off_ms else "off wins",
                                                                          max(off_ms, on_ms) / min(off_ms, on_ms)))
    keep(lines, a.out)


if __name__ == "__main__":
    main()
