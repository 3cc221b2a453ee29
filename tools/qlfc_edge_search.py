#!/usr/bin/env python3
"""Finds the inputs of tests/qlfc_model.SEARCHED again: small texts on which the QLFC coder takes a branch that has to
be looked for, under one pair of state tables.  CPU only: it runs tests/qlfc_model.py, nothing else.

  qlfc_edge_search.py TABLES pend [--first S] [--count N] [--jobs J]
      seeds S .. S + N - 1 of _letters(3000, 9, seed): those whose range coder flushes a pending unit without a carry
      (n) or with one (c), with the segment's return value
  qlfc_edge_search.py TABLES eob [--first S] [--count N] [--jobs J]
      (n, k, seed) of _letters(n, k, seed), n = 1501 and 1502: first the alphabet sizes k whose margin at the last run,
      (n - 1 - 16) - bytes written, changes sign; then the seeds that give margin 0 (n odd) or 1 (n even)
  qlfc_edge_search.py TABLES lanes [--first S] [--count N]
      seeds of run_segment(63, seed, .) and run_segment(65, seed, .) in the second order of RUN_ORDERS whose last run's
      first event is event 63 and event 0 modulo 64 of its chunk (the number of events does not depend on the tables)
  qlfc_edge_search.py TABLES units [--first S] [--count N] [--jobs J]
      (n, seed) of _letters(n, 9, seed), n = 1000 .. 1063, whose payload holds a multiple of 64 units (last) or one
      more (first): the decoder's last unit is the last or the first of a 64-unit load (tests/unqlfc_model.UNIT_CASES)

TABLES is `real` (libbsc's tables out of oracle/_ref/libref_units.so) or the seed of qlfc_model.random_tables.  Every
line printed is a candidate; SEARCHED and RUN_SEEDS hold one of each kind."""
import argparse
import multiprocessing
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import qlfc_model as qm   # noqa: E402

TABLES = None


def _init(which):
    global TABLES
    TABLES = qm.state_tables() if which == "real" else qm.random_tables(int(which))
    if TABLES is None:
        raise SystemExit("the real tables need oracle/_ref/libref_units.so")


def _pend(seed):
    stats = {}
    _, rc = qm.compress(qm._letters(3000, 9, seed), TABLES, stats)
    return seed, rc, stats.get("pend", 0), stats.get("flush_nocarry", 0), stats.get("flush_carry", 0)


def _units(job):
    return job, len(qm.encode_chunk(qm._letters(job[0], 9, job[1]), job[0], TABLES, check=False)) // 2


def _margin(job):
    return job, qm.last_run_margin(qm._letters(*job), TABLES)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("tables")
    ap.add_argument("kind", choices=("pend", "eob", "lanes", "units"))
    ap.add_argument("--first", type=int, default=1000)
    ap.add_argument("--count", type=int, default=400)
    ap.add_argument("--jobs", type=int, default=4)
    args = ap.parse_args()
    seeds = range(args.first, args.first + args.count)
    if args.kind == "lanes":
        _init(args.tables)
        for j, count in enumerate(qm.RUN_ORDERS[1]):
            for seed in seeds if count in qm.RUN_SEEDS else ():
                stats = {}
                qm.encode_chunk(qm.run_segment(count, seed, 65 + 4 * j), 1 << 20, TABLES, stats)
                if stats["lastev"][0] % 64 == (63 if count == 63 else 0):
                    print("lanes: %d runs, seed %d, lastev %d" % (count, seed, stats["lastev"][0]), flush=True)
        return
    with multiprocessing.Pool(args.jobs, _init, (args.tables,)) as pool:
        if args.kind == "units":
            for job, units in pool.imap(_units, [(n, s) for s in seeds for n in range(1000, 1064)], 8):
                if units % 64 < 2:
                    print("units_%s (n, seed) = %r units %d" % ("first" if units % 64 else "last", job, units), flush=True)
            return
        if args.kind == "pend":
            for seed, rc, pend, nocarry, carry in pool.imap(_pend, seeds, 8):
                if nocarry or carry:
                    print("pend_%s seed %d rc %d pend %d flush_nocarry %d flush_carry %d"
                          % ("c" if carry else "n", seed, rc, pend, nocarry, carry), flush=True)
            return
        for n, want in ((1501, 0), (1502, 1)):
            probe = dict(pool.imap(_margin, [(n, k, args.first) for k in range(40, 121, 4)]))
            ks = sorted(k for (_, k, _), m in probe.items() if abs(m - want) <= 40)
            print("n %d: margins by alphabet size %s" % (n, {k: m for (_, k, _), m in sorted(probe.items())}), flush=True)
            ks = range(min(ks) - 2, max(ks) + 3) if ks else range(60, 81)
            for job, m in pool.imap(_margin, [(n, k, s) for s in seeds for k in ks], 8):
                if m == want:
                    print("eob_%d (n, k, seed) = %r margin %d" % (want, job, m), flush=True)


if __name__ == "__main__":
    main()
