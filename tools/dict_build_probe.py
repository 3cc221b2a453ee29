"""Laps of the dictionary build under both values of opts.dict_build_mode: `python tools/dict_build_probe.py N [L]`.
Per mode two loads + builds of the same synthetic pool (bench.py's recipe); the second runs with opts.debug, so its
laps (host clock around a stream synchronise) go to stderr, and both print the HIP-event totals and stats."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import spring_amd  # noqa: E402


def main():
    n = int(sys.argv[1])
    L = int(sys.argv[2]) if len(sys.argv) > 2 else 150
    for mode in (1, 0):
        print("== dict_build_mode %d" % mode, flush=True)
        print("== dict_build_mode %d" % mode, file=sys.stderr, flush=True)
        for rep in (0, 1):
            with spring_amd.ReorderStage(spring_amd.ReorderOpts(dict_build_mode=mode, debug=rep == 1)) as s:
                s.load_synth(n, L, n * L // 25, 11, 10000)
                s.build_dict()
                st = s.stats()
            print("mode=%d rep=%d n=%d unpack=%.2f dict=%.2f path=%d keys=%d+%d dev=%.3fGB"
                  % (mode, rep, n, st["ms_unpack"], st["ms_dict"], st["dict_build_path"], st["numkeys"][0], st["numkeys"][1],
                     st["device_bytes"] / 1e9), flush=True)


if __name__ == "__main__":
    main()
