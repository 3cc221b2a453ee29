"""opts.strand_filter 0 against -1 on one pool in one process: `python tools/strand_filter_ab.py [reads] [readlen] [reps]`
(default: the headline pool, 100 M x 150 bp at 25x).  The first pass of either setting warms the block pool; the counts
must be identical whatever the setting."""
import os
import sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import spring_amd

n = int(sys.argv[1]) if len(sys.argv) > 1 else 100_000_000
L = int(sys.argv[2]) if len(sys.argv) > 2 else 150
reps = int(sys.argv[3]) if len(sys.argv) > 3 else 3
for rep in range(reps):
    for sf in (0, -1):
        with spring_amd.ReorderStage(spring_amd.ReorderOpts(device=0, num_thr=8, strand_filter=sf)) as s:
            s.load_synth(n, L, n * L // 25, 11, 10000)
            s.run()
            st = s.stats()
        print("rep %d strand_filter %2d: ran %d dropped %d  unpack %.2f dict %.2f chains %.2f finalize %.2f ms  rounds %d  n_matched %d n_single %d "
              "unmatched %d  device %.1f GB" % (rep, sf, st["strand_filter"], st["strand_filter_dropped"], st["ms_unpack"], st["ms_dict"],
                                                st["ms_chains"], st["ms_finalize"], st["rounds"], st["n_matched"], st["n_single"], st["unmatched"],
                                                st["device_bytes"] / 1e9), flush=True)
