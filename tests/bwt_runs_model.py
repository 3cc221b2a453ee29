"""The run-aware first keys of the block-sort stage (include/spring_bwt.h::spring_bwt_set_run_keys; DESIGN.md section
15) restated in numpy for one segment: the key, the hop, and the doubling rounds that follow them, plus the layout of
the key and the planner at 76 bytes a position (spring_amd/csrc/bwt_plan.h).  tests/test_bwt_runs_cpu.py holds the
ranks this gives to bwt_model.suffix_ranks."""
import numpy as np

MAX_SUB_SEGMENTS = 1 << 24
BYTES_PER_POS_RUNS, BYTES_PER_SEG = 76, 16


def run_key_layout(sub_segments):
    """bwt_plan.h::run_key_layout -> (seg_bits, key_bytes, run_bits, total_bits)."""
    seg_bits = (max(sub_segments, 1) - 1).bit_length()
    run_bits = 20 if (64 - 4 - 20 - seg_bits) // 8 >= 4 else 16
    key_bytes = min(4, (64 - 4 - run_bits - seg_bits) // 8)
    return seg_bits, key_bytes, run_bits, seg_bits + 8 * key_bytes + 4 + run_bits


def plan(lengths, budget, per_pos=BYTES_PER_POS_RUNS):
    """bwt_plan.h::plan_sub_batches with run keys on -> the first segment of every sub-batch, then the segment count."""
    first, s0, m = [], 0, 0
    for s, n in enumerate(lengths):
        assert n * per_pos + BYTES_PER_SEG <= budget
        if s > s0 and (m + n) * per_pos + (s + 1 - s0) * BYTES_PER_SEG > budget:
            first.append(s0)
            s0, m = s, 0
        m += n
    return (first + [s0] if lengths else []) + [len(lengths)]


def run_lengths(T):
    """L[i]: the positions from i to the end of i's run of equal bytes, i included."""
    n = len(T)
    last = np.ones(n, bool)
    last[:-1] = T[1:] != T[:-1]
    ends = np.flatnonzero(last)
    return ends[np.searchsorted(ends, np.arange(n))] - np.arange(n) + 1


def first_keys(T, k, R, cap_bits=0):
    """-> (key, hop) of every position of the segment T (uint8 array): next k bytes | valid | side | mag as one integer
    (the segment field left out), and the hop."""
    n = len(T)
    cap = (1 << (cap_bits or R)) - 1
    pad = np.concatenate([T.astype(np.int64), np.zeros(k, np.int64)])
    i = np.arange(n)
    valid = np.minimum(n - i, k)
    byts = np.zeros(n, np.int64)
    for j in range(k):
        byts = byts * 256 + np.where(j < valid, pad[i + j], 0)
    L = run_lengths(T)
    run = L >= k
    behind = i + L                                   # the byte behind the run, or n
    d = np.where(behind < n, pad[np.minimum(behind, n)], -1)
    side = (run & (d > T)).astype(np.int64)
    lc = np.minimum(L, cap)
    mag = np.where(run, np.where(side == 1, cap - lc, lc), 0)
    hop = np.where(run & (L < cap), L, 0)
    key = ((byts * 8 + valid) * 2 + side) * (1 << R) + mag
    return key, hop, int(run.sum())


def _regroup(key):
    """rank = the first slot of the group in the order of key (ties share it)."""
    order = np.argsort(key, kind="stable")
    ks = key[order]
    head = np.concatenate(([True], ks[1:] != ks[:-1]))
    first = np.maximum.accumulate(np.where(head, np.arange(len(key)), 0))
    rank = np.empty(len(key), np.int64)
    rank[order] = first
    return rank


def ranks(T, k, R, cap_bits=0, runs=True):
    """The rounds of bwt.hip on one segment -> (rank of every suffix, sort rounds, entries sorted per round).  runs
    False: the plain first key of k bytes."""
    T = np.frombuffer(bytes(T), np.uint8) if not isinstance(T, np.ndarray) else T
    n = len(T)
    if n == 0:
        return np.zeros(0, np.int64), 0, []
    if runs:
        key, hop, _ = first_keys(T, k, R, cap_bits)
    else:
        key, hop, _ = first_keys(T, k, 1, 1)
        hop = np.zeros(n, np.int64)
        key = key >> 2                               # side and mag shifted out: bytes | valid
    rank = _regroup(key)
    sizes = np.bincount(rank, minlength=n)
    rounds, entries, h = 1, [n], k
    while True:
        un = sizes[rank] > 1
        if not un.any():
            return rank, rounds, entries
        q = np.arange(n) + np.maximum(h, hop)
        nx = np.where(q < n, rank[np.minimum(q, n - 1)] + 1, 0)
        rank = _regroup(rank * (n + 2) + nx)         # the resolved positions keep their ranks: their groups are single
        sizes = np.bincount(rank, minlength=n)
        entries.append(int(un.sum()))
        rounds += 1
        h *= 2
        assert rounds <= n.bit_length() + 2, "more rounds than bwt_plan.h::max_rounds allows"


def quality_like_pool(seed=11, count=300, max_len=400):
    """Texts of 1 .. max_len - 1 bytes from six symbols (0x00 and 0xff among them) in runs of 1 .. 90."""
    rng = np.random.default_rng(seed)
    sym = np.array([0x00, 0x23, 0x2c, 0x46, 0x49, 0xff], np.uint8)
    lens = np.array([1, 2, 3, 5, 14, 15, 16, 17, 40, 90])
    out = []
    for _ in range(count):
        n = int(rng.integers(1, max_len))
        parts, have = [], 0
        while have < n:
            r = int(lens[rng.integers(0, len(lens))])
            parts.append(np.full(r, sym[rng.integers(0, 6)], np.uint8))
            have += r
        out.append(np.concatenate(parts)[:n].tobytes())
    return out
