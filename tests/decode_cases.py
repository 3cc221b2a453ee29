"""Hand-built encoder images for the decoder's tests (test infrastructure, not product): aligned reads at chosen
positions, with noise, in the slot order they are given, so that read_pos.bin gets the escapes asked for."""
import numpy as np

import streams_model as sm

_RC = str.maketrans("ACGTN", "TGCAN")
L_ESC = 24
SEQ_LEN = 400000


def _apply(seq, pos, L, rc, noise):
    r = list(seq[pos:pos + L])
    for p, ch in noise:
        r[p] = sm.DEC_NOISE[r[p]][ch]
    s = "".join(r)
    return s if rc == "d" else s.translate(_RC)[::-1]


def custom_case(positions, seed=0, with_noise=True, unaligned=()):
    """Single-end reads in slot order: aligned at `positions` (orientation and noise drawn from `seed`), then the
    `unaligned` reads.  -> (enc, seq, num_reads, reads in slot order)."""
    rng = np.random.default_rng(seed)
    seq = "".join("ACGT"[x] for x in rng.integers(0, 4, SEQ_LEN))
    pos = np.array(positions, np.uint64)
    rcs, lines, npos, reads = [], [], [], []
    for i, p in enumerate(positions):
        rc = "dr"[int(rng.integers(0, 2))]
        noise = []
        if with_noise and i % 3 != 1:
            at = sorted(set(int(x) for x in rng.integers(0, L_ESC, 1 + i % 3)))
            noise = [(a, int(rng.integers(0, 4))) for a in at]
        rcs.append(rc)
        lines.append("".join(str(c) for _, c in noise) + "\n")
        prev = 0
        for a, _ in noise:
            npos.append(a - prev)
            prev = a
        reads.append(_apply(seq, int(p), L_ESC, rc, noise))
    na = len(positions)
    enc = dict(pos=pos, rc="".join(rcs).encode(), noise="".join(lines).encode(), noisepos=np.array(npos, np.uint16),
               order=np.arange(na + len(unaligned), dtype=np.uint32),
               rlen=np.array([L_ESC] * na + [len(u) for u in unaligned], np.uint16),
               unaligned=sm._pack_dnaN(list(unaligned)))
    return enc, seq, na + len(unaligned), reads + list(unaligned)


def escape_cases():
    """name -> positions of read_pos.bin's adversarial corners."""
    down = [200000 - 7919 * i for i in range(25)]                          # every position decreases: all escape
    gaps = [100]
    for g in (65534, 65535, 65534, 65535, 0, 65533, 1):                   # u16 delta 65534, escape at 65535
        gaps.append(gaps[-1] + g)
    ffff = [65535, 131071, 196607, 65535, 131071, 131071 + 65534, 65535, 0, 196607]   # payloads with FF FF at even offsets
    return {"decreasing": down, "gaps": gaps, "ffff_payloads": ffff}


def writer_escapes(enc, num_reads, B):
    """65535 escapes the writer puts into read_pos.bin (single-end, not preserve_order)."""
    st = sm.write_streams(enc, num_reads, False, False, B)
    data, off = st["read_pos.bin"]
    n = 0
    for b in range(len(off) - 1):
        blk = data[int(off[b]):int(off[b + 1])]
        i = 8 if len(blk) else 0   # the block's first aligned read 1: u64
        while i < len(blk):
            if blk[i] == 0xFF and blk[i + 1] == 0xFF:
                n += 1
                i += 10
            else:
                i += 2
    return n
