"""A numpy model of the strand-symmetric presence table (spring_amd/csrc/strand_filter.h): the window
reverse complement, the canonical form, the flags a key sets, hash, bucket and fingerprint -- vectorised over uint64 arrays
and written independently of the header (tests/test_pres_model_cpu.py pins one to the other) -- the dictionary keys of a
pool cut from the reads on the host, and the properties a finished table must have whatever order its keys were entered in
(check_table), which is what the build's kernels are tested against (tests/test_gpu_presence_build.py)."""
import numpy as np

U64 = np.uint64


def mix64(x):
    x = np.asarray(x, dtype=U64).copy()
    with np.errstate(over="ignore"):
        x ^= x >> U64(33)
        x *= U64(0xff51afd7ed558ccd)
        x ^= x >> U64(33)
        x *= U64(0xc4ceb9fe1a85ec53)
        x ^= x >> U64(33)
    return x


def rc_window(w, wl):
    """Reverse complement of windows of wl bases, 2 bits a base, base 0 in bits 0-1; the complement of code c is 3 - c."""
    w = np.asarray(w, dtype=U64)
    out = np.zeros_like(w)
    for i in range(wl):
        out |= (U64(3) - ((w >> U64(2 * i)) & U64(3))) << U64(2 * (wl - 1 - i))
    return out


def canon_and_flags(w, wl, l):
    """-> (canon(W), the flags a key W of dictionary l adds to the slot of canon(W)): bit l where W is the canonical form,
    bit 2 + l where rc(W) is -- both for a palindrome."""
    w = np.asarray(w, dtype=U64)
    r = rc_window(w, wl)
    flags = np.where(w <= r, 1 << l, 0) | np.where(r <= w, 4 << l, 0)
    return np.minimum(w, r), flags.astype(np.uint32)


def bucket_of(h, lgb):
    h = np.asarray(h, dtype=U64)
    return (h >> U64(64 - lgb)) if lgb else np.zeros_like(h)


def fp_of(h):
    f = (np.asarray(h, dtype=U64) & U64(0x0fffffff)).astype(np.uint32)
    return np.where(f == 0, np.uint32(1), f)


def window_len(windows):
    (s0, _), (e0, _) = windows
    return e0 - s0 + 1


def dict_keys(read, ln, windows):
    """The unique keys of the two dictionaries of a pool: read = limbs [n, W] (2 bits a base, base 0 in bits 0-1 of limb 0),
    ln = lengths, windows = (starts, ends) of the two dictionary windows in bases.  A read is in dictionary l when it is
    longer than the window's last base; its key is the bases [start, end] of the read."""
    starts, ends = windows
    read = np.asarray(read, dtype=U64)
    out = []
    for s, e in zip(starts, ends):
        rows = read[np.asarray(ln) > e]
        bit, nb = 2 * s, 2 * (e - s + 1)
        li, off = bit >> 6, bit & 63
        v = rows[:, li] >> U64(off)
        if off and li + 1 < rows.shape[1]:
            v = v | (rows[:, li + 1] << U64(64 - off))
        if nb < 64:
            v = v & U64((1 << nb) - 1)
        out.append(np.unique(v))
    return out


def check_table(slots, lgb, keys, wl, dropped):
    """The contents of a finished table -- slots: [2^lgb, 4] slot words -- against the keys it was built from (keys[l]: the
    unique keys of dictionary l), and the build's drop count.  Holds for every order the keys may have been entered in."""
    slots = np.asarray(slots, dtype=np.uint32)
    assert slots.shape == (1 << lgb, 4)
    taken = slots != 0
    full = taken[:, 3]
    # slots fill in order: no empty slot precedes a taken one
    assert not np.any(~taken[:, :-1] & taken[:, 1:]), "an empty slot precedes a taken one"
    # no bucket holds one fingerprint twice
    fps = np.where(taken, slots >> 4, np.arange(4, dtype=np.uint32)[None, :] + np.uint32(1 << 28))  # (empty: four distinct stand-ins)
    srt = np.sort(fps, axis=1)
    assert not np.any(srt[:, 1:] == srt[:, :-1]), "a bucket holds one fingerprint twice"
    # what the keys ask for: (bucket, fingerprint) -> the OR of their flags
    code, flg = [], []
    for l in (0, 1):
        c, f = canon_and_flags(keys[l], wl, l)
        h = mix64(c)
        code.append((bucket_of(h, lgb) << U64(28)) | fp_of(h).astype(U64))
        flg.append(f)
    code, flg = np.concatenate(code), np.concatenate(flg)
    order = np.argsort(code, kind="stable")
    code, flg = code[order], flg[order]
    ucode, first = np.unique(code, return_index=True)
    uflags = np.bitwise_or.reduceat(flg, first) if len(code) else np.zeros(0, np.uint32)
    # the table's own (bucket, fingerprint) pairs
    bk, sl = np.nonzero(taken)
    tcode = (bk.astype(U64) << U64(28)) | (slots[bk, sl] >> 4).astype(U64)
    tflags = slots[bk, sl] & 15
    # every non-zero slot is explained by the keys of that (bucket, fingerprint), and its flags are exactly their OR
    at = np.searchsorted(ucode, tcode)
    assert np.all(at < len(ucode)) and np.array_equal(ucode[np.minimum(at, len(ucode) - 1)], tcode), "a slot no key explains"
    assert np.array_equal(uflags[at], tflags), "a slot's flags are not the OR of its keys' flags"
    # every key: its bucket is full, or a slot carries its fingerprint with its flag set (the check above: with every flag)
    held = np.isin(code, tcode)
    kb = (code >> U64(28)).astype(np.int64)
    assert np.all(held | full[kb]), "a key is missing from a bucket that is not full"
    # the drop count: the keys whose (bucket, fingerprint) the final table lacks
    assert int(dropped) == int((~held).sum()), (int(dropped), int((~held).sum()))
    return dict(keys=len(code), held=int(held.sum()), full_buckets=int(full.sum()), slots=int(taken.sum()))
