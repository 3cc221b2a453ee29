"""Plain-Python model of SPRING's id codec (reference src/id_compression/: compress_id's tokens, the adaptive
models of stream_model.cpp / sam_models.cpp and the 26-bit arithmetic coder of Arithmetic_stream.cpp), written from
the format as DESIGN.md section 17 states it.  The checker's own code: it does not touch the library.

  tokenize(cur, prev)    -> (symbols, token starts of cur); a symbol is (kind, context, value)
  block_symbols(ids)     -> the symbol words of one block (value | kind << 8 | context << 11)
  encode_symbols(words)  -> the bytes compress_id_block writes for them
  compress_block(ids)    -> encode_symbols(block_symbols(ids))
"""

K_TYPE, K_ALEN, K_ABYTE, K_CHAR, K_DELTA, K_ZEROS, K_INT = range(7)
ALPHA, DIGIT, CHAR, MATCH, ZEROS, DELTA, END = range(7)
ALPHABET = (10, 256, 256, 256, 256, 256, 256)
MAX_ID = 1023
NUM_LIMIT = 1 << 28
WORD_BITS = 26


def _alpha(b):
    return 65 <= b <= 90 or 97 <= b <= 122


def _digit(b):
    return 48 <= b <= 57


def check_id(cur):
    """What the stage refuses (the reference is undefined or lossy there)."""
    if len(cur) > MAX_ID:
        raise ValueError("id longer than %d bytes" % MAX_ID)
    if any(b == 0 or b >= 128 for b in cur):
        raise ValueError("id byte 0 or >= 128")


def tokenize(cur, prev, prev_starts):
    """cur, prev: bytes; prev_starts: the token starts of prev.  -> (symbols, token starts of cur)."""
    check_id(cur)
    plen = len(prev)

    def pb(i):
        return prev[i] if i < plen else 0

    out, starts = [], []
    c, t, n = 0, 0, len(cur)
    while c < n:
        p = prev_starts[t] if t < len(prev_starts) else 0
        b = cur[c]
        e = c + 1
        if _alpha(b):
            while e < n and _alpha(cur[e]):
                e += 1
            ln = e - c
            if ln > 255:
                raise ValueError("letter run longer than 255")
            if all(cur[c + k] == pb(p + k) for k in range(ln)) and not _alpha(pb(p + ln)):
                out.append((K_TYPE, t, MATCH))
            else:
                out.append((K_TYPE, t, ALPHA))
                out.append((K_ALEN, t, ln))
                out.extend((K_ABYTE, t, cur[c + k]) for k in range(ln))
        elif b == 48:
            while e < n and cur[e] == 48:
                e += 1
            ln = e - c
            if ln > 255:
                raise ValueError("zero run longer than 255")
            if all(pb(p + k) == 48 for k in range(ln)) and pb(p + ln) != 48:
                out.append((K_TYPE, t, MATCH))
            else:
                out.append((K_TYPE, t, ZEROS))
                out.append((K_ZEROS, t, ln))
        elif _digit(b):
            v = b - 48
            while e < n and _digit(cur[e]) and v < NUM_LIMIT:
                v = v * 10 + cur[e] - 48
                e += 1
            ln = e - c
            is_num, pv = True, 0
            if plen:
                is_num = _digit(pb(p)) and pb(p) != 48
                if is_num:
                    pv, k = pb(p) - 48, 1
                    while _digit(pb(p + k)) and pv < NUM_LIMIT:
                        pv = pv * 10 + pb(p + k) - 48
                        k += 1
            d = (v - pv) & 0xffffffff
            if d >= 1 << 31:
                d -= 1 << 32
            if is_num and all(cur[c + k] == pb(p + k) for k in range(ln)) and not _digit(pb(p + ln)):
                out.append((K_TYPE, t, MATCH))
            elif is_num and 0 < d < 256:
                out.append((K_TYPE, t, DELTA))
                out.append((K_DELTA, t, d))
            else:
                out.append((K_TYPE, t, DIGIT))
                out.extend((K_INT, 4 * t + k, (v >> (8 * k)) & 0xff) for k in range(4))
        else:
            if b == pb(p):
                out.append((K_TYPE, t, MATCH))
            else:
                out.append((K_TYPE, t, CHAR))
                out.append((K_CHAR, t, b))
        starts.append(c)
        c = e
        t += 1
    out.append((K_TYPE, t, END))
    return out, starts


def word(kind, ctx, value):
    return value | (kind << 8) | (ctx << 11)


def block_symbols(ids):
    """The symbol words of one block, and its largest token count."""
    words, prev, prev_starts, max_tokens = [], b"", [], 0
    for cur in ids:
        sym, starts = tokenize(cur, prev, prev_starts)
        words.extend(word(*s) for s in sym)
        prev, prev_starts = cur, starts
        max_tokens = max(max_tokens, len(starts))
    return words, max_tokens


class _Bits:
    def __init__(self):
        self.out = bytearray()
        self.acc = 0
        self.n = 0

    def put(self, bit):
        self.acc = (self.acc << 1) | (bit & 1)
        self.n += 1
        if self.n == 8:
            self.out.append(self.acc)
            self.acc = 0
            self.n = 0

    def finish(self):   # the byte in progress, padded with zeros, is always written
        self.out.append((self.acc << (8 - self.n)) & 0xff)
        return bytes(self.out)


def encode_symbols(words):
    models = {}
    top, half, quarter = (1 << WORD_BITS) - 1, 1 << (WORD_BITS - 1), 1 << (WORD_BITS - 2)
    low, up, pending = 0, top, 0
    bits = _Bits()
    for w in words:
        x, kind, ctx = w & 0xff, (w >> 8) & 7, (w >> 11) & 0xfff
        m = models.get((kind, ctx))
        if m is None:
            m = models[(kind, ctx)] = [[1] * ALPHABET[kind], ALPHABET[kind]]
        counts, n = m
        cum = sum(counts[:x])
        rng = up - low + 1
        up = low + rng * (cum + counts[x]) // n - 1
        low = low + rng * cum // n
        while True:
            if (low >= half) == (up >= half):
                bit = 1 if low >= half else 0
                bits.put(bit)
                while pending:
                    bits.put(1 - bit)
                    pending -= 1
                low = (low & (half - 1)) << 1
                up = ((up & (half - 1)) << 1) + 1
            elif low >= quarter and up < half + quarter:
                pending += 1
                low = (low << 1) & (half - 1)
                up = (((up << 1) & (half - 1)) | half) + 1
            else:
                break
        counts[x] += 10
        n += 10
        if n >= 1 << 20:
            for i in range(len(counts)):
                counts[i] = (counts[i] >> 1) + 1
            n = sum(counts)
        m[1] = n
    bit = 1 if low >= half else 0
    bits.put(bit)
    while pending:
        bits.put(1 - bit)
        pending -= 1
    for k in range(WORD_BITS - 2, -1, -1):
        bits.put(low >> k)
    return bits.finish()


def compress_block(ids):
    return encode_symbols(block_symbols(ids)[0])


def compress_blocks(ids, B):
    """ids in slot order -> the bytes of id_N.<b> for every block of B ids."""
    return [compress_block(ids[i:i + B]) for i in range(0, len(ids), B)]
