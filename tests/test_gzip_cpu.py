"""CPU-only checks of the gzip stage's host side: the ctypes mirror of spring_gzip_info against the C header, the
exported symbols, and the sequential parts of the coder (spring_amd/csrc/gzip_codes.h, shared by host and device) in a
host build: the length / distance tables against RFC 1951, the length limiter, the CRC-32 arithmetic against zlib."""
import ctypes as C
import os
import re
import subprocess
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LEN_EXTRA = [0] * 8 + [1] * 4 + [2] * 4 + [3] * 4 + [4] * 4 + [5] * 4 + [0]
DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097,
             6145, 8193, 12289, 16385, 24577]
DIST_EXTRA = [0, 0, 0, 0] + [e for e in range(1, 14) for _ in (0, 1)]


def test_ctypes_mirror_matches_the_c_header(tmp_path):
    from spring_amd import _lib
    fields = [k for k, _ in _lib.GzipInfo._fields_]
    src = tmp_path / "abi.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "spring_gzip.h"\nint main(void) {\n'
                   '  printf("%zu", sizeof(spring_gzip_info));\n'
                   + "".join('  printf(" %%zu", offsetof(spring_gzip_info, %s));\n' % k for k in fields)
                   + "  return 0; }\n")
    exe = tmp_path / "abi"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    want = [C.sizeof(_lib.GzipInfo)] + [getattr(_lib.GzipInfo, k).offset for k in fields]
    assert got == want, (got, want)


def test_library_exports_every_declared_symbol():
    from spring_amd import _lib
    import spring_amd
    hdr = open(os.path.join(ROOT, "include", "spring_gzip.h")).read()
    declared = set(re.findall(r"\b(spring_gzip_\w+)\s*\(", hdr))
    assert declared == set(_lib.GZIP_EXPORTS)
    L = _lib.lib()
    for name in sorted(declared):
        assert hasattr(L, name), "libspring_reorder_hip.so does not export " + name
    assert spring_amd.GzipStage is not None


HARNESS = r"""
#include <cstdio>
#include <cstdlib>
#include "gzip_codes.h"
int main(int argc, char **argv) {
  for (int len = 3; len <= 258; len++) { int e, v; int s = gz::len_symbol(len, &e, &v); printf("L %d %d %d %d %d\n", len, s, e, v, gz::len_ebits(s)); }
  for (int d = 1; d <= 32768; d++) { int e, v; int s = gz::dist_symbol(d, &e, &v); printf("D %d %d %d %d %d\n", d, s, e, v, gz::dist_ebits(s)); }
  static gz::CodeWork w;
  for (int c = 0; c < 4; c++) {   // Fibonacci counts over 24 of 286 symbols (a chunk holds at most 65536), over 19, two symbols, flat 286
    static uint32_t f[gz::NUM_LL]; static uint8_t len[gz::NUM_LL]; static uint16_t code[gz::NUM_LL];
    const int n = c == 1 ? 19 : gz::NUM_LL, maxbits = c == 1 ? 7 : 15;
    for (int s = 0; s < n; s++) f[s] = 0;
    if (c == 0) { uint32_t a = 1, b = 1; for (int s = 0; s < 24; s++) { f[7 * s] = a; uint32_t t = a + b; a = b; b = t; } }
    if (c == 1) { uint32_t a = 1, b = 1; for (int s = 0; s < 19; s++) { f[s] = a; uint32_t t = a + b; a = b; b = t; } }
    if (c == 2) { f[65] = 100000; f[256] = 1; }
    if (c == 3) for (int s = 0; s < n; s++) f[s] = 1 + (s % 3);
    gz::limited_lengths(f, n, maxbits, len, &w);
    gz::canonical_codes(len, n, maxbits, code, &w);
    printf("C %d %d", n, maxbits);
    for (int s = 0; s < n; s++) printf(" %u:%u:%u", f[s], len[s], code[s]);
    printf("\n");
  }
  for (int i = 1; i + 2 < argc; i += 3) {
    const uint32_t a = strtoul(argv[i], 0, 10), b = strtoul(argv[i + 1], 0, 10);
    printf("X %u\n", gz::crc_join(a, b, gz::gf_x_pow(8ull * strtoull(argv[i + 2], 0, 10))));
  }
  printf("T %u %u\n", gz::crc_table_entry(1), gz::crc_table_entry(255));
  return 0;
}
"""


def test_coder_tables_limiter_and_crc_in_a_host_build(tmp_path):
    src = tmp_path / "codes.cpp"
    src.write_text(HARNESS)
    exe = tmp_path / "codes"
    subprocess.run(["g++", "-O1", "-std=c++17", "-I", os.path.join(ROOT, "spring_amd", "csrc"), str(src), "-o", str(exe)],
                   check=True)
    parts = [(b"abc" * 1000, b"x"), (b"", b"hello"), (os.urandom(70000), os.urandom(32768)), (b"q", b"")]
    args = []
    for a, b in parts:
        args += [str(zlib.crc32(a)), str(zlib.crc32(b)), str(len(b))]
    out = subprocess.run([str(exe)] + args, check=True, capture_output=True, text=True).stdout.splitlines()
    L = [list(map(int, x.split()[1:])) for x in out if x.startswith("L ")]
    D = [list(map(int, x.split()[1:])) for x in out if x.startswith("D ")]
    assert len(L) == 256 and len(D) == 32768
    for ln, s, e, v, e2 in L:   # RFC 1951 3.2.5
        assert 257 <= s <= 285 and e == e2 == LEN_EXTRA[s - 257] and LEN_BASE[s - 257] + v == ln and 0 <= v < (1 << e), ln
    for d, s, e, v, e2 in D:
        assert 0 <= s <= 29 and e == e2 == DIST_EXTRA[s] and DIST_BASE[s] + v == d and 0 <= v < (1 << e), d
    assert {x[1] for x in L} == set(range(257, 286)) and {x[1] for x in D} == set(range(30))
    codes = [x.split()[1:] for x in out if x.startswith("C ")]
    assert len(codes) == 4
    for row in codes:
        n, maxbits = int(row[0]), int(row[1])
        ent = [tuple(map(int, t.split(":"))) for t in row[2:]]
        assert len(ent) == n
        used = [(f, l, c) for f, l, c in ent if f]
        assert all(l == 0 for f, l, c in ent if not f)
        assert all(1 <= l <= maxbits for f, l, c in used)
        assert sum(2 ** (maxbits - l) for f, l, c in used) == 2 ** maxbits     # complete, not over-subscribed
        for f1, l1, _ in used:                                                  # a rarer symbol never has a shorter code
            for f2, l2, _ in used:
                assert not (f1 < f2 and l1 < l2)
        # prefix-free: the codes are stored bit-reversed, so no code is the low bits of another
        cs = sorted((l, c) for f, l, c in used)
        for i, (l1, c1) in enumerate(cs):
            for l2, c2 in cs[i + 1:]:
                assert (c2 & ((1 << l1) - 1)) != c1 or (l1, c1) == (l2, c2)
    fib = [f for f, l, c in [tuple(map(int, t.split(":"))) for t in codes[0][2:]] if f]
    assert len(fib) == 24 and max(int(t.split(":")[1]) for t in codes[0][2:]) == 15   # unlimited: 23 deep
    X = [int(x.split()[1]) for x in out if x.startswith("X ")]
    assert X == [zlib.crc32(a + b) for a, b in parts]
    assert out[-1] == "T %d %d" % (0x77073096, 0x2D02EF8D)
