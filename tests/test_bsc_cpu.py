"""CPU-only checks of the BSC framing stage: the ctypes mirror of spring_bsc_info against the C header, the exported
symbols and the build lists, the stage's shared arithmetic (spring_amd/csrc/bsc_frame_plan.h: store rule, Adler-32 by
tiles, headers, piece numbering, offsets of both framings) in a stand-alone host build under the address and
undefined-behaviour sanitizers, and the plain-Python model (tests/bsc_frame_model.py) against the real bsc_compress /
bsc_store / bsc_adler32 of oracle/_ref/libref_units.so and the ref_bsc program (skipped where they are not built)."""
import ctypes as C
import os
import re
import struct
import subprocess
import zlib

import numpy as np
import pytest

import bsc_frame_model as fm
import bwt_model as bm
import qlfc_model as qm
import spring_amd.bsc  # noqa: F401  (the stage under test: nothing here runs without it)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = fm.ref_lib()
needs_ref = pytest.mark.skipif(REF is None, reason="oracle/_ref/libref_units.so not built (needs the reference sources)")
MOD = 65521


def test_ctypes_mirror_matches_the_c_header(tmp_path):
    from spring_amd import _lib
    from spring_amd.bsc import BscInfo, FRAMING, KINDS
    fields = [k for k, _ in BscInfo._fields_]
    names = ("HEADER_BYTES", "PASSES", "BLOCKS", "FILE", "STR_ARRAY", "CODED", "STORED_SMALL", "STORED_CODER", "STORED_NO_GAIN")
    src = tmp_path / "abi.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "spring_bsc.h"\nint main(void) {\n'
                   '  printf("%zu", sizeof(spring_bsc_info));\n'
                   + "".join('  printf(" %%d", SPRING_BSC_%s);\n' % k for k in names)
                   + "".join('  printf(" %%zu", offsetof(spring_bsc_info, %s));\n' % k for k in fields)
                   + "  return 0; }\n")
    exe = tmp_path / "abi"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    want = ([C.sizeof(BscInfo), _lib.BSC_HEADER_BYTES, _lib.BSC_PASSES, _lib.BSC_BLOCKS, _lib.BSC_FILE, _lib.BSC_STR_ARRAY,
             _lib.BSC_CODED, _lib.BSC_STORED_SMALL, _lib.BSC_STORED_CODER, _lib.BSC_STORED_NO_GAIN]
            + [getattr(BscInfo, k).offset for k in fields])
    assert got == want, (got, want)
    assert (fm.HEADER, fm.BLOCKS, fm.BSC_FILE, fm.STR_ARRAY) == (_lib.BSC_HEADER_BYTES, _lib.BSC_BLOCKS, _lib.BSC_FILE, _lib.BSC_STR_ARRAY)
    assert (fm.CODED, fm.STORED_SMALL, fm.STORED_CODER, fm.STORED_NO_GAIN) == (0, 1, 2, 3) and len(KINDS) == 4
    assert FRAMING == {"blocks": 0, "file": 1, "str_array": 2}
    s = BscInfo()
    s.stored_no_gain, s.ms_pass[2] = 7, 1.5
    assert s.asdict()["stored_no_gain"] == 7 and s.asdict()["ms_pass"] == [0, 0, 1.5]


def test_library_exports_every_declared_symbol():
    from spring_amd import _lib, build
    import spring_amd
    hdr = open(os.path.join(ROOT, "include", "spring_bsc.h")).read()
    declared = set(re.findall(r"\b(spring_bsc_\w+)\s*\(", hdr))
    assert declared == set(_lib.BSC_EXPORTS) and len(_lib.BSC_EXPORTS) == len(declared)
    others = [getattr(_lib, k) for k in dir(_lib) if k.endswith("EXPORTS") and k != "BSC_EXPORTS"]
    assert len(others) >= 10
    for lst in others:
        assert not declared & set(lst)
    L = _lib.lib()
    for name in sorted(declared):
        assert hasattr(L, name), "libspring_reorder_hip.so does not export " + name
    assert spring_amd.BscStage is not None
    assert "bsc_frame.hip" in build.SOURCES and "bsc_frame_plan.h" in build.HEADERS and "spring_bsc.h" in build.PUBLIC_HEADERS
    for lst in (build.SOURCES, build.HEADERS, build.PUBLIC_HEADERS):
        assert len(lst) == len(set(lst))
        assert all(os.path.exists(os.path.join(ROOT, "include" if lst is build.PUBLIC_HEADERS else "spring_amd/csrc", f)) for f in lst)
    # the info structure lives with its stage: _lib's own set is what tests/test_stage_frame_cpu.py says it is
    assert not hasattr(_lib, "BscInfo")


def test_stage_lifecycle_against_a_stub(monkeypatch):
    """As tests/test_stage_frame_cpu.py does for the other stages: create, get_info, destroy, once each."""
    from spring_amd import _lib
    from spring_amd.bsc import BscStage
    calls = []

    class Stub:
        def __getattr__(self, name):
            def fn(*args):
                calls.append(name)
                if name.endswith("_create"):
                    args[1]._obj.value = 0x1000
                return 0
            return fn
    monkeypatch.setattr(_lib, "lib", lambda: Stub())
    with BscStage() as st:
        assert st._h.value == 0x1000 and st.info is None
        assert isinstance(st.get_info(), dict) and st.info is None
        with pytest.raises(ValueError):
            st.frame(None, None, b"abc")
    assert calls == ["spring_bsc_create", "spring_bsc_get_info", "spring_bsc_destroy"] and not st._h


# ---------------------------------------------------------------------------------------------- bsc_frame_plan.h
HARNESS = r"""
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "bsc_frame_plan.h"
using namespace bscf;

// A segment summed as the device sums it: tiles (bytes and weights as k_tiles forms them), then 256 runs of
// consecutive tiles, then the runs in order (k_fold).  byte_at(i): byte i of the segment.
template <class F> static uint32_t tiled(uint64_t addr, uint64_t len, F byte_at, bool uniform) {
  const uint64_t nt = num_tiles(addr, len), per = (nt + 255) / 256;
  Sum full{0, 0};
  bool have_full = false;
  Sum all{1, 0};
  for (uint64_t lane = 0; lane < 256; lane++) {
    const uint64_t a = lane * per < nt ? lane * per : nt, b = a + per < nt ? a + per : nt;
    Sum acc{1, 0};
    uint64_t run = 0;
    for (uint64_t t = a; t < b; t++) {
      uint64_t lo, hi;
      tile_range(addr, len, t, &lo, &hi);
      Sum s;
      if (uniform && hi - lo == TILE && have_full) {
        s = full;   // every full tile of one repeated byte is the same tile
      } else {
        uint32_t bytes = 0, weighted = 0;
        for (uint64_t i = lo; i < hi; i++) { bytes += byte_at(i); weighted += (uint32_t)(hi - i) * byte_at(i); }
        s = tile_sum(bytes, weighted, (uint32_t)(hi - lo));
        if (uniform && hi - lo == TILE) { full = s; have_full = true; }
      }
      acc = combine(acc, s, hi - lo);
      run += hi - lo;
    }
    all = combine(all, acc, run);
  }
  return value(all);
}

int main(int argc, char **argv) {
  // O: the store rule.  argv[1]: a file of random bytes for the sums.
  const uint64_t rule[][4] = {{0, 1, 0, 0}, {1, 1, 0, 0}, {28, 0, 5, 0}, {28, 1, 0, 0}, {29, 0, 5, 0}, {29, 1, 0, 0}, {29, 0, 27, 0},
                              {29, 0, 28, 0}, {65535, 0, 100, 7}, {65536, 0, 100, 7}, {65535, 0, 65533, 7}, {65535, 0, 65534, 7},
                              {65536, 0, 65536 - 30, 7}, {65536, 0, 65536 - 29, 7}, {70000, 1, 0, 8}, {70000, 0, 69999 - 33, 8},
                              {70000, 0, 70000 - 33, 8}, {1u << 30, 0, 1000, 255}};
  for (auto &c : rule) {
    const int oc = outcome(c[0], (int32_t)c[1], c[2], (uint32_t)c[3]);
    uint64_t len[4];
    piece_lengths(len, BSC_FILE, c[0], oc, c[2], (uint32_t)c[3]);
    printf("O %llu %llu %llu %llu %d %llu %u %llu %llu %llu %llu\n", (unsigned long long)c[0], (unsigned long long)c[1],
           (unsigned long long)c[2], (unsigned long long)c[3], oc, (unsigned long long)block_bytes(c[0], oc, c[2], (uint32_t)c[3]),
           kept_indexes(c[0], (uint32_t)c[3]), (unsigned long long)len[0], (unsigned long long)len[1], (unsigned long long)len[2],
           (unsigned long long)len[3]);
  }
  // T: sums by tiles over windows of the file, at every misalignment
  std::vector<uint8_t> buf;
  FILE *f = fopen(argv[1], "rb");
  if (!f) return 2;
  for (int c; (c = fgetc(f)) != EOF;) buf.push_back((uint8_t)c);
  fclose(f);
  const uint64_t lens[] = {0, 1, 15, 16, 17, 4095, 4096, 4097, 8195, 5552, 5553, 20000};
  for (uint64_t h = 0; h < 16; h++)
    for (uint64_t n : lens) {
      const uint64_t start = 3 * h;
      if (start + n > buf.size()) return 3;
      const uint8_t *p = buf.data() + start;
      printf("T %llu %llu %llu %u %u\n", (unsigned long long)h, (unsigned long long)start, (unsigned long long)n,
             tiled(0x1000 + h, n, [&](uint64_t i) { return (uint32_t)p[i]; }, false), adler_bytes(p, (uint32_t)n));
    }
  // F: 0xFF, up to 2^30 bytes; the largest tile's numbers
  const uint64_t big[] = {4096, 65521, (1ull << 20) + 1, (64ull << 20) + 1, 1ull << 30};
  for (uint64_t n : big)
    for (uint64_t h : {0ull, 5ull, 15ull})
      printf("F %llu %llu %u\n", (unsigned long long)n, (unsigned long long)h, tiled(0x2000 + h, n, [](uint64_t) { return 255u; }, true));
  {
    uint64_t bytes = 0, weighted = 0;
    for (uint64_t i = 0; i < TILE; i++) { bytes += 255; weighted += (TILE - i) * 255; }
    printf("X %llu %llu\n", (unsigned long long)bytes, (unsigned long long)(weighted + TILE));
  }
  // L: offsets of both framings.  argv[2 ..]: per file the number of its blocks; block j has 28 + 7 j + 1 bytes
  std::vector<uint64_t> file_first(1, 0), size;
  for (int i = 2; i < argc; i++) file_first.push_back(file_first.back() + strtoull(argv[i], 0, 10));
  const uint64_t F = file_first.size() - 1, S = file_first.back();
  for (uint64_t j = 0; j < S; j++) size.push_back(HEADER + 7 * j + 1);
  for (int framing = 0; framing < 3; framing++) {
    std::vector<uint64_t> file_off(F + 1), block_off(S + 1);
    layout(framing, size.data(), file_first.data(), F, file_off.data(), block_off.data());
    // the same from the pieces, as the device's scan sees them
    const uint64_t P = F + BLOCK_PIECES * S;
    std::vector<uint64_t> len(P + 1, ~0ull), dst(P + 1);
    for (uint64_t fl = 0; fl < F; fl++) {
      len[piece_of_file(fl, file_first[fl])] = file_header_bytes(framing);
      for (uint64_t j = file_first[fl]; j < file_first[fl + 1]; j++)   // coded: r = 7 j bytes, no indexes
        piece_lengths(&len[piece_of_block(j, fl)], framing, 100000, CODED, 7 * j, 0);
    }
    len[P] = 0;
    uint64_t at = 0, bad = 0;
    for (uint64_t p = 0; p <= P; p++) { if (len[p] == ~0ull) bad++; dst[p] = at; at += len[p]; }
    for (uint64_t fl = 0; fl < F; fl++) {
      if (dst[piece_of_file(fl, file_first[fl])] != file_off[fl]) bad++;
      for (uint64_t j = file_first[fl]; j < file_first[fl + 1]; j++)
        if (dst[piece_of_block(j, fl)] + cut_header_bytes(framing) != block_off[j]) bad++;
    }
    if (dst[P] != file_off[F]) bad++;
    printf("L %d %llu", framing, (unsigned long long)bad);
    for (uint64_t v : file_off) printf(" %llu", (unsigned long long)v);
    printf(" |");
    for (uint64_t j = 0; j < S; j++) printf(" %llu", (unsigned long long)block_off[j]);
    printf("\n");
  }
  // H: headers.  a coded block of n = 70000, r = 1234, k = 8, primary 4321; a stored one of n = 20
  uint8_t h[10 + HEADER];
  cut_header(h, BSC_FILE, 0x123456789aull);
  header_front(h + 10, 70000, CODED, 1234, 8, 4321, 0xdeadbeefu);
  header_back(h + 10, 0x01020304u);
  printf("H ");
  for (uint8_t b : h) printf("%02x", b);
  cut_header(h, STR_ARRAY, 77);
  header_front(h + 2, 20, STORED_SMALL, 0, 3, 9, 0xcafef00du);
  header_back(h + 2, 0xcafef00du);
  printf("\nH ");
  for (int i = 0; i < 2 + (int)HEADER; i++) printf("%02x", h[i]);
  printf("\n");
  return 0;
}
"""


@pytest.fixture(scope="module")
def plan_out(tmp_path_factory):
    d = tmp_path_factory.mktemp("bsc_plan")
    src, exe, data = d / "plan.cpp", d / "plan", d / "bytes"
    src.write_text(HARNESS)
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(ROOT, "spring_amd", "csrc"), str(src), "-o", str(exe)], check=True)
    raw = np.random.default_rng(21).integers(0, 256, 20100).astype(np.uint8)
    raw[4000:9000] = 255     # whole tiles of the largest byte among the random ones
    data.write_bytes(raw.tobytes())
    # leak detection needs ptrace, which not every box grants; the harness frees what it allocates anyway
    r = subprocess.run([str(exe), str(data)] + [str(x) for x in FILES], capture_output=True, text=True,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    assert r.returncode == 0, r.stderr[-2000:]
    return r.stdout.splitlines(), raw.tobytes()


FILES = [0, 2, 0, 0, 1, 3, 0]   # blocks per file: files without cuts at both ends and in the middle


def _rows(out, tag):
    return [x.split()[1:] for x in out if x.startswith(tag + " ")]


def test_store_rule(plan_out):
    rows = [[int(v) for v in r] for r in _rows(plan_out[0], "O")]
    got = {(n, status, r, k): (oc, size, kept, pieces) for n, status, r, k, oc, size, kept, *pieces in rows}
    S, C, G, K = fm.STORED_SMALL, fm.STORED_CODER, fm.STORED_NO_GAIN, fm.CODED
    want = {(0, 1, 0, 0): S, (1, 1, 0, 0): S, (28, 0, 5, 0): S, (28, 1, 0, 0): S, (29, 0, 5, 0): K, (29, 1, 0, 0): C,
            (29, 0, 27, 0): K,                     # r + 1 = n - 1: coded
            (29, 0, 28, 0): G,                     # r + 1 = n: stored
            (65535, 0, 100, 7): K, (65536, 0, 100, 7): K,
            (65535, 0, 65533, 7): K,               # below 64 KiB the indexes do not count: r + 1 = n - 1
            (65535, 0, 65534, 7): G,
            (65536, 0, 65536 - 30, 7): K,          # from 64 KiB on they do: r + 1 + 28 = n - 1
            (65536, 0, 65536 - 29, 7): G,
            (70000, 1, 0, 8): C, (70000, 0, 69999 - 33, 8): K, (70000, 0, 70000 - 33, 8): G, (1 << 30, 0, 1000, 255): K}
    assert set(got) == set(want)
    for key, oc in want.items():
        n, status, r, k = key
        kept = 0 if n < 65536 else k
        size = 28 + (r + 1 + 4 * kept if oc == K else n)
        assert got[key] == (oc, size, kept, [38, r if oc == K else n, 4 * kept if oc == K else 0, int(oc == K)]), key
        assert fm.outcome(n, r if status == 0 else -3, k) == oc, key      # and the Python model says the same


def test_sums_by_tiles_equal_a_byte_loop(plan_out):
    out, raw = plan_out
    rows = [[int(v) for v in r] for r in _rows(out, "T")]
    assert len(rows) == 16 * 12
    for h, start, n, tiled, loop in rows:
        want = zlib.adler32(raw[start:start + n]) & 0xffffffff
        assert tiled == want and loop == want, (h, start, n)
    assert any(n == 0 and tiled == 1 for _, _, n, tiled, _ in rows)


def test_sums_of_ff_up_to_one_gibibyte_equal_the_closed_form(plan_out):
    rows = [[int(v) for v in r] for r in _rows(plan_out[0], "F")]
    assert {n for n, _, _ in rows} == {4096, 65521, (1 << 20) + 1, (64 << 20) + 1, 1 << 30} and len(rows) == 15
    for n, h, got in rows:
        a = (1 + 255 * n) % MOD
        b = (n + 255 * n * (n + 1) // 2) % MOD
        assert got == b << 16 | a, (n, h)
    assert zlib.adler32(b"\xff" * ((1 << 20) + 1)) & 0xffffffff == [g for n, h, g in rows if n == (1 << 20) + 1][0]
    (bytes_, weighted), = [[int(v) for v in r] for r in _rows(plan_out[0], "X")]
    assert bytes_ == 255 * 4096 and weighted == 255 * 4096 * 4097 // 2 + 4096 < 1 << 32


def test_offsets_of_both_framings(plan_out):
    rows = _rows(plan_out[0], "L")
    assert len(rows) == 3
    first = np.cumsum([0] + FILES)
    blocks = [bytes(28 + 7 * j + 1) for j in range(int(first[-1]))]
    for row in rows:
        framing, bad = int(row[0]), int(row[1])
        bar = row.index("|")
        file_off, block_off = [int(v) for v in row[2:bar]], [int(v) for v in row[bar + 1:]]
        assert bad == 0, framing                 # the piece numbering gives the same places as layout()
        files = [fm.frame(framing, [(0, blocks[j]) for j in range(first[f], first[f + 1])]) for f in range(len(FILES))]
        assert file_off == list(np.cumsum([0] + [len(x) for x in files])), framing
        assert len(files[0]) == (0 if framing == fm.BLOCKS else 4)
        at = {fm.BLOCKS: 0, fm.BSC_FILE: 10, fm.STR_ARRAY: 2}[framing]
        for f in range(len(FILES)):
            pos = file_off[f] + (0 if framing == fm.BLOCKS else 4)
            for j in range(first[f], first[f + 1]):
                assert block_off[j] == pos + at, (framing, j)
                pos += at + len(blocks[j])


def test_headers(plan_out):
    a, b = [bytes.fromhex(r[0]) for r in _rows(plan_out[0], "H")]
    head = struct.pack("<iiiiII", 28 + 1234 + 1 + 32, 70000, fm.MODE, 4321, 0xdeadbeef, 0x01020304)
    assert a == struct.pack("<qbb", 0x123456789a, 1, 1) + head + struct.pack("<I", fm.adler(head))
    head = struct.pack("<iiiiII", 48, 20, 0, 0, 0xcafef00d, 0xcafef00d)
    assert b == b"\x01\x01" + head + struct.pack("<I", fm.adler(head))


# ---------------------------------------------------------------------------------------------- the model
def test_model_on_worked_examples():
    blk = fm.store(b"abc")
    assert len(blk) == 31 and fm.parse_block(blk) == dict(size=31, n=3, mode=0, primary=0, adler_in=fm.adler(b"abc"), body=b"abc")
    data = fm.text(70000)
    blk, kind = fm.block(data, 17, list(range(1, 9)), b"xyz", 3)
    p = fm.parse_block(blk)
    assert kind == fm.CODED and p["mode"] == 33 and p["primary"] == 17 and p["body"] == b"xyz" + struct.pack("<8i", *range(1, 9)) + b"\x08"
    blk, kind = fm.block(data[:65535], 17, list(range(1, 8)), b"xyz", 3)
    assert kind == fm.CODED and fm.parse_block(blk)["body"] == b"xyz\x00"
    assert fm.block(data, 17, [], b"", -3) == (fm.store(data), fm.STORED_CODER)
    assert fm.block(data[:28], 1, [], b"x", 1) == (fm.store(data[:28]), fm.STORED_SMALL)
    assert fm.block(data[:100], 1, [], bytes(99), 99) == (fm.store(data[:100]), fm.STORED_NO_GAIN)
    assert fm.cuts(0, 10) == [] and fm.cuts(25, 10) == [(0, 10), (10, 20), (20, 25)] and fm.cuts(20, 10) == [(0, 10), (10, 20)]
    assert fm.bsc_file([]) == fm.str_array_file([]) == b"\0\0\0\0"
    assert fm.bsc_file([(0, b"AA"), (5, b"B")]) == b"\2\0\0\0" + bytes(8) + b"\1\1AA" + b"\5" + bytes(7) + b"\1\1B"
    assert fm.str_array_file([b"AA", b"B"]) == b"\2\0\0\0\1\1AA\1\1B"
    data, off = fm.sum_batch()
    lens = np.diff(off).astype(np.int64)
    assert set(fm.SUM_LENGTHS) <= set(lens) and lens[-1] == (64 << 20) + 1 and lens[-2] == (1 << 20) + 1
    starts = {int(o) % 16 for o, n in zip(off[:-1], lens) if n == 100}
    assert starts == set(range(16))
    assert len(fm.no_gain_case()) == fm.NO_GAIN_N + fm.NO_GAIN_RUN


def _real_parts(data):
    """The real block sort and coder on data -> (primary, indexes, coded, rc)."""
    out, primary, idx = bm.ref_bwt(data, fm.FEATURES)
    coded, rc = qm.ref_compress(out)
    return primary, idx, coded, rc


CASES = tuple(qm.SMALL) + ("a300000", "bwt300000", "random4096")


@needs_ref
def test_model_equals_the_real_bsc_compress_and_bsc_store():
    seen = set()
    datas = [qm.case(n) for n in CASES] + [fm.text(n) for n in (1, 28, 29, 65535, 65536)] + [
        fm.no_gain_case(), fm.no_gain_case(fm.NO_GAIN_EQ_RUN), fm.no_gain_case(fm.GAIN_RUN)]
    for data in datas:
        want = fm.ref_block(data)
        got, kind = fm.block(data, *_real_parts(data))
        seen.add(kind)
        assert got == want, len(data)
        assert fm.ref_adler(data) == fm.adler(data)
        back, rc = fm.ref_decompress(got, len(data))
        assert rc == 0 and back == data
        assert fm.ref_store(data) == fm.store(data)
        assert (fm.ref_inplace_rc(data) == fm.NOT_COMPRESSIBLE) == (kind in (fm.STORED_CODER, fm.STORED_NO_GAIN)), len(data)
    assert seen == {0, 1, 2, 3}
    assert fm.ref_adler(b"") == 1


@needs_ref
def test_the_no_gain_cases_take_the_branches_they_are_for():
    for run, want, margin in ((fm.NO_GAIN_RUN, fm.STORED_NO_GAIN, 12), (fm.NO_GAIN_EQ_RUN, fm.STORED_NO_GAIN, 0),
                              (fm.GAIN_RUN, fm.CODED, -1)):
        data = fm.no_gain_case(run)
        primary, idx, coded, rc = _real_parts(data)
        assert rc == fm.NO_GAIN_CODED >= 0 and len(idx) == 8 and len(data) >= 65536
        assert rc + 1 + 4 * len(idx) - len(data) == margin
        assert (fm.ref_inplace_rc(data) == fm.NOT_COMPRESSIBLE) == (want == fm.STORED_NO_GAIN)
        assert fm.block(data, primary, idx, coded, rc)[1] == want
    # below the window the coder itself gives up
    assert _real_parts(fm.no_gain_case(800))[3] == fm.NOT_COMPRESSIBLE


@needs_ref
@pytest.mark.skipif(fm.ref_bsc_bin() is None, reason="oracle/_ref/ref_bsc not built")
def test_model_equals_the_ref_bsc_program():
    for data in (b"", b"x", fm.text(5000), qm.case("random4096"), fm.text(70000)):
        blocks = [(lo, fm.block(data[lo:hi], *_real_parts(data[lo:hi]))[0]) for lo, hi in fm.cuts(len(data), 64 << 20)]
        assert fm.ref_bsc_file(data) == fm.bsc_file(blocks), len(data)
