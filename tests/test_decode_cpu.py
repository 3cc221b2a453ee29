"""CPU tests of the stream decoder (include/spring_decode.h): the C ABI surface that needs no device, and the
adversarial-escape fixtures of tests/decode_cases.py through the checker (tests/streams_model.py)."""
import ctypes as C
import os
import re
import subprocess

import pytest

import decode_cases as dc
import streams_model as sm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_declarations_equal_decode_exports():
    from spring_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "spring_decode.h")).read()
    declared = set(re.findall(r"\b(spring_decode_\w+)\s*\(", hdr))
    assert declared == set(_lib.DECODE_EXPORTS)
    assert not set(_lib.DECODE_EXPORTS) & set(_lib.EXPORTS)
    assert not set(_lib.DECODE_EXPORTS) & set(_lib.STREAMS_EXPORTS)
    L = _lib.lib()
    for name in sorted(declared):
        assert hasattr(L, name), name


def test_decode_info_matches_the_c_layout(tmp_path):
    from spring_amd import _lib
    fields = [f for f, _ in _lib.DecodeInfo._fields_]
    src = tmp_path / "off.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "spring_decode.h"\nint main(void){\n'
                   'printf("%zu\\n", sizeof(spring_decode_info));\n'
                   + "".join('printf("%%zu\\n", offsetof(spring_decode_info, %s));\n' % f for f in fields)
                   + "return 0;}\n")
    exe = tmp_path / "off"
    subprocess.run(["gcc", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert got[0] == C.sizeof(_lib.DecodeInfo)
    assert got[1:] == [getattr(_lib.DecodeInfo, f).offset for f in fields]


def test_refusals_without_a_device(tmp_path):
    from spring_amd import _lib
    L = _lib.lib()
    info = _lib.DecodeInfo()
    assert L.spring_decode_create(0, None) == -1
    assert L.spring_decode_seq_from_encoder(None, None) == -1
    assert L.spring_decode_seq_from_host(None, 0, None, None, None) == -1
    assert L.spring_decode_from_streams(None, None, C.byref(info)) == -1
    assert L.spring_decode_from_host(None, None, None, 0, 1, 1, 0, 0, 1, C.byref(info)) == -1
    assert L.spring_decode_download(None, 0, None, None) == -1
    assert L.spring_decode_get_info(None, C.byref(info)) == -1
    assert L.spring_decode_seq_from_files(None, None, 1, ) == -1
    assert L.spring_decode_from_files(None, None, 0, 1, 1, 0, 0, 1, C.byref(info)) == -1
    L.spring_decode_destroy(None)
    # a directory without the files: an I/O error before any device is touched; nothing created or removed
    d = str(tmp_path)
    open(os.path.join(d, "keep.txt"), "w").write("x")
    assert L.spring_decode_seq_from_files(None, d.encode(), 2) == -2
    assert L.spring_decode_from_files(None, d.encode(), 0, 1, 10, 0, 0, 10, C.byref(info)) == -2
    assert L.spring_decode_from_files(None, d.encode(), 3, 2, 10, 1, 1, 2, C.byref(info)) == -2
    assert os.listdir(d) == ["keep.txt"]


@pytest.mark.parametrize("name", sorted(dc.escape_cases()))
@pytest.mark.parametrize("B", [1, 3, 7, 1 << 30])
def test_escape_fixtures_round_trip_through_the_checker(name, B):
    enc, seq, N, reads = dc.custom_case(dc.escape_cases()[name], unaligned=("ACGTN" * 3, ""))
    st = sm.write_streams(enc, N, False, False, B)
    assert sm.read_all(st, seq, N, False, False, B) == reads
    if B == 1 << 30:
        assert dc.writer_escapes(enc, N, B) >= {"decreasing": 24, "gaps": 2, "ffff_payloads": 4}[name]
