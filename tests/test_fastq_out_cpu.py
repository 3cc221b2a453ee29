"""CPU tests of the FASTQ assembler: the checker (tests/fastq_out_model.py) reassembles the golden files from their own
lines, and the C ABI surface that needs no device (exports, header, struct layouts, NULL refusals)."""
import ctypes as C
import os
import re
import subprocess

import pytest

import fastq_out_model as fm
import qualid_model as qm
from helpers import GOLDEN

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("j", [1, 2])
def test_model_reassembles_the_golden_file(j):
    raw = open(os.path.join(GOLDEN, "test_%d.fastq" % j), "rb").read()
    ids, reads, quals = qm.fastq_lines(raw)
    n = len(ids)
    slots = qm.order_array(None, n, False)
    by_slot = [qm.from_fastq(raw, kind, slots, 97)["lines"] for kind in (qm.QUALITY, qm.ID)]
    text, off = fm.assemble(by_slot[1], reads, by_slot[0])
    # the third line of a record is written as "+" whatever it was
    lines = [qm._no_cr(x) for x in qm._lines(raw)]
    lines[2::4] = [b"+"] * n
    assert text == b"".join(x + b"\n" for x in lines)
    if b"\r" not in raw and all(x == b"+" for x in qm._lines(raw)[2::4]):
        assert text == raw if raw.endswith(b"\n") else text == raw + b"\n"
    assert len(off) == n + 1 and int(off[-1]) == len(text)
    assert all(text[int(off[k]):int(off[k + 1])] == b"%s\n%s\n+\n%s\n" % (ids[k], reads[k], quals[k]) for k in range(n))
    # two-line form, a range, numbered ids
    t2, o2 = fm.assemble(ids, reads)
    assert t2 == b"".join(b"%s\n%s\n" % r for r in zip(ids, reads))
    tr, orr = fm.assemble(ids, reads, quals, (3, 10))
    assert tr == text[int(off[3]):int(off[10])] and orr.tolist() == (off[3:11] - off[3]).tolist()
    assert fm.numbered_ids(97, 3, 1) == [b"@98/2", b"@99/2", b"@100/2"]


def test_model_modify_id():
    assert fm.modify_id(b"@r1/1", 1) == b"@r1/2"
    assert fm.modify_id(b"@r1 x", 2) == b"@r1 x"
    assert fm.modify_id(b"@A:1 1:N:0 1:x", 3) == b"@A:1 2:N:0 1:x"   # only the first space counts
    assert fm.modify_id(b"1", 1) == b"2" and fm.modify_id(b" 1", 3) == b" 2"
    for rid, code in ((b"", 1), (b"", 3), (b"@nospace", 3), (b"@end ", 3), (b"@a", 0), (b"@a", 4)):
        with pytest.raises(fm.Refused):
            fm.modify_id(rid, code)
    # what check_id_pattern accepted, modify_id reproduces
    for a, b in ((b"@r1/1", b"@r1/2"), (b"@SRR1.5 5", b"@SRR1.5 5"), (b"@A:1:2 1:N:0:ACGT", b"@A:1:2 2:N:0:ACGT")):
        assert fm.modify_id(a, qm.find_id_pattern(a, b)) == b


def test_library_exports_the_assembler():
    """Fails without the stage: every spring_fastq_out_* symbol of the header is in the built library, and the Python
    class is exported."""
    import spring_amd
    from spring_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "spring_fastq_out.h")).read()
    declared = set(re.findall(r"^(?:int|void)\s+(spring_\w+)\s*\(", hdr, re.M))
    assert declared == set(_lib.FASTQ_OUT_EXPORTS) and len(declared) == 6
    assert not declared & (set(_lib.EXPORTS) | set(_lib.STREAMS_EXPORTS) | set(_lib.DECODE_EXPORTS) | set(_lib.QUALID_EXPORTS))
    L = _lib.lib()
    for name in sorted(declared):
        assert hasattr(L, name), name
    assert spring_amd.FastqOutStage is not None
    from spring_amd import build
    assert "fastq_out.hip" in build.SOURCES and "fastq_out_internal.h" in build.HEADERS
    assert "spring_fastq_out.h" in build.PUBLIC_HEADERS


@pytest.mark.parametrize("struct,mirror", [("spring_fastq_out_params", "FastqOutParams"),
                                           ("spring_fastq_out_sources", "FastqOutSources"),
                                           ("spring_fastq_out_info", "FastqOutInfo")])
def test_mirrors_match_the_c_layout(tmp_path, struct, mirror):
    from spring_amd import _lib
    M = getattr(_lib, mirror)
    fields = [f for f, _ in M._fields_]
    src = tmp_path / "off.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "spring_fastq_out.h"\nint main(void){\n'
                   'printf("%%zu\\n", sizeof(%s));\n' % struct
                   + "".join('printf("%%zu\\n", offsetof(%s, %s));\n' % (struct, f) for f in fields)
                   + "return 0;}\n")
    exe = tmp_path / "off"
    subprocess.run(["gcc", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert got[0] == C.sizeof(M)
    assert got[1:] == [getattr(M, f).offset for f in fields]


def test_refusals_without_a_device():
    from spring_amd import _lib
    L = _lib.lib()
    P, S, info = _lib.FastqOutParams(), _lib.FastqOutSources(), _lib.FastqOutInfo()
    assert L.spring_fastq_out_create(0, None) == -1
    assert L.spring_fastq_out_assemble(None, C.byref(P), C.byref(S), C.byref(info)) == -1
    assert L.spring_fastq_out_download(None, None, None) == -1
    assert L.spring_fastq_out_write(None, b"/dev/null", 0, None) == -1
    assert L.spring_fastq_out_get_info(None, C.byref(info)) == -1
    L.spring_fastq_out_destroy(None)
