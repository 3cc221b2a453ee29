"""GPU parity with the REFERENCE'S OWN STAGES (run with `pytest -m gpu`): the `num_chains = 1` reorder path and the
encoder stage against the files reorder_main<N> and encoder_main<N> themselves wrote, recorded in
tests/golden/ref_stage_<case>.npz (tests/golden/make_ref_golden.py; tests/test_oracle_vs_ref_stages.py keeps the fixtures
honest on the CPU).  Only the fixtures are read: a few hundred reads each, no shape beyond them.  Bar: byte for byte.

The reference's four gzip files are recorded uncompressed (the gzip filter is the one thing the reference build leaves
out); the GPU reader expects them compressed, so the tests gzip them, and gunzip what the GPU writes.

The three-thread fixture (thr3) stays at the CPU level: its hand-made file set swaps the singleton pool, so some clean
reads are referenced by no file and `streams + singletons == num_reads_clean`, which spring_encoder_run validates, does
not hold.  The entry point is not loosened for it."""
import ctypes as C
import gzip
import os

import numpy as np
import pytest

from helpers import ENCODER_FILES, GOLDEN, GZIP_TID_FILES
from ref_stage_cases import fixture_files

pytestmark = pytest.mark.gpu

CASES = ("fixed100", "var", "short20", "long300", "deepN", "fixed33", "fixed150", "fixed251")     # (thr3: see above)


def _fx(case):
    z = np.load(os.path.join(GOLDEN, "ref_stage_%s.npz" % case))
    assert bool(z["reorder_by_reference"]) and int(z["T"]) == 1 and int(z["K"]) == 1
    return dict(dna=z["in.dna"].tobytes(), dnaN=z["in.dnaN"].tobytes(), order_N=z["in.order_N"], n=int(z["n"]),
                L=int(z["L"]), reorder=fixture_files(z, "reorder"), encoder=fixture_files(z, "encoder"),
                matched=tuple(z["matched"].tolist()), unmatched=int(z["unmatched"]))


def _dir_files(d):
    out = {}
    for f in sorted(os.listdir(d)):
        with open(os.path.join(d, f), "rb") as fh:
            out[f] = fh.read()
    return out


def _put(d, files):
    for name, data in files.items():
        with open(os.path.join(d, name), "wb") as fh:
            fh.write(data)


def _gunzipped(files):
    return {k: (gzip.decompress(v) if k.rsplit(".", 1)[0] in GZIP_TID_FILES else v) for k, v in files.items()}


def _check_encoder_files(got, fx, info, what):
    """every stream, read_seq.bin.0.tmp against the reference's inflated .raw, .tail, the counts, nothing else left"""
    want = dict(fx["encoder"])
    want["read_seq.bin.0.tmp"] = want.pop("read_seq.bin.0.raw")
    assert sorted(got) == sorted(want), (what, sorted(got))
    assert set(ENCODER_FILES) <= set(got)
    for k in sorted(want):
        assert got[k] == want[k], (what, k, len(got[k]), len(want[k]))
    assert (info.matched_s, info.matched_N) == fx["matched"], what


@pytest.mark.parametrize("fused", [0, -1])
@pytest.mark.parametrize("case", CASES)
def test_ref_stages_reorder_in_memory(case, fused):
    """ReorderStage(num_chains = 1, num_thr = 1), fused round kernel and two-kernel round: the six streams against
    the reference's files, emit_dna against its temp.dna.0 / temp.dna.singleton."""
    import spring_amd as sa
    fx = _fx(case)
    ref = fx["reorder"]
    with sa.ReorderStage(sa.ReorderOpts(num_chains=1, num_thr=1, collect_stats=True, fused=fused)) as s:
        s.load_dna(fx["dna"], fx["n"], fx["L"])
        got = s.run().streams()
        dna0, dna_s = s.emit_dna(0), s.emit_dna(-1)
    for k, f, dt in (("order", "read_order.bin.0", np.uint32), ("rc", "read_rev.txt.0", np.uint8),
                     ("flag", "tempflag.txt.0", np.uint8), ("pos", "temppos.txt.0", np.int64),
                     ("rlen", "read_lengths.bin.0", np.uint16), ("order_s", "read_order.bin.singleton", np.uint32)):
        assert np.asarray(got[k], dt).tobytes() == ref[f], (case, k)
    assert dna0 == ref["temp.dna.0"] and dna_s == ref["temp.dna.singleton"]
    assert got["stats"]["unmatched"] == fx["unmatched"]
    assert np.array([len(got["order_s"])], np.uint32).tobytes() == ref["temp.dna.singleton.count"]


@pytest.mark.parametrize("case", CASES)
def test_ref_stages_reorder_file_contract(tmp_path, case):
    """spring_reorder_run with one chain and one thread: the gunzipped files equal the reference's byte for byte, the
    uncompressed ones equal as they are, the input is consumed and nothing else is left."""
    import spring_amd as sa
    from spring_amd import _lib
    fx = _fx(case)
    d = str(tmp_path)
    _put(d, {"input_clean_1.dna": fx["dna"]})
    L_ = _lib.lib()
    o = sa.ReorderOpts(num_chains=1, num_thr=1).to_c()
    assert L_.spring_reorder_run(d.encode(), fx["L"], 1, 0, fx["n"], 0, C.byref(o)) == 0, L_.spring_reorder_last_error()
    got = _dir_files(d)
    for f in GZIP_TID_FILES:
        assert got[f + ".0"][:2] == b"\x1f\x8b", f       # a gzip member, as the reference's encoder expects
    got = _gunzipped(got)
    assert sorted(got) == sorted(fx["reorder"]), sorted(got)
    for k in sorted(got):
        assert got[k] == fx["reorder"][k], (case, k)


@pytest.mark.parametrize("case", CASES)
def test_ref_stages_encoder_on_the_references_reorder_files(tmp_path, case):
    """spring_encoder_run on the reference's OWN reorder files (+ input_N.dna, read_order_N.bin) against the reference
    encoder's files."""
    from spring_amd import _lib
    fx = _fx(case)
    d = str(tmp_path)
    _put(d, {k: (gzip.compress(v, 6) if k.rsplit(".", 1)[0] in GZIP_TID_FILES else v) for k, v in fx["reorder"].items()})
    _put(d, {"input_N.dna": fx["dnaN"], "read_order_N.bin": fx["order_N"].tobytes()})
    L_ = _lib.lib()
    info = _lib.EncoderInfo()
    rc = L_.spring_encoder_run(d.encode(), fx["L"], 1, fx["n"] + len(fx["order_N"]), fx["n"], -1, C.byref(info))
    assert rc == 0, L_.spring_reorder_last_error()
    _check_encoder_files(_dir_files(d), fx, info, case)
    if case == "deepN":
        assert info.max_bin > 1000                       # the bin beyond MAX_SEARCH_ENCODER is there on the device too


@pytest.mark.parametrize("entry", ["two_calls", "one_call"])
@pytest.mark.parametrize("case", CASES)
def test_ref_stages_chained(tmp_path, case, entry):
    """GPU reorder (one chain) -> GPU encoder == reference reorder -> reference encoder, the N reads handed over the way
    the reference reads them (input_N.dna + read_order_N.bin): spring_reorder_run then spring_encoder_run over the
    files, and spring_reorder_encode_run with everything resident."""
    import spring_amd as sa
    from spring_amd import _lib
    fx = _fx(case)
    d = str(tmp_path)
    _put(d, {"input_clean_1.dna": fx["dna"], "input_N.dna": fx["dnaN"], "read_order_N.bin": fx["order_N"].tobytes()})
    L_ = _lib.lib()
    o = sa.ReorderOpts(num_chains=1, num_thr=1).to_c()
    info = _lib.EncoderInfo()
    total = fx["n"] + len(fx["order_N"])
    if entry == "two_calls":
        assert L_.spring_reorder_run(d.encode(), fx["L"], 1, 0, fx["n"], 0, C.byref(o)) == 0, L_.spring_reorder_last_error()
        rc = L_.spring_encoder_run(d.encode(), fx["L"], 1, total, fx["n"], -1, C.byref(info))
    else:
        rc = L_.spring_reorder_encode_run(d.encode(), fx["L"], 1, 0, fx["n"], 0, total, C.byref(o), C.byref(info))
    assert rc == 0, L_.spring_reorder_last_error()
    _check_encoder_files(_dir_files(d), fx, info, (case, entry))
