"""Builds libspring_reorder_hip.so in-tree with hipcc for gfx950 (no GPU needed to build)."""
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(HERE, "csrc")
LIBDIR = os.path.join(HERE, "lib")
LIB = os.path.join(LIBDIR, "libspring_reorder_hip.so")
SOURCES = ["reorder_kernels.hip", "reorder_pipeline.cpp", "reorder_files.cpp", "order_ops.hip", "fastq_kernels.hip",
           "encoder.hip", "fastq_reorder.hip", "streams.hip", "decode.hip", "qualid.hip", "fastq_out.hip", "dict_build.hip",
           "gzip.hip", "bwt.hip", "unbwt.hip", "idcodec.hip", "qlfc.hip", "bsc_frame.hip", "unqlfc.hip"]
HEADERS = ["reorder_device.h", "reorder_internal.h", "reorder_round_mc.h", "synth_common.h", "call_reorder.h",
           "encoder_internal.h", "streams_internal.h", "fastq_out_internal.h", "dict_build.h", "strand_filter.h",
           "gzip_codes.h", "bwt_plan.h", "bwt_internal.h", "unbwt_plan.h", "stage_host.h", "qlfc_plan.h", "qlfc_params.h",
           "bsc_frame_plan.h", "unqlfc_plan.h", "copy_words.h"]
PUBLIC_HEADERS = ["spring_reorder.h", "spring_encoder.h", "spring_streams.h", "spring_decode.h", "spring_qualid.h",
                  "spring_fastq_out.h", "spring_gzip.h", "spring_bwt.h", "spring_unbwt.h", "spring_idcodec.h",
                  "spring_qlfc.h", "spring_bsc.h", "spring_unqlfc.h"]


def _stale():
    if not os.path.exists(LIB):
        return True
    t = os.path.getmtime(LIB)
    deps = [os.path.join(CSRC, f) for f in SOURCES + HEADERS] + [os.path.join(ROOT, "include", h) for h in PUBLIC_HEADERS]
    return any(os.path.getmtime(d) > t for d in deps)


def build(force=False, verbose=False):
    if not force and not _stale():
        return LIB
    os.makedirs(LIBDIR, exist_ok=True)
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    objs, cmds = [], []
    for src in SOURCES:
        obj = os.path.join(LIBDIR, os.path.splitext(src)[0] + ".o")
        objs.append(obj)
        if not force and os.path.exists(obj) and os.path.getmtime(obj) > max(
                os.path.getmtime(os.path.join(CSRC, f)) for f in [src] + HEADERS) and os.path.getmtime(obj) > max(
                os.path.getmtime(os.path.join(ROOT, "include", h)) for h in PUBLIC_HEADERS):
            continue  # object newer than its source and every header
        cmds.append([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-x", "hip",
                     "-I" + os.path.join(ROOT, "include"), "-I" + CSRC, "-c", os.path.join(CSRC, src), "-o", obj])
    procs = []
    for cmd in cmds:  # the translation units are independent: compile them side by side
        if verbose:
            print(" ".join(cmd), file=sys.stderr)
        procs.append((cmd, subprocess.Popen(cmd)))
    for cmd, pr in procs:
        if pr.wait() != 0:
            raise subprocess.CalledProcessError(pr.returncode, cmd)
    cmd = [hipcc, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", LIB] + objs + ["-lz"]
    subprocess.run(cmd, check=True)
    return LIB


if __name__ == "__main__":
    print(build(force="--force" in sys.argv, verbose=True))
