"""Build libnmhip.so (gfx950) in-tree with hipcc.

``python -m neuralmonkey_amd.build`` or ``__graft_entry__.build()``.  The
shared object is git-ignored but travels to the GPU box with the snapshot.
"""
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
LIB = os.path.join(HERE, "libnmhip.so")
ARCH = "gfx950"


# extra hipcc flags of single sources.  nm_ctc_beam.hip is compiled without the packed fp32 instructions (v_pk_add_f32,
# v_pk_mul_f32, v_pk_fma_f32): its arithmetic is per-lane log-space sums that gain nothing from them.  nm_edit.hip gets
# the same flag as a guard only: its arithmetic is integer, and its device assembly is the same with and without the
# flag -- it keeps a later floating-point line in that file from bringing the packed forms in.  nm_chrf.hip likewise:
# integer counts and a double-precision finish.  nm_sdp_stream.hip: its fp32 work is on the matrix cores and in per-lane
# softmax scalars; the rescale of four accumulators by one scalar is the only place the packed forms could appear.  The host half of the compilation does not know the feature and says so
# in a warning.
SOURCE_FLAGS = {
    "nm_ctc_beam.hip": ["-Xclang", "-target-feature", "-Xclang", "-packed-fp32-ops"],
    "nm_edit.hip": ["-Xclang", "-target-feature", "-Xclang", "-packed-fp32-ops"],
    "nm_chrf.hip": ["-Xclang", "-target-feature", "-Xclang", "-packed-fp32-ops"],
    "nm_sdp_stream.hip": ["-Xclang", "-target-feature", "-Xclang", "-packed-fp32-ops"],
}


def sources():
    return sorted(os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(".hip"))


def needs_build():
    if not os.path.exists(LIB):
        return True
    lib_m = os.path.getmtime(LIB)
    deps = sources() + [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(".h")]
    return any(os.path.getmtime(d) > lib_m for d in deps)


def build(force=False, verbose=True):
    if not force and not needs_build():
        return LIB
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    objs = []
    procs = []
    for src in sources():
        obj = src[:-4] + ".o"
        hdrs = [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(".h")]
        if (not force and os.path.exists(obj)
                and all(os.path.getmtime(obj) > os.path.getmtime(d) for d in [src] + hdrs)):
            objs.append(obj)
            continue
        cmd = [hipcc, f"--offload-arch={ARCH}", "-O3", "-std=c++17", "-fPIC", "-c", src, "-o", obj,
               "-Wno-unused-result"] + SOURCE_FLAGS.get(os.path.basename(src), []) \
            + os.environ.get("NM_HIPCC_FLAGS", "").split()
        if verbose:
            print(" ".join(cmd), flush=True)
        procs.append((subprocess.Popen(cmd), src))
        objs.append(obj)
    for p, src in procs:
        if p.wait() != 0:
            raise RuntimeError(f"hipcc failed on {src}")
    cmd = [hipcc, f"--offload-arch={ARCH}", "-shared", "-fPIC", "-o", LIB] + objs
    if verbose:
        print(" ".join(cmd), flush=True)
    subprocess.check_call(cmd)
    return LIB


if __name__ == "__main__":
    build(force="--force" in sys.argv)
    print(LIB)
