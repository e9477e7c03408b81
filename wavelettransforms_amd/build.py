"""Build libwtprune.so (HIP, gfx950) in-tree: wavelettransforms_amd/_lib/libwtprune.so.

hipcc cross-compiles for gfx950 without a GPU.  -ffp-contract=off is part of the parity
contract: PyWavelets' float32 filter bank uses separate multiplies and adds, so the
compiler must not fuse them into FMAs.

python -m wavelettransforms_amd.build [--force] [--csrc DIR] [--out FILE]
--csrc builds the *.hip files found in DIR (another revision's sources, or an edited copy: the
lab variants of tools/) against DIR/../../include, into --out.
"""
import argparse
import glob
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
OUT_DIR = os.path.join(HERE, "_lib")
LIB = os.path.join(OUT_DIR, "libwtprune.so")
SOURCES = ["prune_unit.hip", "filterbank.hip", "small.hip", "abs.hip", "modes.hip", "sweep.hip",
           "host_plan.hip", "host_chains.hip", "host_prune.hip", "host_methods.hip", "host_query.hip",
           "host_sweep.hip", "half.hip", "host_half.hip", "global.hip", "host_global.hip"]
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
ARCH = os.environ.get("WTP_OFFLOAD_ARCH", "gfx950")

FLAGS = ["--offload-arch=" + ARCH, "-O3", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off",
         "-Wall", "-Wno-unused-function"]


def stale():
    if not os.path.exists(LIB):
        return True
    t = os.path.getmtime(LIB)
    # every file of csrc/ is a dependency: a new header or .inc cannot be forgotten
    deps = glob.glob(os.path.join(CSRC, "*")) + [os.path.join(os.path.dirname(HERE), "include", "wtprune.h")]
    return any(os.path.getmtime(d) > t for d in deps)


def build(force=False, verbose=False, csrc=None, out=None):
    """csrc: a source directory other than the tree's (every *.hip in it is a translation unit, its
    public header is csrc/../../include); out: the library to write (default: the in-tree LIB)."""
    if csrc is None and out is None and not force and not stale():
        return LIB
    src_dir = os.path.abspath(csrc) if csrc else CSRC
    lib = os.path.abspath(out) if out else LIB
    sources = sorted(glob.glob(os.path.join(src_dir, "*.hip"))) if csrc else [os.path.join(CSRC, s) for s in SOURCES]
    inc = os.path.join(os.path.dirname(os.path.dirname(src_dir)), "include")
    os.makedirs(os.path.dirname(lib), exist_ok=True)
    tmp = lib + ".tmp"
    cmd = [HIPCC] + FLAGS + ["-I" + src_dir, "-I" + inc, "-o", tmp] + sources
    if verbose:
        print(" ".join(cmd), file=sys.stderr)
    subprocess.check_call(cmd)
    os.replace(tmp, lib)
    return lib


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--force", action="store_true", help="rebuild even when the library is up to date")
    ap.add_argument("--csrc", metavar="DIR", help="build the *.hip files of DIR instead of the tree's sources")
    ap.add_argument("--out", metavar="FILE", help="write the library to FILE")
    a = ap.parse_args()
    print(build(force=a.force, verbose=True, csrc=a.csrc, out=a.out))
