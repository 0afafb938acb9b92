"""In-tree build of the native parts (gfx950 only): the HIP libraries of the ``HIP_LIBS`` table below -- each
``csrc/pvnet_<name>.hip`` with its C ABI in ``include/pvnet_<name>.h`` becomes ``libpvnet_<name>.so``, hipcc, no torch -- and
``ransac_voting.so``, the pybind11/torch shim over the C ABI of ``libpvnet_vote.so`` (host compiler only).

All land next to this file so they travel with the source tree (a JIT cache
under ~/.cache would not).  hipcc cross-compiles for gfx950 without a GPU.
"""
import os
import shutil
import subprocess
import sys
import sysconfig

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
INCLUDE = os.path.join(ROOT, "include")
CSRC = os.path.join(HERE, "csrc")
EXT = os.path.join(HERE, "ransac_voting.so")
ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")

# -ffp-contract=off is part of the numerical contract (bit-exact inlier counts), not a tuning flag.
# -fno-slp-vectorize: the SLP vectoriser turns pairs of scalar f32 ops into v_and/v_pk_* sequences that cost
# more issue slots than they save on gfx950 (count kernel 0.435 -> 0.395 ms with it off)
# (measured on the round-1 VALU kernel; kept: the SLP vectoriser has nothing to gain in these kernels).
# -amdgpu-mfma-vgpr-form: MFMA results land in VGPRs (gfx950 has a unified register file) instead of AGPRs plus one
# v_accvgpr_read per value (k_count_bf16 consumes every result on the VALU).
HIPCC_FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fno-slp-vectorize",
               "-mllvm", "-amdgpu-mfma-vgpr-form", "-fPIC", "-shared", "-fvisibility=hidden", "-Wall",
               "-Wno-unused-function"]
# pnp and pose are binary64 throughout and not part of the bit-exactness contract: default fp-contract
PNP_FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-shared", "-fvisibility=hidden", "-Wall"]

# The HIP libraries: name -> (flags, include directories) of csrc/pvnet_<name>.hip.  metrics and vsd take HIPCC_FLAGS for
# -ffp-contract=off: the ADD-S indices, the stated operation order and the bit-for-bit numpy twins need it.
HIP_LIBS = {
    "vote": (HIPCC_FLAGS, [INCLUDE, CSRC]),   # the voting kernels, one translation unit in parts (csrc/*.hpp)
    "nn": (HIPCC_FLAGS, [INCLUDE]),           # the ADD-S nearest-neighbour search
    "pnp": (PNP_FLAGS, [INCLUDE]),            # the batched uncertainty-PnP refinement
    "pose": (PNP_FLAGS, [INCLUDE]),           # the batched pose with its start: P3P / DLT + the refinement of pnp (csrc/pnp_lm.hpp)
    "metrics": (HIPCC_FLAGS, [INCLUDE]),      # the batched pose scores: ADD, ADD-S with its search, 2D projection, 5 cm 5 degrees, mask IoU
    "vsd": (HIPCC_FLAGS, [INCLUDE]),          # the batched depth rasteriser and the Visible Surface Discrepancy
    "icp": (HIPCC_FLAGS, [INCLUDE]),          # the batched ICP pose refinement: clouds, samples, the search and the fit
}


def _newer(target, *sources):
    if not os.path.exists(target):
        return False
    t = os.path.getmtime(target)
    return all(os.path.getmtime(s) <= t for s in sources)


def _run(cmd, verbose):
    if verbose:
        print("+", " ".join(cmd), flush=True)
    subprocess.check_call(cmd)


def lib_path(name):
    return os.path.join(HERE, "libpvnet_%s.so" % name)


def hip_sources(name):
    """What ``libpvnet_<name>.so`` is rebuilt after: its .hip, its ABI header and every csrc/*.hpp (more than any one library
    includes, so that no header edit leaves a stale build)."""
    return [os.path.join(CSRC, "pvnet_%s.hip" % name), os.path.join(INCLUDE, "pvnet_%s.h" % name),
            *(os.path.join(CSRC, f) for f in sorted(os.listdir(CSRC)) if f.endswith(".hpp"))]


def build_hip(name, force=False, verbose=False):
    flags, inc = HIP_LIBS[name]
    target, src = lib_path(name), hip_sources(name)
    if not force and _newer(target, *src):
        return target
    hipcc = shutil.which("hipcc") or os.path.join(ROCM, "bin", "hipcc")
    _run([hipcc, *flags, *("-I" + d for d in inc), "-o", target, src[0]], verbose)
    return target


def build_lib(force=False, verbose=False):
    return build_hip("vote", force, verbose)


def build_ext(force=False, verbose=False):
    src = os.path.join(CSRC, "ransac_voting_ext.cpp")
    hdr = os.path.join(INCLUDE, "pvnet_vote.h")
    lib = build_lib(verbose=verbose)
    if not force and _newer(EXT, src, hdr, lib):
        return EXT
    import torch
    from torch.utils import cpp_extension as ce
    tlib = os.path.join(os.path.dirname(torch.__file__), "lib")
    inc = [*ce.include_paths(), sysconfig.get_paths()["include"], INCLUDE, os.path.join(ROCM, "include")]
    cxx = os.environ.get("CXX", "g++")
    cmd = [cxx, "-O2", "-std=c++17", "-fPIC", "-shared", "-fvisibility=hidden", "-Wno-deprecated-declarations",
           "-DTORCH_EXTENSION_NAME=ransac_voting", "-DTORCH_API_INCLUDE_EXTENSION_H",
           "-D__HIP_PLATFORM_AMD__=1", "-DUSE_ROCM=1",
           "-D_GLIBCXX_USE_CXX11_ABI=%d" % int(torch._C._GLIBCXX_USE_CXX11_ABI)]
    cmd += ["-I" + p for p in inc]
    cmd += [src, "-o", EXT, "-L" + HERE, "-lpvnet_vote", "-L" + tlib, "-lc10", "-lc10_hip", "-ltorch_cpu",
            "-ltorch_hip", "-ltorch", "-ltorch_python", "-L" + os.path.join(ROCM, "lib"), "-lamdhip64",
            "-Wl,-rpath,$ORIGIN", "-Wl,-rpath," + tlib, "-Wl,-rpath," + os.path.join(ROCM, "lib")]
    _run(cmd, verbose)
    return EXT


def build_all(force=False, verbose=False):
    return (*(build_hip(name, force, verbose) for name in HIP_LIBS), build_ext(force, verbose))


if __name__ == "__main__":
    build_all(force="--force" in sys.argv, verbose=True)
