"""In-tree build of the native parts (gfx950 only).

  libpvnet_vote.so   HIP kernels + C ABI (include/pvnet_vote.h), hipcc, no torch
  ransac_voting.so   pybind11/torch shim over that C ABI, host compiler only
  libpvnet_nn.so     ADD-S nearest-neighbour search (include/pvnet_nn.h)
  libpvnet_pnp.so    batched uncertainty-PnP refinement (include/pvnet_pnp.h)
  libpvnet_pose.so   batched pose with its start: P3P / DLT + the same refinement (include/pvnet_pose.h)
  libpvnet_metrics.so  batched pose scores: ADD, ADD-S with its search, 2D projection, 5 cm 5 degrees, mask IoU
                     (include/pvnet_metrics.h)
  libpvnet_vsd.so    batched depth rasteriser and Visible Surface Discrepancy (include/pvnet_vsd.h)

Both land next to this file so they travel with the source tree (a JIT cache
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
LIB = os.path.join(HERE, "libpvnet_vote.so")
EXT = os.path.join(HERE, "ransac_voting.so")
NNLIB = os.path.join(HERE, "libpvnet_nn.so")
PNPLIB = os.path.join(HERE, "libpvnet_pnp.so")
POSELIB = os.path.join(HERE, "libpvnet_pose.so")
METRICSLIB = os.path.join(HERE, "libpvnet_metrics.so")
VSDLIB = os.path.join(HERE, "libpvnet_vsd.so")
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


def _newer(target, *sources):
    if not os.path.exists(target):
        return False
    t = os.path.getmtime(target)
    return all(os.path.getmtime(s) <= t for s in sources)


def _run(cmd, verbose):
    if verbose:
        print("+", " ".join(cmd), flush=True)
    subprocess.check_call(cmd)


def build_lib(force=False, verbose=False):
    src = os.path.join(CSRC, "pvnet_vote.hip")
    hdr = os.path.join(INCLUDE, "pvnet_vote.h")
    parts = [os.path.join(CSRC, f) for f in sorted(os.listdir(CSRC)) if f.endswith(".hpp")]
    if not force and _newer(LIB, src, hdr, *parts):
        return LIB
    hipcc = shutil.which("hipcc") or os.path.join(ROCM, "bin", "hipcc")
    _run([hipcc, *HIPCC_FLAGS, "-I" + INCLUDE, "-I" + CSRC, "-o", LIB, src], verbose)
    return LIB


def build_nn(force=False, verbose=False):
    """libpvnet_nn.so: the ADD-S nearest-neighbour search (include/pvnet_nn.h), hipcc, no torch."""
    src = os.path.join(CSRC, "pvnet_nn.hip")
    hdr = os.path.join(INCLUDE, "pvnet_nn.h")
    if not force and _newer(NNLIB, src, hdr):
        return NNLIB
    hipcc = shutil.which("hipcc") or os.path.join(ROCM, "bin", "hipcc")
    _run([hipcc, *HIPCC_FLAGS, "-I" + INCLUDE, "-o", NNLIB, src], verbose)
    return NNLIB


def build_metrics(force=False, verbose=False):
    """libpvnet_metrics.so: the batched pose scores (include/pvnet_metrics.h), hipcc, no torch.  The flags of build_nn: the
    ADD-S indices and the stated operation order need -ffp-contract=off."""
    src = os.path.join(CSRC, "pvnet_metrics.hip")
    hdr = os.path.join(INCLUDE, "pvnet_metrics.h")
    if not force and _newer(METRICSLIB, src, hdr):
        return METRICSLIB
    hipcc = shutil.which("hipcc") or os.path.join(ROCM, "bin", "hipcc")
    _run([hipcc, *HIPCC_FLAGS, "-I" + INCLUDE, "-o", METRICSLIB, src], verbose)
    return METRICSLIB


def build_vsd(force=False, verbose=False):
    """libpvnet_vsd.so: the batched depth rasteriser and VSD (include/pvnet_vsd.h), hipcc, no torch.  The flags of
    build_metrics: the device equals the numpy twin bit for bit only with -ffp-contract=off."""
    src = os.path.join(CSRC, "pvnet_vsd.hip")
    hdr = os.path.join(INCLUDE, "pvnet_vsd.h")
    if not force and _newer(VSDLIB, src, hdr):
        return VSDLIB
    hipcc = shutil.which("hipcc") or os.path.join(ROCM, "bin", "hipcc")
    _run([hipcc, *HIPCC_FLAGS, "-I" + INCLUDE, "-o", VSDLIB, src], verbose)
    return VSDLIB


def build_pnp(force=False, verbose=False):
    """libpvnet_pnp.so: the batched uncertainty-PnP refinement (include/pvnet_pnp.h), hipcc, no torch.  binary64
    throughout and not part of the bit-exactness contract: default fp-contract."""
    return _build_pnp_lib("pvnet_pnp", PNPLIB, force, verbose)


def build_pose(force=False, verbose=False):
    """libpvnet_pose.so: the batched pose with its start on the device (include/pvnet_pose.h), the refinement shared with
    libpvnet_pnp.so through csrc/pnp_lm.hpp; hipcc, no torch, flags as build_pnp."""
    return _build_pnp_lib("pvnet_pose", POSELIB, force, verbose)


def _build_pnp_lib(name, target, force, verbose):
    src = os.path.join(CSRC, name + ".hip")
    hdr = os.path.join(INCLUDE, name + ".h")
    if not force and _newer(target, src, hdr, os.path.join(CSRC, "pnp_lm.hpp")):
        return target
    hipcc = shutil.which("hipcc") or os.path.join(ROCM, "bin", "hipcc")
    _run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-shared", "-fvisibility=hidden", "-Wall",
          "-I" + INCLUDE, "-o", target, src], verbose)
    return target


def build_ext(force=False, verbose=False):
    src = os.path.join(CSRC, "ransac_voting_ext.cpp")
    hdr = os.path.join(INCLUDE, "pvnet_vote.h")
    build_lib(verbose=verbose)
    if not force and _newer(EXT, src, hdr, LIB):
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
    return (build_lib(force, verbose), build_ext(force, verbose), build_nn(force, verbose), build_pnp(force, verbose),
            build_pose(force, verbose), build_metrics(force, verbose), build_vsd(force, verbose))


if __name__ == "__main__":
    build_all(force="--force" in sys.argv, verbose=True)
