"""``python setup.py build_ext --inplace`` -- the command the reference's README documents for this directory
(/root/reference/README.md:41-44, lib/csrc/uncertainty_pnp/setup.py).  The reference compiles its CUDA extension here; this
one builds the native libraries of clean-pvnet_amd (hipcc --offload-arch=gfx950 + the host shim) in place, next to the
package, through ``clean-pvnet_amd/_build.py`` -- the same thing ``python __graft_entry__.py`` does.  Any other
setup.py command is refused: nothing here is meant to be installed into site-packages."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))


def main(argv):
    if "build_ext" not in argv:
        sys.exit("usage: python setup.py build_ext --inplace   (builds libpvnet_pnp.so and libpvnet_pose.so in clean-pvnet_amd/)")
    sys.path.insert(0, ROOT)
    from lib import build_in_place
    build_in_place("pnp", "pose")


if __name__ == "__main__":
    main(sys.argv[1:])
