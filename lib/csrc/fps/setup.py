"""``python setup.py build_ext --inplace`` -- the command the reference's README documents for this directory
(lib/csrc/fps/setup.py).  The reference compiles its C++ extension here; this one builds ``libpvnet_vote.so``, whose last
section holds the sampling kernels, in place, next to the package, through ``clean-pvnet_amd/_build.py`` -- the same thing
``python __graft_entry__.py`` does.  Any other setup.py command is refused: nothing here is meant to be installed into
site-packages."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))


def main(argv):
    if "build_ext" not in argv:
        sys.exit("usage: python setup.py build_ext --inplace   (builds libpvnet_vote.so in clean-pvnet_amd/)")
    sys.path.insert(0, ROOT)
    from lib import build_in_place
    build_in_place("vote")


if __name__ == "__main__":
    main(sys.argv[1:])
