"""Loader of the committed golden fixtures (tests/golden/*.npz, written by tests/golden/make_golden.py)."""
import os

import numpy as np

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def load(name):
    """tests/golden/<name>.npz as a dict of arrays.  An array whose images repeat is stored once per distinct image, as
    ``<key>_rows`` plus the index list ``<key>_take``, to keep the file under the size limit of a committed file; it is
    returned whole, as ``<key>`` = ``rows[take]``."""
    c = dict(np.load(os.path.join(GOLD, name + ".npz")))
    for key in [k[:-len("_rows")] for k in c if k.endswith("_rows")]:
        c[key] = c.pop(key + "_rows")[c.pop(key + "_take")]
    return c
