"""Drop-in import path of the reference's DCNv2 extension: ``from lib.csrc.dcn_v2 import _ext`` (lib/networks/dcn_v2.py:13)."""
