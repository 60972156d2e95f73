"""The closed box at the library boundary, without a GPU: the cross-compiled libraries export the new entries, the header
declares them, and the Python side lists them."""
import ctypes
import os
import re

import pytest

from cubez_amd import lib

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
NEW = ["cz_set_closed_box", "cz_closed_mean", "czhip_shift_sums_async", "czhip_cg_update_closed_async"]


@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_libraries_export_the_closed_box_entries(prec):
    h = ctypes.CDLL(lib.lib_path(prec))
    assert not [s for s in NEW if not hasattr(h, s)]


def test_header_declares_them_and_python_lists_them():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "cz_hip.h")).read(), flags=re.S)
    for s in NEW:
        assert re.search(r"\b%s\s*\(" % s, src), s
        assert s in lib.ABI_SYMBOLS, s
    assert re.search(r"double\s+cz_closed_mean\s*\(\s*cz_handle\s*\*\s*,\s*int", src)
    assert lib.LABELS[-2:] == ("shift_sums", "cg_update_closed")
