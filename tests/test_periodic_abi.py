"""Periodic directions at the library boundary, without a GPU: the cross-compiled libraries export the new entries, the
header declares them, and the Python side lists them."""
import ctypes
import os
import re

import pytest

from cubez_amd import lib

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
NEW = ["cz_set_periodic", "czhip_fill_faces_async", "czhip_mg_set_periodic"]


@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_libraries_export_the_periodic_entries(prec):
    h = ctypes.CDLL(lib.lib_path(prec))
    assert not [s for s in NEW if not hasattr(h, s)]


def test_header_declares_them_and_python_lists_them():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "cz_hip.h")).read(), flags=re.S)
    for s in NEW:
        assert re.search(r"\b%s\s*\(" % s, src), s
        assert s in lib.ABI_SYMBOLS, s
    assert re.search(r"int\s+cz_set_periodic\s*\(\s*cz_handle\s*\*\s*,\s*const\s+int\s*\*", src)
    assert "bc_mirror" in lib.LABELS and len(lib.LABELS) == 23  # the fills are timed under the mirror's label: no new one
