"""The projection step at the library boundary, without a GPU: the cross-compiled libraries export the two entries, the
header declares them, and the Python side lists them."""
import ctypes
import os
import re

import pytest

from cubez_amd import lib

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
NEW = ["cz_set_rhs_div", "cz_sub_grad"]


@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_libraries_export_the_projection_entries(prec):
    h = ctypes.CDLL(lib.lib_path(prec))
    assert not [s for s in NEW if not hasattr(h, s)]


def test_header_declares_them_and_python_lists_them():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "cz_hip.h")).read(), flags=re.S)
    for s in NEW:
        assert re.search(r"\b%s\s*\(" % s, src), s
        assert s in lib.ABI_SYMBOLS, s
    real = r"\s*CZ_REAL\s*\*\s*\w*\s*,"
    assert re.search(r"int\s+cz_set_rhs_div\s*\(\s*cz_handle\s*\*\s*,(\s*const" + real + r"){3}\s*const\s+long\s+long\s*\*", src)
    assert re.search(r"int\s+cz_sub_grad\s*\(\s*cz_handle\s*\*\s*,(" + real + r"){3}\s*const\s+long\s+long\s*\*", src)
    assert "field_io" in lib.LABELS and len(lib.LABELS) == 23  # the kernels are timed under the import's label: no new one


def test_the_driver_class_has_the_three_methods():
    from cubez_amd import CZ
    assert all(callable(getattr(CZ, n, None)) for n in ("set_rhs_div", "sub_grad", "project"))
