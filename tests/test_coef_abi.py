"""Face coefficients at the library boundary, without a GPU: the cross-compiled libraries export the entry, the header
declares it, and the Python side lists it."""
import ctypes
import os
import re

import pytest

from cubez_amd import lib

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
NEW = "cz_set_face_coef"


@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_libraries_export_the_entry(prec):
    assert hasattr(ctypes.CDLL(lib.lib_path(prec)), NEW)


def test_header_declares_it_and_python_lists_it():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "cz_hip.h")).read(), flags=re.S)
    real = r"\s*const\s+CZ_REAL\s*\*\s*\w*\s*,"
    assert re.search(r"int\s+cz_set_face_coef\s*\(\s*cz_handle\s*\*\s*,(" + real + r"){3}\s*const\s+long\s+long\s*\*\s*\w*\s*,\s*int\s+\w*\s*,\s*void\s*\*", src)
    assert NEW in lib.ABI_SYMBOLS
    # no new timing label: the SpMV runs under calc_ax, the residual under calc_rk, import / check / gradient under field_io, the scaling under ewise
    assert len(lib.LABELS) == 23 and all(n in lib.LABELS for n in ("calc_ax", "calc_rk", "field_io", "ewise"))


def test_the_driver_classes_have_the_method():
    from cubez_amd import CZ
    from cubez_amd.refine import Refined
    assert callable(getattr(CZ, "set_face_coef", None)) and callable(getattr(Refined, "set_face_coef", None))
