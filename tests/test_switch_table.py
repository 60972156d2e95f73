"""CPU check that no configuration switch is without a test: every variable of cubez_amd/csrc/cz_config.h -- read from
czhip_config_describe(0), which does not start the device -- is a row of tests/switch_table.py's SWITCHES (run on the GPU by
tests/test_gpu_switches.py) or an entry of EXEMPT with its reason.  A switch added later without a leg fails here."""
import ctypes
import os
import re
import sys

import pytest

from cubez_amd import lib

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import switch_table as T  # noqa: E402


def _table_names():
    h = ctypes.CDLL(lib.lib_path("f32"))
    h.czhip_config_describe.restype = ctypes.c_char_p
    names = [re.split(r"[ =]", line, 1)[0] for line in h.czhip_config_describe(0).decode().splitlines() if line]
    assert len(names) == len(set(names)) >= 39, names
    return names


def _missing(names, rows, exempt):
    return [n for n in names if n not in {r["var"] for r in rows} and n not in exempt]


def test_every_variable_has_a_leg_or_a_reason():
    names = _table_names()
    assert not _missing(names, T.SWITCHES, T.EXEMPT), _missing(names, T.SWITCHES, T.EXEMPT)
    both = [n for n in T.EXEMPT if n in {r["var"] for r in T.SWITCHES}]
    assert not both, f"exempt and tested: {both}"
    gone = [n for n in list(T.EXEMPT) + [r["var"] for r in T.SWITCHES] if n not in names]
    assert not gone, f"not in cz_config.h: {gone}"
    assert all(isinstance(v, str) and len(v) > 10 and "\n" not in v for v in T.EXEMPT.values())


def test_a_removed_row_is_noticed():
    names = _table_names()
    for var in ("CZHIP_FUSE_FIN", "CZ_COMM_PACK_J", "CZ_FIELD_FORM"):
        assert _missing(names, [r for r in T.SWITCHES if r["var"] != var], T.EXEMPT) == [var]


def test_rows_are_well_formed():
    """every row names known cases, sets its own variable, shows its effect by at least one observable, and the legs the table must hold are there"""
    for r in T.SWITCHES + T.RCCL_ROWS:
        assert r["env"][r["var"]] == r["value"] and all(c in T.CASES for c in r["cases"]), r["id"]
        assert r["cases"] or r.get("rccl"), r["id"]
        assert any(r.get(k) for k in ("tuning", "in_force", "launch", "info")), f"{r['id']}: no observable shows that the switch took effect"
        assert all(T.CASES[c]["iter"] is not None for c in r.get("counters", [])), r["id"]
    ids = [r["id"] for r in T.SWITCHES]
    assert len(ids) == len(set(ids))
    for leg in ("CZHIP_FUSE_FIN=0", "CZHIP_T2=0", "CZHIP_T2=1,1024,2,11", "CZHIP_T2_MAP=0", "CZHIP_T2_MAP=2", "CZHIP_T2_ROWS=0", "CZHIP_T2_KWIN=0", "CZHIP_T2_KWIN=3",
                "CZHIP_T2_PRE=0", "CZHIP_RB4=0", "CZHIP_RB4=1,5,3", "CZHIP_JAC3=0", "CZHIP_JAC3=2", "CZHIP_JAC3=1,5,3", "CZHIP_JAC3_MEDIUM=0", "CZHIP_UNIT_COEF=0",
                "CZHIP_TUNING=512,2,7,0", "CZHIP_PCR=0", "CZHIP_PCR=1,0", "CZHIP_PCR=2,1", "CZHIP_PCR_PIPE=0", "CZHIP_PCR_PIPE=1,2,2,2", "CZHIP_PCR_WG_PER_CU=1",
                "CZHIP_PCR_MAX_WG=4", "CZHIP_PSOR=0", "CZHIP_PSOR=1,1", "CZ_OVERLAP=0", "CZ_LAG_REDUCE=0", "CZ_COMM_CUS=0", "CZ_COMM_CUS=4", "CZ_COMM_CUS=64",
                "CZ_COMM_PACK_J=1", "CZ_COMM_PACK_J=0", "CZ_COMM_ONE_COMM=1", "CZ_BICG_FUSE=0", "CZ_BICG_DEVSC=0", "CZ_BICG_ALIAS=0", "CZ_CG_FUSE=0", "CZ_MG_TAIL=0",
                "CZ_MG_GATHER=1", "CZ_MGRB_ZERO4=0", "CZ_FIELD_FORM=3"):
        assert leg in ids, leg
    assert T.child_timeout([]) == 60.0 and T.child_timeout(list(T.CASES), abi=True) >= 60.0


@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_tuning_describe_needs_no_device(prec):
    """czhip_tuning_describe before any context: ready=0 and the built-in defaults, every value an integer"""
    h = ctypes.CDLL(lib.lib_path(prec))
    t = lib.tuning_in_force(h)
    assert t["ready"] == 0 and t["cu_reserved"] == 0
    assert (t["threads"], t["m"], t["tj"], t["pf"], t["fuse_fin"], t["use_t2"], t["rb4"], t["jac3"], t["pcr_fast"], t["psor_ahead"]) == (512, 2, 16, 0, 1, 1, 1, 1, 2, 0)
