"""The table behind tests/test_gpu_switches.py and tests/test_switch_table.py: every environment variable of cubez_amd/csrc/cz_config.h is either
a row of SWITCHES -- the variable in the environment of a fresh child process (tests/switch_worker.py), the cases the child solves, and the
observable that proves the other path ran -- or an entry of EXEMPT with the reason.  Nothing here touches the GPU or loads the library.

A row:
  var, value   the switch and its alternate value; env = what the child's environment gets (the switch, and a partner where the switch
               only shows beside one: CZHIP_JAC3_MEDIUM needs jac3_k on a small grid, CZHIP_TUNING the single sweeps)
  cases        names of CASES the child runs
  tuning       czhip_tuning_describe values the child must report (what czhip_init's parse made of the value)
  in_force     cz_config_in_force values every driver of the child must report; an int, or a string naming a rule of test_gpu_switches.py
  launch       {case or "*": {label: rule}} on the launch counts of czhip_timing_read: an int, ">0", "sweeps" (one launch per sweep: every
               recorded iteration, and at most two poll periods of launches that found the flag set -- the host looks every 32 iterations
               and reads the look before), ">default" / "default" (against the default-environment leg of the same case)
  info         {case or "*": {key: value}} on cz_info
  counters     the landing cases whose own counters (the path they name) hold in this leg too
  abi          True: the child also runs the C-ABI checks (drop-in symbols and checked launches) under the switch
  also         an existing test that sets the same value through the environment, where there is one

Every leg, whatever its row says: stationary cases equal the wide-accumulating oracle (field bit for bit, iteration count, history and res to
the bars of test_gpu_convergence_landing.py); Krylov cases equal the default-environment leg byte for byte (field, history, count), which
test_default_leg holds to the exact-dot oracle bit for bit -- they are the FP32 cases of bicg_parity / cg_parity / mg_parity / mgrb_parity whose
premise (no summation order of a dot product can flip a rounding; tests/test_oracle.py, test_cg_oracle.py, test_mg_oracle.py,
test_mgrb_oracle.py) makes that the bar for EVERY switch, "same bits" in the table or not."""
import json
import os

HERE = os.path.dirname(os.path.abspath(__file__))
with open(os.path.join(HERE, "golden", "landing_cases.json")) as _f:
    _LANDING = {c["name"]: c for c in json.load(_f)["cases"]}


def _landing(name):
    c = _LANDING[name]
    return dict(family="stationary", prec=c["prec"], gsz=tuple(c["gsz"]), solver=c["solver"], itr_max=c["itr_max"], coef=c["coef"], pc=None,
                div=tuple(c["div"]) if "div" in c else None, iter=c["iter"], counters=c["counters"])


def _fixed(prec, gsz, solver, itr_max, coef):
    return dict(family="stationary", prec=prec, gsz=tuple(gsz), solver=solver, itr_max=itr_max, coef=coef, pc=None, div=None, iter=None, counters={})


def _krylov(module, cid, div=None):
    """a case of tests/{bicg,cg,mg,mgrb}_parity.py by its id; K iterations (ItrMax as that module's GPU test sets it)"""
    return dict(family="krylov", module=module, id=cid, div=div)


CASES = {
    # -- tests/golden/landing_cases.json: converge at a pinned position; the default environment takes the path their `switches` name
    "jacobi_pair_sweep1_poll_last": _landing("jacobi_pair_sweep1_poll_last"),
    "jacobi_pair_sweep2_poll_last": _landing("jacobi_pair_sweep2_poll_last"),
    "sor2sma_one_poll_last": _landing("sor2sma_one_poll_last"),
    "sor2sma_one_poll_first": _landing("sor2sma_one_poll_first"),
    "jacobi_maf_sweep1": _landing("jacobi_maf_sweep1"),
    "sor2sma_maf": _landing("sor2sma_maf"),
    "psor_poll_last": _landing("psor_poll_last"),
    "pcr_rb": _landing("pcr_rb"),
    "jacobi_single_poll_last": _landing("jacobi_single_poll_last"),                  # CZHIP_T2=0 is its `switches`
    "jacobi_triple_sweep1_poll_last": _landing("jacobi_triple_sweep1_poll_last"),    # CZHIP_JAC3=2 is its `switches`
    "jacobi_decomposed_2x1x1_lag1_sweep1": _landing("jacobi_decomposed_2x1x1_lag1_sweep1"),
    "jacobi_decomposed_1x2x2_lag1_sweep1": _landing("jacobi_decomposed_1x2x2_lag1_sweep1"),
    "jacobi_decomposed_2x1x1_lag0_sweep1": _landing("jacobi_decomposed_2x1x1_lag0_sweep1"),  # CZ_LAG_REDUCE=0 is their `lag_reduce`
    "jacobi_decomposed_1x2x2_lag0_sweep1": _landing("jacobi_decomposed_1x2x2_lag0_sweep1"),
    # -- fixed iteration counts on the boxes of test_gpu_pass_contract.py (rows of 65 values: no multiple of the vector width; rows of 1104:
    # cut into k windows), and the line / point SOR names on 16^3 and 9 x 7 x 12
    "jacobi_40x36x61_f32": _fixed("f32", (40, 36, 61), "jacobi", 12, 0.9),
    "sor2sma_40x36x61_f64": _fixed("f64", (40, 36, 61), "sor2sma", 9, 1.3),
    "jacobi_9x7x1100_f32": _fixed("f32", (9, 7, 1100), "jacobi", 9, 0.9),
    "sor2sma_9x7x1100_f64": _fixed("f64", (9, 7, 1100), "sor2sma", 8, 1.3),
    "psor_9x7x12_f32": _fixed("f32", (9, 7, 12), "psor", 10, 1.2),
    "pcr_16_f32": _fixed("f32", (16, 16, 16), "pcr", 10, 1.1),
    "pcr_esa_9x7x12_f64": _fixed("f64", (9, 7, 12), "pcr_esa", 8, 1.1),
    # -- Krylov solvers: FP32 cases whose premise is checked on the CPU
    "bicg_jacobi": _krylov("bicg_parity", "pbicgstab_jacobi_9x7x12_f32_K3"),
    "bicg_sor2sma": _krylov("bicg_parity", "pbicgstab_sor2sma_40x36x61_f32_K5"),
    "bicg_none": _krylov("bicg_parity", "pbicgstab_none_33x47x61_f32_K5"),
    "pcg_jacobi": _krylov("cg_parity", "pcg_jacobi_33x47x61_f32_K5"),
    "pcg_mg": _krylov("mg_parity", "pcg_mg_33x47x61_f32_K4"),
    "pcg_mgrb": _krylov("mgrb_parity", "pcg_mgrb_33x47x61_f32_K4_w1.2"),
    "pcg_mg_2x1x2": _krylov("mg_parity", "pcg_mg_33x47x61_f32_K4", div=(2, 1, 2)),
}

JAC = ["jacobi_pair_sweep1_poll_last", "jacobi_pair_sweep2_poll_last", "jacobi_40x36x61_f32", "jacobi_9x7x1100_f32", "jacobi_maf_sweep1"]
RB = ["sor2sma_one_poll_last", "sor2sma_one_poll_first", "sor2sma_40x36x61_f64", "sor2sma_9x7x1100_f64", "sor2sma_maf"]
LINE = ["pcr_rb", "pcr_16_f32", "pcr_esa_9x7x12_f64"]
LEX = ["pcr_16_f32", "pcr_esa_9x7x12_f64"]
POINT = ["psor_poll_last", "psor_9x7x12_f32"]
BICG = ["bicg_jacobi", "bicg_sor2sma", "bicg_none"]
PCG = ["pcg_jacobi", "pcg_mg", "pcg_mgrb"]
DEC = ["jacobi_decomposed_2x1x1_lag1_sweep1", "jacobi_decomposed_1x2x2_lag1_sweep1"]
DEC0 = ["jacobi_decomposed_2x1x1_lag0_sweep1", "jacobi_decomposed_1x2x2_lag0_sweep1"]
DEFAULT_CASES = [n for n in CASES if n not in ("jacobi_single_poll_last", "jacobi_triple_sweep1_poll_last") + tuple(DEC0)]
FUSED_LABELS = {"jacobi2": 0, "jacobi3": 0, "rbsor2": 0, "rbsor4": 0, "pair_shell": 0}
PLAIN_JAC = ["jacobi_pair_sweep1_poll_last", "jacobi_pair_sweep2_poll_last", "jacobi_40x36x61_f32", "jacobi_9x7x1100_f32"]


def _row(var, value, cases, env=None, **kw):
    return dict(var=var, value=value, env=dict(env or {}, **{var: value}), cases=list(cases), id=f"{var}={value}", **kw)


SWITCHES = [
    # ---- kernels (czhip_init)
    _row("CZHIP_FUSE_FIN", "0", JAC + RB + LINE + POINT + BICG + PCG + DEC[:1], abi=True, tuning=dict(fuse_fin=0),
         launch={"*": FUSED_LABELS, **{c: dict(FUSED_LABELS, reduce=">0") for c in JAC + RB}}, info={"*": dict(rb4_passes=0, jac3_passes=0, bicg_fused=0)}),
    _row("CZHIP_T2", "0", JAC + RB + ["jacobi_single_poll_last"], abi=True, tuning=dict(use_t2=0), counters=["jacobi_single_poll_last"],
         launch={"*": dict(jacobi2=0, jacobi3=0), **{c: dict(jacobi2=0, jacobi3=0, jacobi="sweeps") for c in PLAIN_JAC + ["jacobi_single_poll_last"]}}),
    _row("CZHIP_T2", "1,1024,2,11", JAC + RB, tuning=dict(use_t2=1, t2_threads=1024, t2_mv=2, t2_tj=11),
         launch={c: dict(jacobi2=">0") for c in PLAIN_JAC}),
    _row("CZHIP_T2_MAP", "0", JAC + RB + ["bicg_sor2sma"], tuning=dict(t2_map=0), launch={c: dict(jacobi2=">0") for c in PLAIN_JAC}),
    _row("CZHIP_T2_MAP", "2", JAC + RB + ["bicg_sor2sma"], tuning=dict(t2_map=2), launch={c: dict(jacobi2=">0") for c in PLAIN_JAC}),
    _row("CZHIP_T2_ROWS", "0", JAC + RB, tuning=dict(t2_any_rows=0), also="test_gpu_cli.py::test_scalar_kernels_of_rounds_1_and_2_give_the_history_of_the_vector_kernels",
         launch={"jacobi_40x36x61_f32": dict(jacobi2=0, jacobi="sweeps"), "sor2sma_40x36x61_f64": dict(rbsor2=0), "jacobi_9x7x1100_f32": dict(jacobi2=">0")}),
    _row("CZHIP_T2_KWIN", "0", JAC + RB, tuning=dict(t2_kwin=0), launch={"jacobi_9x7x1100_f32": dict(jacobi2=">0")}),
    _row("CZHIP_T2_KWIN", "3", JAC + RB, tuning=dict(t2_kwin=3), launch={"jacobi_9x7x1100_f32": dict(jacobi2=">0")},
         also="test_gpu_decomp.py::test_decomposed_bricks_in_every_form_of_the_pass"),
    _row("CZHIP_T2_PRE", "0", JAC + RB, tuning=dict(t2_pre=0), launch={c: dict(jacobi2=">0") for c in PLAIN_JAC},
         also="test_gpu_decomp.py::test_decomposed_bricks_in_every_form_of_the_pass"),
    _row("CZHIP_RB4", "0", RB, tuning=dict(rb4=0, rb4_kwin=0, rb4_tj=0), launch={"*": dict(rbsor4=0)}, info={"*": dict(rb4_passes=0)}),
    _row("CZHIP_RB4", "1,5,3", RB, tuning=dict(rb4=1, rb4_kwin=5, rb4_tj=3), launch={"*": dict(rbsor4="default")}),
    _row("CZHIP_JAC3", "0", JAC, tuning=dict(jac3=0, jac3_kwin=0, jac3_tj=0), launch={"*": dict(jacobi3=0)}, info={"*": dict(jac3_passes=0)}),
    _row("CZHIP_JAC3", "2", JAC + ["jacobi_triple_sweep1_poll_last"], tuning=dict(jac3=2, jac3_kwin=0, jac3_tj=0), counters=["jacobi_triple_sweep1_poll_last"],
         launch={c: dict(jacobi3=">0") for c in PLAIN_JAC + ["jacobi_triple_sweep1_poll_last"]}),
    _row("CZHIP_JAC3", "1,5,3", JAC, tuning=dict(jac3=1, jac3_kwin=5, jac3_tj=3), launch={"*": dict(jacobi3="default")}),
    _row("CZHIP_JAC3_MEDIUM", "0", PLAIN_JAC, env={"CZHIP_JAC3": "2"}, tuning=dict(jac3=2, jac3_medium=0),
         launch={c: dict(jacobi3=">0") for c in PLAIN_JAC}, also="test_gpu_jac3_forms.py::test_off_switch"),
    _row("CZHIP_UNIT_COEF", "0", PLAIN_JAC + RB[:4], tuning=dict(unit_coef=0), launch={c: dict(jacobi2=">0") for c in PLAIN_JAC}),
    _row("CZHIP_TUNING", "512,2,7,0", JAC + RB + ["pcg_jacobi"], env={"CZHIP_T2": "0"}, tuning=dict(threads=512, m=2, tj=7, pf=0, use_t2=0),
         launch={c: dict(jacobi="sweeps", jacobi2=0) for c in PLAIN_JAC}),
    _row("CZHIP_PCR", "0", LINE, tuning=dict(pcr_fast=0, pcr_variant=0), launch={"*": dict(pcr_rb=">0")}),
    _row("CZHIP_PCR", "1,0", LINE, tuning=dict(pcr_fast=1, pcr_variant=0), launch={"*": dict(pcr_rb=">0")}),
    _row("CZHIP_PCR", "2,1", LINE, tuning=dict(pcr_fast=2, pcr_variant=1), launch={"*": dict(pcr_rb=">0")}),
    _row("CZHIP_PCR_PIPE", "0", LEX, tuning=dict(pcr_pipe=0), launch={"*": dict(pcr_rb=">default")}),
    _row("CZHIP_PCR_PIPE", "1,2,2,2", LEX, tuning=dict(pcr_pipe=1, pipe_spin_ticks=200000000, pcr_rows=2, pcr_q=2), launch={"*": dict(pcr_rb="default")}),
    _row("CZHIP_PCR_WG_PER_CU", "1", LEX, tuning=dict(pcr_wg_per_cu=1), launch={"*": dict(pcr_rb="default")}),
    _row("CZHIP_PCR_MAX_WG", "4", LEX, tuning=dict(pcr_max_wg=4, pcr_slots=0), launch={"*": dict(pcr_rb="default")}),
    _row("CZHIP_PSOR", "0", POINT, tuning=dict(psor_col=0), launch={"*": dict(psor="default")}),   # (the label counts sweeps, not tile launches)
    _row("CZHIP_PSOR", "1,1", POINT, tuning=dict(psor_col=1, psor_wg_per_cu=1), launch={"*": dict(psor="default")}),
    # ---- driver (CZ)
    _row("CZ_OVERLAP", "0", DEC, in_force=dict(overlap=0), launch={"*": dict(pair_shell=0, jacobi2=">0")}, info={"*": dict(overlap=0)},
         also="test_gpu_decomp.py::test_decomposed_equals_single_domain[serial]"),
    _row("CZ_LAG_REDUCE", "0", DEC0, in_force=dict(lag_reduce=0), counters=DEC0, also="test_gpu_convergence_landing.py::test_decomposed_landing"),
    _row("CZ_COMM_CUS", "0", DEC, in_force=dict(comm_cus=0, comm_cus_reserved=0), tuning=dict(cu_reserved=0), info={"*": dict(comm_cus=0)}),
    _row("CZ_COMM_CUS", "4", DEC, in_force=dict(comm_cus=4, comm_cus_reserved="clamped"), tuning=dict(cu_reserved="clamped"), info={"*": dict(comm_cus="clamped")}),
    _row("CZ_COMM_CUS", "64", DEC, in_force=dict(comm_cus=64, comm_cus_reserved="clamped"), tuning=dict(cu_reserved="clamped"), info={"*": dict(comm_cus="clamped")}),
    _row("CZ_BICG_FUSE", "0", BICG, in_force=dict(bicg_fuse=0), info={"*": dict(bicg_fused=0)},
         also="test_gpu_bicgstab_parity.py::test_bicgstab_switch_off_vs_exact_dot_oracle"),
    _row("CZ_BICG_DEVSC", "0", BICG, in_force=dict(bicg_devsc=0), also="test_gpu_bicgstab_parity.py::test_bicgstab_switch_off_vs_exact_dot_oracle"),
    _row("CZ_BICG_ALIAS", "0", BICG, in_force=dict(bicg_alias=0),  # (the copies it brings back carry no timing label)
         also="test_gpu_bicgstab_parity.py::test_bicgstab_switch_off_vs_exact_dot_oracle"),
    _row("CZ_CG_FUSE", "0", PCG, in_force=dict(cg_fuse=0), info={"*": dict(cg_fused=0)}, also="test_gpu_pcg.py::test_pcg_unfused_vs_exact_dot_oracle"),
    _row("CZ_MG_TAIL", "0", ["pcg_mg", "pcg_mgrb"], in_force=dict(mg_tail=0), launch={"*": dict(mg_tail=0)}, also="test_gpu_mg.py::test_apply_equals_restated_vcycle"),
    _row("CZ_MG_GATHER", "1", ["pcg_mg_2x1x2"], in_force=dict(mg_gather=1), info={"*": dict(mg_gather_level="gather_level")},
         also="test_gpu_mg_decomp.py::test_distributed_cycle_equals_single_domain"),
    _row("CZ_MGRB_ZERO4", "0", ["pcg_mgrb"], in_force=dict(mgrb_zero4=0), launch={"*": dict(rbsor4=0, rbsor2="default")}, also="test_gpu_mgrb.py::test_level0_through_every_pass_gives_equal_bits"),
    _row("CZ_FIELD_FORM", "3", ["jacobi_40x36x61_f32", "sor2sma_40x36x61_f64"], in_force=dict(field_form=3), info={"*": dict(field_form=3)},
         also="test_gpu_problem.py::test_import_and_export_move_exactly_the_brick"),
    # ---- transport (cz_comm.cpp)
    _row("CZ_COMM_PACK_J", "1", DEC, in_force=dict(comm_pack_j=1, comm_direct_messages=0)),
    _row("CZ_COMM_PACK_J", "0", DEC, in_force=dict(comm_pack_j=0, comm_direct_messages="default")),   # 0 behaves as unset
    _row("CZ_COMM_ONE_COMM", "1", [], rccl=True, in_force=dict(comm_one_comm=1)),
]
# the second RCCL-only leg: packed J faces through ncclSend / ncclRecv from the pack buffers
RCCL_ROWS = [r for r in SWITCHES if r.get("rccl")] + [_row("CZ_COMM_PACK_J", "1", [], rccl=True, in_force=dict(comm_pack_j=1, comm_direct_messages=0))]
RCCL_CASE = ("f32", (40, 36, 44), "jacobi", 12, 0.8, (1, 2, 1))   # tests/test_gpu_rccl.py's J-face case, two ranks on one GPU

EXEMPT = {
    "RANK": "launcher: which rank this process is (test_gpu_cli.py, test_gpu_rccl.py run the launcher's protocol)",
    "WORLD_SIZE": "launcher: number of ranks",
    "LOCAL_RANK": "launcher: selects the GPU; a one-GPU box has one value",
    "MASTER_ADDR": "launcher: job key of the communicator-id record",
    "MASTER_PORT": "launcher: job key / default id file",
    "CZ_JOB_ID": "launcher: job key of the communicator-id record",
    "CZ_COMM_ID_FILE": "launcher: where rank 0 leaves the RCCL id",
    "CZ_COMM_DEBUG": "prints what a run decided and arms the watchdog; computes nothing (set by every run of test_gpu_rccl.py)",
    "CZ_COMM_TIMEOUT": "a time limit of the collectives; a leg would have to wait for it",
    "CZ_TEST_SKEW": "test aid that delays one rank; its effect is a delay",
    "CZ_FATAL_LOG": "where a fatal exit is logged: test_abi.py::test_a_fatal_exit_of_the_library_leaves_a_line",
    "CZ_SPH": "tested through the command line (test_gpu_cli.py)",
    "CZ_PROFILE": "tested through the command line (test_gpu_cli.py)",
    "CZHIP_PCR_PIPE_PROF": "development builds only (-DCZ_LEX_PROF)",
    "CZHIP_PCR_SLOTS": "a ring forced small makes the sweep give up, which test_gpu_kernels.py covers through czhip_set_pcr_lex_limits; no leg forces a give-up",
}

# Wall time [s] on an MI355X of a default-environment child (switch_worker.py records it): its start (imports, library load; the first case
# carries the context's start), each case, the C-ABI checks, and the two RCCL ranks.  A child's time limit is ten times the sum for its
# cases, at least 60 s -- with these figures (the whole default child: 1.4 s) every limit is the 60 s floor.
CHILD_START_SECONDS = 0.5
ABI_SECONDS = 0.6
CASE_SECONDS = dict({n: 0.05 for n in CASES}, jacobi_pair_sweep1_poll_last=0.3, jacobi_decomposed_2x1x1_lag1_sweep1=0.45, jacobi_decomposed_1x2x2_lag1_sweep1=0.22,
                    jacobi_decomposed_2x1x1_lag0_sweep1=0.42, jacobi_decomposed_1x2x2_lag0_sweep1=0.18, pcg_mg_2x1x2=0.37)
RCCL_SECONDS = 6.0


def child_timeout(cases, abi=False):
    return max(60.0, 10.0 * (CHILD_START_SECONDS + sum(CASE_SECONDS[n] for n in cases) + (ABI_SECONDS if abi else 0.0)))
