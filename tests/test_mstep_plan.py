"""The M-step's plan (bayesml_amd/csrc/mstep_plan.h: mstep_needs_counters, plan_mstep) without a GPU.

tests/mstep_plan_cases.cpp includes only that header; it is built here by the host compiler with AddressSanitizer and UBSan
and run once over every case below.  The expected values were worked out by hand from gmmvb_mstep as it stood before the
decision was moved out of it, read line by line - not from the new code; the arithmetic is written next to the cases.
Nothing is loaded into Python.

The facts are set directly: components per workgroup (kpw_pre = 4, kpw_raw = 2) are chosen to differ so that a mixed-up
`pre` shows, and S_cap / split_rows are whatever makes a clamp bite - a real workspace's S_cap is at least
ceil(max_rows / split_rows), so it only reaches the split_rows clamp through the rounding of rows_per_split to 64
(profiles/capi_mstep.md).  Every list plan has qpart = 1: the lists need E-step output (e_state 1), the only state in which
the builders of delta and mmask lists are handed the per-block counts."""
import os
import subprocess

from test_pass_plan import HERE, host_compiler

GENERIC, MFMA, SMALL, HMM_SMALL, WIDE, LISTS = range(6)                 # kind
CENTRED, XP32, X32 = range(3)                                           # rows
NONE, MMASK, MASKS = range(3)                                           # build
R_GENERIC, R_STATS, R_CHUNKS = range(3)                                 # reduce
OK, ESTATE = 0, 5
NO_RESP = "no responsibilities for these rows: call gmmvb_estep or gmmvb_load_responsibilities first"
REGROUPED = "the workspace's rows are regrouped for another sample matrix: call gmmvb_prepare_rows first"
PRUNED = "a pruned E-step needs the list M-step over the matrix of the E-step (gmmvb_prepare_rows)"
SETTLED = "settled rows need the list M-step over the matrix of the E-step (gmmvb_prepare_rows)"
LOST = "the M-step's lists were used by a read-out of settled rows: call gmmvb_estep again"

# loaded responsibilities over rows nobody prepared
BASE = "K=6 D=64 T=4 n_rows=6000 e_rows=6000 ldx=64 S_cap=176 split_rows=32768 kpw_pre=4 kpw_raw=2 list_m_below=0.5 e_state=2 has_xc=1 f64=0 vec=1"
GEN = "generic=1 D=257 T=17 K=3 e_state=1"
PRE = "xc_of_x=1"
ONE_TILE = "T=1 D=16 K=70 xc_of_x=1"
WIDE_ROWS = "wide=1 D=129 T=10 K=4 n_rows=600 e_rows=600 kpw_pre=1 kpw_raw=1 S_cap=256 split_rows=13120"
# E-step output of a pruned pass over prepared f32 rows
LIST = "K=8 e_state=1 act_rows=6000 sparse=1 has_masks=1 xc_of_x=1 rec_live=1"
# ... and of a counted dense pass
COUNTED = LIST + " rec_live=0 lag_valid=1 lag_act=0.1*n_rows*K"
CACHE = LIST + " lock_live=1"


def rows(n):
    return f"n_rows={n} e_rows={n}"


CASES = [
    # ---- entry
    ("e_state=0", dict(status=ESTATE, message=NO_RESP, needs_counters=0, need_row_lse=0)),
    ("e_state=4", dict(status=ESTATE, message=NO_RESP)),
    ("e_state=1 e_rows=5999", dict(status=ESTATE, message=NO_RESP)),
    ("e_state=0 lse_stale=1", dict(status=ESTATE, need_row_lse=0)),
    ("e_state=1 lse_stale=1", dict(status=OK, message="", need_row_lse=1)),
    ("e_state=2 lse_stale=1", dict(status=OK, need_row_lse=0)),
    (GEN + " lse_stale=1", dict(status=OK, need_row_lse=1)),
    # ---- generic: rps = round_up(ceil(n / gen_S), 64), S = ceil(n / rps)
    (GEN + " gen_S=1 " + rows(1), dict(kind=GENERIC, S=1, rows_per_split=64, reduce=R_GENERIC, counter=5, needs_counters=0)),
    (GEN + " gen_S=1 " + rows(64), dict(S=1, rows_per_split=64)),
    (GEN + " gen_S=1 " + rows(65), dict(S=1, rows_per_split=128)),
    (GEN + " gen_S=1 " + rows(32769), dict(S=1, rows_per_split=32832)),
    (GEN + " gen_S=2 " + rows(1), dict(S=1, rows_per_split=64)),
    (GEN + " gen_S=2 " + rows(64), dict(S=1, rows_per_split=64)),
    (GEN + " gen_S=2 " + rows(65), dict(S=2, rows_per_split=64)),                 # ceil(65 / 2) = 33 -> 64
    (GEN + " gen_S=2 " + rows(32769), dict(S=2, rows_per_split=16448)),           # ceil(32769 / 2) = 16385 -> 16448
    (GEN + " e_state=1", dict(direct_r=0, gamma_weights=0, aux_lnrho=0, need_gamma_cm=0)),
    (GEN + " e_state=2", dict(direct_r=1, gamma_weights=0, aux_lnrho=0, need_gamma_cm=0)),
    (GEN + " e_state=3", dict(direct_r=2, gamma_weights=1, aux_lnrho=1, need_gamma_cm=1)),
    (GEN + " e_state=3 hmm_skip_h=1", dict(direct_r=2, aux_lnrho=0, need_gamma_cm=1)),
    (GEN + " e_state=3 hmm_no_lnrho=1", dict(aux_lnrho=1)),                       # (the generic path does not look at it)
    (GEN + " e_state=2 sorted=1", dict(status=OK)),                               # ... nor at the row order
    # ---- dense geometry.  6000 rows: 94 groups of 64 < S_cap; rps = round_up(ceil(6000 / 94), 64) = 64; S = 94
    ("", dict(status=OK, kind=MFMA, pre=0, S=94, rows_per_split=64, KG=3, KGW=0, grid=8 * 12 * 3, direct_r=1, may_calibrate=0,
              reduce=R_STATS, counter=5, elems=10 * 256 + 64 + 2, needs_counters=0, need_recenter=0, add_cache=0)),
    (PRE, dict(kind=MFMA, pre=1, S=94, KG=2, grid=8 * 12 * 2)),
    (rows(65), dict(S=2, rows_per_split=64, grid=8 * 1 * 3)),                     # S clamped by the 64-row groups
    (rows(1), dict(S=1, rows_per_split=64, grid=8 * 1 * 3)),
    (rows(20000), dict(S=157, rows_per_split=128, grid=8 * 20 * 3)),              # S_cap: ceil(20000 / 176) = 114 -> 128
    # rows_per_split clamped by split_rows: ceil(600000 / 8) = 75000 -> 75008 > 32768; S = ceil(600000 / 32768) = 19
    ("S_cap=8 " + rows(600000), dict(S=19, rows_per_split=32768, grid=8 * 3 * 3)),
    ("S_cap=8 split_rows=0 " + rows(600000), dict(S=8, rows_per_split=75008, grid=8 * 1 * 3)),
    ("e_state=1", dict(direct_r=0, may_calibrate=1, gamma_weights=0, aux_lnrho=0)),
    ("e_state=3", dict(direct_r=2, may_calibrate=0, gamma_weights=1, aux_lnrho=1, need_gamma_cm=1, kind=MFMA)),
    ("e_state=3 hmm_no_lnrho=1", dict(aux_lnrho=0, need_gamma_cm=1)),
    ("e_state=3 hmm_skip_h=1", dict(aux_lnrho=0, direct_r=2)),
    (PRE + " e_state=3", dict(kind=MFMA, need_gamma_cm=1)),
    # one feature tile over the centred copy: 32 components per workgroup; KG stays what the argument block carries
    (ONE_TILE, dict(kind=SMALL, KGW=3, KG=18, grid=8 * 12 * 3, may_calibrate=0, hmm_sparse_walk=0)),
    (ONE_TILE + " K=32", dict(KGW=1, grid=8 * 12 * 1)),
    (ONE_TILE + " K=33", dict(KGW=2, grid=8 * 12 * 2)),
    (ONE_TILE + " e_state=1", dict(kind=SMALL, may_calibrate=0)),
    (ONE_TILE + " e_state=3", dict(kind=HMM_SMALL, need_gamma_cm=0, gamma_weights=1, hmm_sparse_walk=1, KGW=3, direct_r=2)),
    (ONE_TILE + " e_state=3 opt_hmm_mstep_dense=1", dict(kind=HMM_SMALL, hmm_sparse_walk=0)),
    (ONE_TILE + " e_state=3 xc_of_x=0", dict(kind=MFMA, need_gamma_cm=1, KGW=0, KG=35, grid=8 * 12 * 35)),
    (ONE_TILE + " xc_of_x=0", dict(kind=MFMA, KGW=0)),
    # ---- wide and row order.  600 rows: 10 groups; rps = 64; S = 10; one component per workgroup
    (WIDE_ROWS, dict(status=OK, kind=WIDE, need_prepare=1, pre=1, S=10, KG=4, grid=8 * 2 * 4, need_recenter=0)),
    (WIDE_ROWS + " sorted=1 xc_stale=1", dict(status=OK, need_prepare=1, pre=1, need_recenter=0)),      # the fresh copy is neither
    (WIDE_ROWS + " xc_of_x=1", dict(kind=WIDE, need_prepare=0, pre=1)),
    (WIDE_ROWS + " xc_of_x=1 xc_stale=1", dict(need_prepare=0, need_recenter=1)),
    ("sorted=1", dict(status=ESTATE, message=REGROUPED, needs_counters=0, need_prepare=0)),
    ("sorted=1 e_state=3", dict(status=ESTATE, message=REGROUPED, need_gamma_cm=1)),      # (the transpose is on its way by then)
    (PRE + " sorted=1", dict(status=OK, pre=1)),
    (PRE + " xc_stale=1", dict(need_recenter=1)),
    ("xc_stale=1", dict(need_recenter=0)),
    # ---- lists: eligibility.  48000 pairs; at most ceil(48000 / 1024) + 8 = 55 chunks -> ceil(55 / 4) = 14 workgroups
    (LIST, dict(status=OK, kind=LISTS, needs_counters=0, counter=6, pre=1, cap_chunks=176 * 8, r_min=1024, lgrid=14, grid=14, S=0,
                rows_per_split=1024, reduce=R_CHUNKS, add_cache=0, apply_delta=0, build=MASKS, active_lists=1, clear_blk_fresh=1,
                qpart=1, rows=X32, list_ldx=64, elems=2626, need_recenter=0, may_calibrate=0)),
    (COUNTED, dict(kind=LISTS, needs_counters=1)),
    (COUNTED + " sparse=0", dict(kind=MFMA, needs_counters=0, counter=5)),
    (COUNTED + " has_masks=0", dict(kind=MFMA, needs_counters=0)),
    (COUNTED + " xc_of_x=0", dict(kind=MFMA, pre=0, needs_counters=0)),
    (COUNTED + " e_state=2", dict(kind=MFMA, needs_counters=0)),
    (COUNTED + " act_rows=0", dict(kind=MFMA, needs_counters=0)),
    (COUNTED + " lag_valid=0", dict(kind=MFMA, needs_counters=1, may_calibrate=1)),
    (COUNTED + " lag_act=0.99*list_m_below*n_rows*K", dict(kind=LISTS, needs_counters=1)),
    (COUNTED + " lag_act=1.01*list_m_below*n_rows*K", dict(kind=MFMA, needs_counters=1)),
    (LIST + " lag_valid=1 lag_act=n_rows*K", dict(kind=LISTS, needs_counters=0)),      # a pruned pass: however many are active
    (COUNTED + " K=257", dict(status=OK, kind=MFMA, needs_counters=1)),
    # ---- lists: refusals
    (LIST + " sparse=0", dict(status=ESTATE, message=PRUNED)),
    (LIST + " K=257", dict(status=ESTATE, message=PRUNED)),
    (LIST + " xc_of_x=0", dict(status=ESTATE, message=PRUNED)),
    (LIST + " e_state=2", dict(status=OK, kind=MFMA)),                               # (loaded responsibilities: no pruned output)
    (COUNTED + " lock_live=1 lag_valid=0", dict(status=ESTATE, message=SETTLED, needs_counters=1)),
    ("lock_live=1", dict(status=ESTATE, message=SETTLED)),
    # ---- lists: row source
    (LIST + " ldx=80", dict(rows=X32, list_ldx=80)),
    (LIST + " ldx=80 sorted=1 has_xp=1", dict(rows=XP32, list_ldx=64)),
    (LIST + " vec=0", dict(rows=CENTRED, list_ldx=0)),
    (LIST + " T=2 D=32", dict(rows=X32)),
    (LIST + " T=8 D=128 sorted=1 has_xp=1", dict(rows=XP32, list_ldx=128)),
    (LIST + " T=3 D=48", dict(rows=CENTRED)),
    (LIST + " D=60", dict(rows=CENTRED)),
    (LIST + " f64=1", dict(rows=CENTRED)),
    (LIST + " f64=1 sorted=1 has_xp=1", dict(rows=CENTRED)),
    (LIST + " opt_mlist_xc=1", dict(rows=CENTRED)),
    (LIST + " opt_mlist_xc=1 sorted=1 has_xp=1", dict(rows=CENTRED)),
    (LIST + " xc_stale=1", dict(rows=X32, need_recenter=0)),                         # the centred copy is not read
    (LIST + " sorted=1 has_xp=1 xc_stale=1", dict(rows=XP32, need_recenter=0)),
    (LIST + " sorted=1 has_xp=1 xc_stale=1 f64=1", dict(rows=CENTRED, need_recenter=1)),
    (LIST + " sorted=1 has_xp=1 xc_stale=1 opt_mlist_xc=1", dict(rows=CENTRED, need_recenter=1)),
    # ---- lists: grids.  600000 rows: ceil(4800000 / 1024) + 8 = 4696 chunks at most, more than the 1408 slabs
    (LIST + " act_rows=600000 " + rows(600000), dict(cap_chunks=1408, lgrid=352, grid=352)),
    (LIST + " K=200", dict(cap_chunks=35200, lgrid=(1172 + 200 + 3) // 4)),          # ceil(1200000 / 1024) = 1172
    # the delta lists: at most one entry per row, ceil(6000 / 1024) + 8 = 14 chunks -> 4 workgroups; never more than lgrid
    (CACHE + " delta_pending=1", dict(apply_delta=1, dgrid=4, lgrid=14)),
    (CACHE + " delta_pending=1 S_cap=1", dict(apply_delta=1, cap_chunks=8, lgrid=2, dgrid=2)),
    (CACHE, dict(apply_delta=0, dgrid=0)),
    # ---- lists: the cache of settled rows
    (CACHE + " delta_pending=1 mlists_done=1 active_lists=1",
     dict(status=OK, apply_delta=1, build=MMASK, delta_pending=0, mlists_done=1, active_lists=0, add_cache=1, qpart=1, clear_blk_fresh=0)),
    (CACHE + " delta_pending=1 mlists_done=1 mlists_lost=1",
     dict(status=ESTATE, message=LOST, kind=LISTS, apply_delta=1, build=NONE, delta_pending=0, mlists_done=0, active_lists=0)),
    (CACHE + " mlists_lost=1", dict(status=ESTATE, message=LOST, kind=LISTS, apply_delta=0, build=NONE)),
    (CACHE + " mlists_done=1 mlists_lost=1", dict(status=OK, build=NONE)),
    (CACHE + " mlists_done=1", dict(status=OK, apply_delta=0, build=NONE, mlists_done=1, active_lists=0, add_cache=1)),
    (CACHE, dict(build=MMASK, mlists_done=1, active_lists=0, clear_blk_fresh=0, add_cache=1)),
    (CACHE + " active_lists=1", dict(build=MMASK, mlists_done=1, active_lists=0)),
    (LIST + " active_lists=1", dict(build=NONE, active_lists=1, clear_blk_fresh=0, add_cache=0)),
    (LIST + " delta_pending=1", dict(apply_delta=0, delta_pending=1, build=MASKS)),  # (no cache in force: nothing to apply)
    (LIST + " mlists_done=1", dict(build=MASKS, mlists_done=1, active_lists=1)),
]


def answers(tmp_path, cxx):
    exe = str(tmp_path / "mstep_plan_cases")
    subprocess.run(cxx + ["-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                          os.path.join(HERE, "mstep_plan_cases.cpp"), "-o", exe], check=True)
    lines = [f"{BASE} {over}" for over, _want in CASES]
    run = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True)      # directly: no LD_PRELOAD
    assert run.returncode == 0 and run.stderr == "", run.stderr
    out = []
    for ln in run.stdout.splitlines():
        head, _, message = ln.partition(" | ")
        out.append(dict({kv.split("=")[0]: int(kv.split("=")[1]) for kv in head.split()}, message=message))
    assert len(out) == len(lines), run.stdout
    return out


def test_plan_mstep(tmp_path):
    got = answers(tmp_path, host_compiler())
    wrong = [(case, key, val, have[key]) for (case, want), have in zip(CASES, got) for key, val in want.items() if have[key] != val]
    assert not wrong, wrong
