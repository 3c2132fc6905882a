"""The E-step's choice of pass (bayesml_amd/csrc/pass_plan.h: choose_pass, BoundLevel::choose) without a GPU.

tests/pass_plan_cases.cpp includes only that header; it is built here by the host compiler with AddressSanitizer and UBSan,
run once over every case below, and its answers are compared with what the code of gmmvb_estep gave for the same facts
before the decision was moved out of it (read line by line).  Thresholds are named, not written out: the program takes
them from PolicyTable after init(8, 4) (D = 128), where prune_below() is 0.478 and dense_again_above() 0.636."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
DENSE, BOUND, SWEEP = 0, 1, 3

# P = rows * K pairs.  The base case is a carried pass in full swing: the plan is a sweep.
BASE = ("K=64 T=8 D=128 n_rows=rows L.rows=rows L.valid=1 prune=1 can_prune=1 big=1 known=1 same_rows=1 have_drift=1 "
        "dense_valid=1 typical_gamma=-1 L.mode=sweep L.act=0.05*P L.eval=0.06*P bound_tb=0 bound_fail_act=-1")
NO_DRIFT = "have_drift=0"                      # the simplest way to a bound plan
REGROUP = "sort_rows=1 has_xp=1 sorted=0 sorts=0 after_estep=1 has_xc=1 xc_of_x=1"
CACHE = "has_lock=1 cache_on=1 sparse=1 has_masks=1 has_xc=1 xc_of_x=1"
PROOF = CACHE + " opt_proof=1 xq_of_x=1 has_bound_images=1 xq_current=1"
FALLBACK = "have_drift=0 L.mode=bound L.act=0.4*P L.eval=0.7*P"

PLANS = [
    # (overrides of the base case, expected fields of the plan)
    ("", dict(mode=SWEEP, fell_back=0, bound_fail_act=-1, regroup=0, reset_cache=0, settle=0, proof_capable=0, skip_margin=-1)),
    # pruning unavailable
    ("can_prune=0", dict(mode=DENSE)),
    ("big=0", dict(mode=DENSE)),
    # prune threshold
    ("L.act=1.01*prune_below*P", dict(mode=DENSE, fell_back=0)),
    ("L.act=0.99*prune_below*P", dict(mode=SWEEP)),
    # forget
    ("forget=1 bound_fail_act=0.4", dict(mode=DENSE, bound_fail_act=-1)),
    ("forget=1 prune=2 have_drift=0", dict(mode=BOUND)),
    # counters not arrived
    ("known=0", dict(mode=DENSE)),
    ("known=0 prune=2", dict(mode=SWEEP)),
    ("known=0 prune=2 have_drift=0", dict(mode=BOUND)),
    # bound-fail hold-off
    ("bound_fail_act=0.4 L.act=0.31*P", dict(mode=DENSE, fell_back=0, bound_fail_act=0.4)),
    ("bound_fail_act=0.4 L.act=0.29*P", dict(mode=SWEEP)),
    ("bound_fail_act=0.4 L.act=0.31*P prune=2", dict(mode=SWEEP)),
    # no usable carry
    ("have_drift=0", dict(mode=BOUND)),
    ("opt_carry_off=1", dict(mode=BOUND)),
    ("same_rows=0", dict(mode=BOUND)),
    # drift summary
    ("typical_gamma=0.49", dict(mode=BOUND)),
    ("typical_gamma=0.5", dict(mode=SWEEP)),
    ("typical_gamma=0", dict(mode=SWEEP)),
    ("typical_gamma=-1", dict(mode=SWEEP)),
    # bound array not valid
    ("dense_valid=0", dict(mode=BOUND)),
    ("dense_valid=0 can_project=1 opt_project=2", dict(mode=SWEEP)),
    ("dense_valid=0 can_project=1 opt_project=1", dict(mode=BOUND)),
    # spare veto at bound level 3: bound_cost = 0.12 * 6 + 0.039 * 96 against 0.81 * 36 * spare * 2.5
    ("L.eval=L.act+0.07*P", dict(mode=BOUND, spare_set=1)),
    ("L.eval=L.act+0.05*P", dict(mode=SWEEP, spare_set=1)),
    ("L.eval=L.act+0.07*P bound_tb=4", dict(mode=SWEEP)),
    ("L.proof=0.2*P L.mode=sweep", dict(mode=BOUND)),
    ("L.proof=0.2*P L.mode=bound", dict(mode=SWEEP)),
    # overflow rows
    ("L.over=0.021*rows", dict(mode=BOUND)),
    ("L.over=0.019*rows", dict(mode=SWEEP)),
    # the carried pass lost its bounds (carried_eval_above)
    ("L.act=0.36*P L.eval=0.36*P", dict(mode=BOUND)),
    # after a dense pass
    ("L.mode=dense L.act=0.11*P", dict(mode=BOUND)),
    ("L.mode=dense L.act=0.09*P typical_gamma=0.84", dict(mode=BOUND)),
    ("L.mode=dense L.act=0.09*P typical_gamma=0.86", dict(mode=SWEEP)),
    ("L.mode=dense L.act=0.09*P typical_gamma=-1", dict(mode=SWEEP)),
    ("L.mode=dense L.eval=0.9*P", dict(mode=SWEEP, spare_set=0)),
    # dense fallback
    (FALLBACK, dict(mode=DENSE, fell_back=1, bound_fail_act=0.4)),
    (FALLBACK + " prune=2", dict(mode=BOUND, fell_back=0)),
    (FALLBACK + " have_drift=1", dict(mode=DENSE, fell_back=1, spare_set=1)),
    # forced regrouping
    (REGROUP + " L.act=2.4*rows", dict(mode=BOUND, regroup=1)),
    (REGROUP + " L.act=2.6*rows", dict(mode=SWEEP, regroup=0)),
    (REGROUP + " L.act=2.4*rows sorts=1", dict(mode=SWEEP, regroup=0)),
    (REGROUP + " have_drift=0 L.act=3.9*rows", dict(mode=BOUND, regroup=1)),
    (REGROUP + " have_drift=0 L.act=4.1*rows", dict(mode=BOUND, regroup=0)),
    (REGROUP + " have_drift=0 L.act=2.4*rows sorted=1 moved_since_sort=0.04*rows", dict(mode=BOUND, regroup=0)),
    (REGROUP + " have_drift=0 L.act=2.4*rows sorted=1 moved_since_sort=0.06*rows", dict(mode=BOUND, regroup=1)),
    (REGROUP + " have_drift=0 L.act=2.4*rows hmm=1", dict(mode=BOUND, regroup=0)),
    (REGROUP + " L.act=2.4*rows hmm=1", dict(mode=BOUND, regroup=0)),
    # cache of settled rows
    (CACHE + " lock_reset=1", dict(mode=BOUND, reset_cache=1, settle=1)),
    (CACHE + " lock_live=1 big=0", dict(mode=DENSE, reset_cache=1, settle=0)),
    (CACHE + " lock_live=1 same_rows=0", dict(mode=BOUND, reset_cache=1)),
    (CACHE + " lock_live=1 delta_pending=1", dict(mode=BOUND, reset_cache=1)),
    (CACHE + " lock_live=1", dict(mode=SWEEP, reset_cache=0, settle=1)),
    (CACHE + " big=0", dict(mode=DENSE, settle=0)),
    (CACHE + " cache_on=0", dict(mode=SWEEP, settle=0)),
    (CACHE + " has_lock=0 lock_reset=1", dict(mode=SWEEP, reset_cache=0, settle=0)),
    (PROOF + " settle_margin=2.5", dict(settle=1, proof_capable=1, skip_margin=2.5)),
    (PROOF + " settle_margin=-1", dict(settle=1, proof_capable=1, skip_margin=-1)),
    (PROOF + " settle_margin=2.5 opt_proof=0", dict(settle=1, proof_capable=0, skip_margin=-1)),
    (PROOF + " settle_margin=2.5 xq_current=0", dict(proof_capable=0, skip_margin=-1)),
    (PROOF + " settle_margin=2.5 cache_on=0", dict(settle=0, proof_capable=0, skip_margin=-1)),
]

# BoundLevel::choose.  The observed-level update: a bound pass at level 3 of 4 (D = 128) has reported.
SEEN = "K=64 T=8 D=128 has_bound_images=1 mode=bound known=1 L.valid=1 L.rows=rows L.mode=bound tb=3 L.act=0.05*P"
LEVELS = [
    # a first bound pass picks min(3, t32); one that will be carried takes every block
    ("K=64 T=4 D=64 has_bound_images=1 mode=bound", dict(tb=2)),
    ("K=64 T=8 D=128 has_bound_images=1 mode=bound", dict(tb=3)),
    ("K=64 T=8 D=128 has_bound_images=1 mode=bound carried_after=1 wants_drift=1", dict(tb=4)),
    ("K=64 T=8 D=128 has_bound_images=0 mode=bound", dict(tb=0)),
    ("K=64 T=8 D=128 has_bound_images=1 mode=sweep tb=3 cand3=0.1", dict(tb=3, cand3=0.1)),
    # the report is booked under the level in force; a level not seen for 32 passes is forgotten, a fresher one is kept
    (SEEN + " L.eval=0.1*P cand1=0.3 act1=0.05 seen1=5 cand2=0.2 act2=0.05 seen2=32",
     dict(tb=3, cand3=0.1, act3=0.05, seen3=0, cand1=0.3, seen1=6, cand2=-1, seen2=33)),
    # ... and so is one observed at an active share 1.5 x off the present one, either way
    (SEEN + " L.eval=0.1*P cand2=0.2 act2=0.08 cand4=0.06 act4=0.03 cand1=0.3 act1=0.07",
     dict(tb=3, cand2=-1, cand4=-1, cand1=0.3)),
    # the cheapest known level: 0.12 * 3 + 0.039 * 64 + 29.16 * 0.12 = 6.36 at level 2 against 4.464 + 29.16 * 0.1 = 7.38 at 3
    (SEEN + " L.eval=0.1*P cand2=0.12 act2=0.05", dict(tb=2, cand2=0.12)),
    (SEEN + " L.eval=0.1*P cand2=0.16 act2=0.05", dict(tb=3)),
    # few spares (0.001 * 64 < 0.25): one level down if it is unknown - but 0.02 is the line when carried passes will inherit them
    (SEEN + " L.eval=0.051*P", dict(tb=2)),
    (SEEN + " L.eval=0.051*P wants_drift=1", dict(tb=3)),
    (SEEN + " L.eval=0.051*P cand2=0.3 act2=0.05", dict(tb=3)),
    # many spares (0.07 * 29.16 > 0.12 * 4 + 0.039 * 32): one level up if it is unknown
    (SEEN + " L.eval=0.12*P", dict(tb=4)),
    (SEEN + " L.eval=0.10*P", dict(tb=3)),
    # the counters are not a bound pass's, or have not arrived: the level stays
    (SEEN + " L.eval=0.12*P L.mode=sweep", dict(tb=3, cand3=-1)),
    (SEEN + " L.eval=0.12*P known=0", dict(tb=3, cand3=-1)),
    # a dense plan clears what was learnt
    ("K=64 T=8 D=128 has_bound_images=1 mode=dense tb=3 cand1=0.3 cand2=0.2 cand3=0.1 cand4=0.05 act3=0.05 seen3=4",
     dict(tb=3, cand1=-1, cand2=-1, cand3=-1, cand4=-1, act3=0.05, seen3=4)),
]


def host_compiler():
    for cxx in (os.environ.get("CXX"), "c++", "/opt/rocm/llvm/bin/clang++", "/opt/rocm/bin/amdclang++"):
        if cxx and shutil.which(cxx.split()[0]):
            return cxx.split()
    pytest.fail("no host C++ compiler: set CXX")


def answers(tmp_path):
    exe = str(tmp_path / "pass_plan_cases")
    subprocess.run(host_compiler() + ["-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                                      os.path.join(HERE, "pass_plan_cases.cpp"), "-o", exe], check=True)
    lines = [f"plan {BASE} {over}" for over, _want in PLANS] + [f"level {args}" for args, _want in LEVELS]
    run = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True)
    assert run.returncode == 0, run.stderr
    out = [dict((kv.split("=")[0], float(kv.split("=")[1])) for kv in ln.split()) for ln in run.stdout.splitlines()]
    assert len(out) == len(lines), run.stdout
    return out


def test_choose_pass_and_bound_level(tmp_path):
    got = answers(tmp_path)
    wrong = []
    for (case, want), have in zip(PLANS + LEVELS, got):
        for key, val in want.items():
            if abs(have[key] - val) > 1e-9:
                wrong.append((case, key, val, have[key]))
    assert not wrong, wrong
