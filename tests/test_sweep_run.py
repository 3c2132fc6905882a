"""The run length of the carried sweep (csrc/workspace_plan.h): which of the compiled lengths 1, 2, 4 a shape and the
developer switch GMMVB_SWEEP_RUN get, and that the launch's dispatch hands out that constant.  tests/sweep_run_cases.cpp
includes only the plain header; it is built here by the host compiler with AddressSanitizer and UBSan and run once.

tests/test_gpu_sweep_runs.py compares the run lengths' results on the GPU, where nothing observable tells them apart; that
the switch reaches the launch is what this file holds: the option is read (behind GMMVB_DEBUG only), rounded to the compiled
length nearest below, ignored above K = 128, and dispatched as asked."""
import os
import subprocess

import pytest

from test_pass_plan import HERE, host_compiler

DEFAULT = 2
# (K, asked) -> run length
LENGTHS = [((64, 0), DEFAULT), ((64, 1), 1), ((64, 2), 2), ((64, 3), 2), ((64, 4), 4), ((64, 5), 4), ((64, 1000), 4),
           ((1, 0), DEFAULT), ((65, 4), 4), ((128, 0), DEFAULT), ((128, 4), 4), ((128, 1), 1),
           ((129, 0), 1), ((129, 2), 1), ((129, 4), 1), ((130, 4), 1), ((256, 2), 1), ((256, 0), 1)]
OPTIONS = [({}, 0), ({"GMMVB_SWEEP_RUN": "4"}, 0), ({"GMMVB_DEBUG": "0", "GMMVB_SWEEP_RUN": "4"}, 0),
           ({"GMMVB_DEBUG": "1"}, 0), ({"GMMVB_DEBUG": "1", "GMMVB_SWEEP_RUN": "1"}, 1),
           ({"GMMVB_DEBUG": "1", "GMMVB_SWEEP_RUN": "2"}, 2), ({"GMMVB_DEBUG": "2", "GMMVB_SWEEP_RUN": "4"}, 4),
           ({"GMMVB_DEBUG": "1", "GMMVB_SWEEP_RUN": "-3"}, 0), ({"GMMVB_DEBUG": "1", "GMMVB_SWEEP_RUN": "x"}, 0)]


@pytest.fixture(scope="module")
def answers(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("sweep_run") / "sweep_run_cases")
    subprocess.run(host_compiler() + ["-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                                      os.path.join(HERE, "sweep_run_cases.cpp"), "-o", exe], check=True)
    lines = [f"length {K} {asked}" for (K, asked), _want in LENGTHS]
    lines += ["option " + " ".join(f"env.{k}={v}" for k, v in env.items()) for env, _want in OPTIONS]
    run = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True)      # directly: no LD_PRELOAD
    assert run.returncode == 0 and run.stderr == "", run.stderr
    out = run.stdout.splitlines()
    assert len(out) == len(lines), run.stdout
    return out


@pytest.mark.parametrize("i", range(len(LENGTHS)), ids=[f"K{K}-asked{a}" for (K, a), _ in LENGTHS])
def test_run_length_and_dispatch(answers, i):
    want = LENGTHS[i][1]
    assert answers[i].split() == [str(want), str(want)]


@pytest.mark.parametrize("i", range(len(OPTIONS)), ids=[str(i) for i in range(len(OPTIONS))])
def test_switch_is_read_behind_debug_only(answers, i):
    assert int(answers[len(LENGTHS) + i]) == OPTIONS[i][1]
