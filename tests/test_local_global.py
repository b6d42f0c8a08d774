"""CPU: the stopping rule of the local / global alternation (csrc/smg_local_global.hpp; smg_arap_solve, smg_param_arap).

The header holds the control flow alone -- no HIP, no library symbol -- so tests/local_global_driver.cpp (its own main, one translation unit)
drives it with scripted energies and a scripted inner solve: max_iter, the relative drop (equality and an increase included), max_iter 0, a
non-finite energy, a failing solve, null outputs.  The history and cycle arrays are heap arrays of exactly max_iter + 1 and max_iter entries."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_stopping_rule_under_asan_ubsan(tmp_path):
    """compiled with -fsanitize=address,undefined and the static sanitizer runtimes, run directly: nothing is loaded into python, nothing preloaded"""
    exe = str(tmp_path / "local_global_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-static-libasan", "-static-libubsan",
                           "-fno-omit-frame-pointer", "-fno-sanitize-recover=undefined", "-ffp-contract=off",
                           "-I" + os.path.join(ROOT, "surface_multigrid_code_amd", "csrc"), os.path.join(ROOT, "tests", "local_global_driver.cpp"), "-o", exe])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1:abort_on_error=0", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([exe], env=env, capture_output=True, text=True, timeout=120)
    out = r.stdout + r.stderr
    assert "AddressSanitizer" not in out and "runtime error:" not in out, out[-4000:]
    assert r.returncode == 0 and "LOCAL_GLOBAL_DRIVER OK" in out, out[-4000:]
