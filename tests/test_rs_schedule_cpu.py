"""The resampler's phase schedule (libtsd_amd/csrc/rs_schedule.hpp) is host arithmetic that decides a bit-exact index result: its
stand-alone C++ test (tests/cpp/test_rs_schedule_cpu.cc) holds it to the literal float32 recurrence, built with
-fsanitize=address,undefined and, for the shared-schedule section, with -fsanitize=thread.  No GPU, no library, nothing loaded into
Python."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def run(target, *args):
    subprocess.run(["make", "-C", os.path.join(ROOT, "tests", "cpp"), "build/" + target], check=True, capture_output=True)
    r = subprocess.run([os.path.join(ROOT, "tests", "cpp", "build", target), *args], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    assert "RS SCHEDULE OK" in r.stdout


def test_schedule_against_the_literal_recurrence_under_sanitizers():
    """every index 0..20000 and scattered ones to 3 periods for twelve ratios, their cycles, the cache, position 10^9, eight threads"""
    run("test_rs_schedule_cpu")


def test_shared_schedule_under_the_thread_sanitizer():
    """eight threads extend and read one shared schedule: no data race, the single-threaded results"""
    run("test_rs_schedule_tsan", "threads")
