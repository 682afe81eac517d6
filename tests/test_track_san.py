"""The tracker core under AddressSanitizer + UndefinedBehaviorSanitizer:
tests/cpp/track_replay.cpp includes csrc/track_core.hpp (STL only, host only)
and replays scripted sequences; it is built with -fsanitize=address,undefined
into a temporary directory and run as a program of its own.  Nothing is loaded
into Python under a sanitizer."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_track_core_clean_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "track_replay")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-Wall", os.path.join(ROOT, "tests", "cpp", "track_replay.cpp"),
                    "-o", exe], check=True, capture_output=True, timeout=300)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=env)
    out = r.stdout + r.stderr
    assert "runtime error" not in out and "AddressSanitizer" not in out and "LeakSanitizer" not in out, out[-4000:]
    assert r.returncode == 0 and "track replay: ok" in out, out[-4000:]
