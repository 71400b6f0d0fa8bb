"""The ordered text buffer of the unpaired mapping calls and its parked-buffer cache on the CPU: tests/host/textout_main.cpp instantiates GmTextOut / GmTextCache of
shrimp_amd/csrc/gm_textout.h with a counting allocator and walks the order of the appends, every allocation failure, failed jobs, the hand-over and the parked buffer.
The program is built twice, with AddressSanitizer + UBSan and with ThreadSanitizer, where their runtimes are installed (it is a stand-alone program: nothing is
preloaded), and without them otherwise -- the program's own counters decide either way.  Needs no GPU."""
import os, subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _build_and_run(tmp_path, sanitizer):
    exe = str(tmp_path / "textout_main")
    base = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-pthread", "-I", os.path.join(ROOT, "shrimp_amd", "csrc"), "-o", exe, os.path.join(ROOT, "tests", "host", "textout_main.cpp")]
    r = subprocess.run(base + ["-fsanitize=" + sanitizer, "-fno-sanitize-recover=undefined"], capture_output=True, text=True)
    sanitized = r.returncode == 0
    if not sanitized:                                                # (no sanitizer runtime on this machine)
        r = subprocess.run(base, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    assert "warning" not in r.stderr, r.stderr[-4000:]
    p = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    if sanitized and "LeakSanitizer has encountered a fatal error" in p.stderr:      # (it cannot stop the world in this sandbox: the allocator's counters still see every leak)
        p = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    print("sanitizers: %s\n%s" % (sanitizer if sanitized else "none (runtime not installed)", p.stdout.strip()))
    assert p.returncode == 0, (p.stdout + p.stderr)[-4000:]
    assert "textout ok" in p.stdout


def test_textout_rules(tmp_path):
    for sanitizer in ("address,undefined", "thread"):
        _build_and_run(tmp_path, sanitizer)
