"""The seed lookup's choice of kernel and shape on the CPU: tests/host/lookup_plan_main.cpp runs k1_plan of shrimp_amd/csrc/gm_lookup_plan.h (a header without HIP) over a
table of index and read shapes -- the ones DESIGN.md section 5 argues from, the forced variants of the GPU tests, the switches of a call, both sides of the 8 000- and
30 000-entry thresholds -- whose expected kernels and shapes were recorded from the launch code as it was before the plan existed.  The program is built with
AddressSanitizer + UBSan where their runtimes are installed (it is a stand-alone program: nothing is preloaded), and without them otherwise.  Needs no GPU."""
import os, subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_lookup_plan_table(tmp_path):
    exe = str(tmp_path / "lookup_plan_main")
    base = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-I", os.path.join(ROOT, "shrimp_amd", "csrc"), "-o", exe, os.path.join(ROOT, "tests", "host", "lookup_plan_main.cpp")]
    r = subprocess.run(base + ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"], capture_output=True, text=True)
    sanitized = r.returncode == 0
    if not sanitized:                                                # (no sanitizer runtime on this machine)
        r = subprocess.run(base, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    assert "warning" not in r.stderr, r.stderr[-4000:]
    p = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    if sanitized and "LeakSanitizer has encountered a fatal error" in p.stderr:      # (where it cannot stop the world; the program allocates nothing it keeps)
        p = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    print("sanitizers: %s\n%s" % ("address,undefined" if sanitized else "none (runtime not installed)", p.stdout.strip()))
    assert p.returncode == 0, (p.stdout + p.stderr)[-4000:]
    assert "lookup plan ok" in p.stdout
