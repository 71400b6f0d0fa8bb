"""GmDevMem's ownership rules on the CPU: tests/host/devmem_main.cpp instantiates the holder of shrimp_amd/csrc/gm_devmem.h with a counting allocator, fails
every allocator call of a seam-shaped sequence in turn and checks that nothing leaks, nothing is freed twice and the result buffer is freed unless handed over.
The program is built with AddressSanitizer and UBSan where their runtimes are installed (it is a stand-alone program: nothing is preloaded), and without them
otherwise -- the program's own counters decide either way.  Needs no GPU."""
import os, subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_devmem_ownership_rules(tmp_path):
    exe = str(tmp_path / "devmem_main")
    base = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-I", os.path.join(ROOT, "shrimp_amd", "csrc"), "-o", exe, os.path.join(ROOT, "tests", "host", "devmem_main.cpp")]
    r = subprocess.run(base + ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"], capture_output=True, text=True)
    sanitized = r.returncode == 0
    if not sanitized:                                                # (no sanitizer runtime on this machine)
        r = subprocess.run(base, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    p = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    if sanitized and "LeakSanitizer has encountered a fatal error" in p.stderr:      # (it cannot stop the world in this sandbox: the allocator's counters still see every leak)
        p = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    print("sanitizers: %s\n%s" % ("address,undefined" if sanitized else "none (runtime not installed)", p.stdout.strip()))
    assert p.returncode == 0, (p.stdout + p.stderr)[-4000:]
    assert "devmem ok" in p.stdout
