"""bench.py --dump-outputs: the SAM text of a step as float64 arrays (sam_arrays), checked on a committed golden without a GPU."""
import gzip, os, subprocess, sys, zlib
import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)
import bench


def body(name):
    with gzip.open(os.path.join(ROOT, "tests", "golden", name + ".sam.gz"), "rb") as f:
        return b"".join(l + b"\n" for l in f.read().split(b"\n") if l and not l.startswith(b"@"))


def test_sam_arrays_every_record_when_the_step_is_small():
    text = body("cfg5s_2x150_1Mbp")
    lines = text.split(b"\n")[:-1]
    a = bench.sam_arrays(text, 1500)
    assert all(v.dtype == np.float64 for v in a.values())
    r = a["sam_records"]
    assert r.shape == (len(lines), len(bench.SAM_COLUMNS))
    f = lines[0].split(b"\t")
    assert list(r[0]) == [0, int(f[1]), 2, int(f[3]), int(f[4]), 2, int(f[7]), int(f[8]), 1450, 2] and f[2] == b"contig2" and f[6] == b"="
    assert list(a["sam_record_crc32"]) == [zlib.crc32(l) for l in lines]
    assert list(a["sam_totals"]) == [len(lines), len(text), zlib.crc32(text)]


def test_sam_arrays_sample_is_fixed_and_whole_units(monkeypatch):
    text = body("cfg2s_100bp_2Mbp")
    monkeypatch.setattr(bench, "DUMP_UNITS", 300)
    a, b = bench.sam_arrays(text, 5000), bench.sam_arrays(text, 5000)
    assert all((a[k] == b[k]).all() for k in a)
    units = a["sam_records"][:, 0].astype(int)
    assert len(set(units)) == 300 and (np.diff(units) >= 0).all()
    full = bench.sam_arrays(text, 5000 * 2)["sam_totals"]                    # the totals always cover the whole text
    assert (a["sam_totals"] == full).all()


def test_bench_options():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--help"], capture_output=True, text=True, check=True).stdout
    assert "--full" in out and "--dump-outputs" in out and "--steps" in out
