#!/usr/bin/env python3
"""Generate tests/golden/genfa/<case>/ from the REFERENCE binaries built by oracle/Makefile.ref: genome FASTA files as the binary read them, the index it
wrote from them (-S: idx.genome, idx.seed.N) and the SAM of its -L run on that index (the @PG line dropped, it embeds the command line).

Runs only where the reference is built (oracle/_ref).  Fixtures are data only.  Every case is checked here: the contig count and lengths inside the
reference's idx.genome must equal this generator's own parse of the files -- a case the binary rejects or truncates is not a golden.

    make -f oracle/Makefile.ref && python tools/make_genome_golden.py
"""
import gzip, json, os, shutil, struct, subprocess, sys, tempfile
import numpy as np
sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))
from shrimp_amd import synth

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
GOLD = os.path.join(ROOT, "tests", "golden")
OUT = os.path.join(GOLD, "genfa")
SEEDS = "11110111,1101011011"
LETTERS = b"ACGTUMRWSYKVHDBN"
T = np.frombuffer(LETTERS, dtype=np.uint8)


def parse_fasta(texts):
    """the reference's reader for a genome, restated: names and letters (bytes) per contig over the files in order"""
    names, seqs = [], []
    for text in texts:
        for line in text.split(b"\n"):
            if line[:1] == b"#":
                continue
            if line[:1] == b">":
                names.append(line[1:].split(b"\t")[0].strip().split(b" ")[0]); seqs.append(bytearray())
            else:
                seqs[-1] += line
    return names, [bytes(s) for s in seqs]


def letters_to_codes(seq):
    lut = np.full(256, 255, dtype=np.uint8)
    for i, c in enumerate(LETTERS):
        lut[c] = i; lut[c | 0x20] = i
    for c in b"Xx.":
        lut[c] = 15
    codes = lut[np.frombuffer(seq, dtype=np.uint8)]
    assert (codes != 255).all()
    return codes


def read_ref_genome_table(path):
    """contig lengths and names of a reference idx.genome"""
    with gzip.open(path, "rb") as f:
        b = f.read()
    mode, hflag, nc = struct.unpack_from("<3I", b, 0)
    lens = struct.unpack_from("<%dI" % nc, b, 12)
    p = 12 + 8 * nc; names = []
    for _ in range(nc):
        (nl,) = struct.unpack_from("<I", b, p); names.append(b[p + 4:p + 4 + nl]); p += 4 + nl + 1
    return list(lens), names


def gz(text):
    """the genome files are stored (and given to the binary) gzip-compressed, which it reads like plain text; the tests also run plain copies"""
    return gzip.compress(text, 9, mtime=0)


def ragged_lines(rng, text, lo=1, hi=200):
    out, k = [], 0
    while k < len(text):
        w = int(rng.integers(lo, hi + 1)); out.append(text[k:k + w]); k += w
    return out


def lower_runs(rng, text, n):
    b = bytearray(text)
    for _ in range(n):
        a = int(rng.integers(0, len(b))); e = min(len(b), a + int(rng.integers(1, 400)))
        b[a:e] = bytes(b[a:e]).lower()
    return bytes(b)


def case_ragged():
    rng = np.random.default_rng(101)
    cs = [rng.integers(0, 4, n, dtype=np.uint8) for n in (9001, 7013, 5002)]
    cs[0][1200:1260] = 15
    f = [b"# a comment before the first header", b"#", b">chrR1 ragged lines"]
    for i, c in enumerate(cs):
        if i:
            f += [b"# between contigs", b">chrR%d" % (i + 1)]
        lines = ragged_lines(rng, lower_runs(rng, T[c].tobytes(), 6))
        for k, l in enumerate(lines):
            f.append(l)
            if k % 17 == 5: f.append(b"#comment inside a sequence > with a mark")
            if k % 23 == 7: f.append(b"")                       # an empty line inside a sequence: the reference appends nothing (checked below like every case)
    return {"g.fa.gz": gz(b"\n".join(f))}                            # no '\n' after the last line


def case_iupac():
    rng = np.random.default_rng(102)
    f = []
    for k in range(8):
        n = 2400 + 8 * int(rng.integers(0, 30)) + k             # lengths = 0..7 mod 8
        c = rng.integers(0, 4, n, dtype=np.uint8)
        iu = rng.integers(0, n, 60); c[iu] = rng.integers(4, 16, 60).astype(np.uint8)
        for a in (5, 13, 803, 1606):                            # N runs across word edges
            c[a:a + 3 + k] = 15
        c[n - 2 - k % 3:] = 15                                  # ... and across the contig's end
        if k % 2: c[:1 + k] = 15
        t = bytearray(T[c].tobytes())
        for a in rng.integers(0, n, 12):
            if t[a] == ord("N"): t[a] = b"Xx.n"[int(rng.integers(0, 4))]
        t[20:24] = b"Xx.."
        f += [b">iu%d len %d" % (k, n)] + ragged_lines(rng, lower_runs(rng, bytes(t), 2), 40, 90)
    return {"g.fa.gz": gz(b"\n".join(f) + b"\n")}


def case_names():
    rng = np.random.default_rng(103)
    heads = [b">  gi|12345|ref|NC_000001.1|   Homo sapiens chromosome 1, a long description " + b"x" * 300, b">dup second", b">dup", b">name\twith a tab and more"]
    f = []
    for h, n in zip(heads, (6000, 4001, 3003, 2500)):
        f += [h] + ragged_lines(rng, T[rng.integers(0, 4, n, dtype=np.uint8)].tobytes(), 60, 60)
    return {"g.fa.gz": gz(b"\n".join(f) + b"\n")}


def case_twofiles():
    rng = np.random.default_rng(104)
    def one(names, lens):
        f = []
        for nm, n in zip(names, lens):
            f += [b">" + nm] + ragged_lines(rng, T[rng.integers(0, 4, n, dtype=np.uint8)].tobytes(), 70, 70)
        return b"\n".join(f) + b"\n"
    return {"z_first.fa.gz": gz(one([b"zA", b"zB"], [7001, 3005])), "a_second.fa": one([b"aC"], [6004])}


def case_chunk_edges():
    rng = np.random.default_rng(105)
    f = [b"# one line per contig"]
    for k, n in enumerate((131071, 99999, 70003)):
        c = rng.integers(0, 4, n, dtype=np.uint8)
        for a in range(0, n, 10000):                            # N blocks keep the seed files small; their edges still move every list
            c[a + 1500:a + 10000] = 15
        f += [b">edge%d" % k, T[c].tobytes()]
        if k == 0: f += [b"#" + b"c" * 5000]
    return {"g.fa.gz": gz(b"\n".join(f) + b"\n")}


def run_case(name, files, binary="gmapper-ls", reads_from=None, order=None):
    """files: {file name: bytes} written into the case directory, or paths relative to it (existing fixtures)"""
    d = os.path.join(OUT, name); shutil.rmtree(d, ignore_errors=True); os.makedirs(d)
    order = order or list(files)
    for fn in order:
        if files[fn] is not None:
            with open(os.path.join(d, fn), "wb") as f: f.write(files[fn])
    paths = [os.path.join(d, fn) for fn in order]
    texts = [(gzip.open(p, "rb") if open(p, "rb").read(2) == b"\x1f\x8b" else open(p, "rb")).read() for p in paths]
    names, seqs = parse_fasta(texts)
    contigs = [letters_to_codes(s) for s in seqs]
    ref = os.path.join(ROOT, "oracle", "_ref", binary)
    if reads_from is None:
        reads, _ = synth.make_reads(contigs, 300, 50, 91)
        with gzip.GzipFile(os.path.join(d, "reads.fa.gz"), "wb", 9, mtime=0) as f:
            for i, r in enumerate(reads): f.write(b">r%d\n" % i + T[r].tobytes() + b"\n")
        reads_rel = "reads.fa.gz"
    else:
        reads_rel = reads_from
    subprocess.run([ref, "-s", SEEDS, "-S", os.path.join(d, "idx"), *paths], capture_output=True, check=True)
    lens, rnames = read_ref_genome_table(os.path.join(d, "idx.genome"))
    assert lens == [len(c) for c in contigs] and rnames == names, (name, lens, [len(c) for c in contigs], rnames, names)
    p = subprocess.run([ref, "-N", "2", "-L", os.path.join(d, "idx"), os.path.join(d, reads_rel)], capture_output=True, check=True)
    body = b"".join(l + b"\n" for l in p.stdout.split(b"\n") if l and not l.startswith(b"@PG"))
    with gzip.GzipFile(os.path.join(d, "from_index.sam.gz"), "wb", 9, mtime=0) as f: f.write(body)
    with open(os.path.join(d, "case.json"), "w") as f:
        json.dump({"genome_files": order, "reads": reads_rel, "seeds": SEEDS.split(","), "binary": binary, "build_options": ["-s", SEEDS], "map_options": ["-N", "2"]}, f, indent=1)
        f.write("\n")
    print("%-14s %d contigs %s, %d SAM records, %s" % (name, len(lens), lens, sum(1 for l in body.split(b"\n") if l and not l.startswith(b"@")),
                                                        {fn: os.path.getsize(os.path.join(d, fn)) for fn in sorted(os.listdir(d))}))


def main():
    ragged = case_ragged()
    run_case("ragged", ragged)
    run_case("iupac", case_iupac())
    run_case("names", case_names())
    run_case("twofiles_gz", case_twofiles(), order=["z_first.fa.gz", "a_second.fa"])
    run_case("rna_last_rna", {"../../rna_genome_last_rna.fa.gz": None}, reads_from="../../rna_reads_ls.fa.gz")
    run_case("rna_last_dna", {"../../rna_genome_last_dna.fa.gz": None}, reads_from="../../rna_reads_ls.fa.gz")
    # colour space: the genome whose LAST contig is DNA.  The binary sets genome_is_rna only while it reads FASTA (genome.c:1064), so its -L run on an index whose
    # last contig is RNA maps colour-space reads differently from its own run on the FASTA; the library derives the flag from the resident genome either way.
    run_case("cs", {"../../rna_genome_last_dna.fa.gz": None}, binary="gmapper-cs", reads_from="../../rna_reads_cs.fa.gz")
    run_case("chunk_edges", case_chunk_edges())


if __name__ == "__main__":
    main()
