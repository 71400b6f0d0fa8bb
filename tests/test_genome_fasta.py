"""gm_index_build_fasta: the index straight from genome FASTA files, packed on the device -- against what the reference binary made of the same files
(tests/golden/genfa/<case>/, written by tools/make_genome_golden.py) and against gm_index_build on the contigs parsed here in Python."""
import ctypes as C
import gzip, json, os, struct, subprocess, sys
import numpy as np
import pytest

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
GENFA = os.path.join(ROOT, "tests", "golden", "genfa")
CASES = ["ragged", "iupac", "names", "twofiles_gz", "rna_last_rna", "rna_last_dna", "cs", "chunk_edges"]
LETTERS = b"ACGTUMRWSYKVHDBN"


def load_case(name):
    d = os.path.join(GENFA, name)
    with open(os.path.join(d, "case.json")) as f:
        c = json.load(f)
    c["dir"] = d
    c["paths"] = [os.path.normpath(os.path.join(d, g)) for g in c["genome_files"]]
    c["reads_path"] = os.path.normpath(os.path.join(d, c["reads"]))
    c["colour"] = c["binary"] == "gmapper-cs"
    return c


def read_text(path):
    with open(path, "rb") as f:
        raw = f.read()
    return gzip.decompress(raw) if raw[:2] == b"\x1f\x8b" else raw


def parse_fasta(texts):
    """the reference's reader for a genome, restated (common/fasta.c:316-553): contig names and 4-bit code arrays over the files in order"""
    lut = np.full(256, 255, dtype=np.uint8)
    for i, ch in enumerate(LETTERS):
        lut[ch] = i; lut[ch | 0x20] = i
    for ch in b"Xx.":
        lut[ch] = 15
    names, seqs = [], []
    for text in texts:
        for line in text.split(b"\n"):
            if line[:1] == b"#": continue
            if line[:1] == b">": names.append(line[1:].split(b"\t")[0].strip().split(b" ")[0]); seqs.append(bytearray())
            else: seqs[-1] += line
    contigs = [lut[np.frombuffer(bytes(s), dtype=np.uint8)] for s in seqs]
    assert all((c != 255).all() for c in contigs)
    return names, contigs


def ref_genome_file(path):
    """mode, contig lengths, names and forward bitfields of a reference idx.genome (layout: gm_index_io.inc)"""
    with gzip.open(path, "rb") as f:
        b = f.read()
    mode, hflag, nc = struct.unpack_from("<3I", b, 0)
    lens = list(struct.unpack_from("<%dI" % nc, b, 12)); offs = list(struct.unpack_from("<%dI" % nc, b, 12 + 4 * nc))
    p = 12 + 8 * nc; names = []
    for _ in range(nc):
        (nl,) = struct.unpack_from("<I", b, p); names.append(b[p + 4:p + 4 + nl]); p += 4 + nl + 1
    (total,) = struct.unpack_from("<I", b, p); p += 4
    fwd = []
    for n in lens:
        w = (n + 7) // 8; fwd.append(np.frombuffer(b, dtype="<u4", count=w, offset=p)); p += 4 * w
    assert total == sum((n + 7) // 8 for n in lens)
    return mode, lens, offs, names, fwd


# ---- without a GPU ------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", CASES)
def test_fixture_fasta_parsed_here_equals_the_reference_index(name):
    """guards the goldens themselves: each case's FASTA, parsed by the dozen lines above, equals the contig table and the forward bitfields inside the
    reference's idx.genome"""
    from shrimp_amd import synth
    c = load_case(name)
    names, contigs = parse_fasta([read_text(p) for p in c["paths"]])
    mode, lens, offs, rnames, fwd = ref_genome_file(os.path.join(c["dir"], "idx.genome"))
    assert mode == (2 if c["colour"] else 1)
    assert rnames == names and lens == [len(x) for x in contigs]
    assert offs == [int(x) for x in np.cumsum([0] + lens[:-1])]
    for k, x in enumerate(contigs):
        assert np.array_equal(synth.pack_nibbles(x), fwd[k]), (name, k)


def test_fixture_cases_cover_what_they_are_for():
    """the properties each case was generated for are in the committed files"""
    t = read_text(load_case("ragged")["paths"][0])
    lines = t.split(b"\n")
    assert t[:1] == b"#" and not t.endswith(b"\n") and b"" in lines and any(l[:1] == b"#" for l in lines[5:]) and any(l != l.upper() for l in lines if l[:1] not in (b"#", b">"))
    widths = {len(l) for l in lines if l[:1] not in (b"#", b">", b"")}
    assert min(widths) <= 4 and max(widths) >= 195 and len(widths) >= 60, sorted(widths)
    names, contigs = parse_fasta([read_text(load_case("iupac")["paths"][0])])
    assert sorted(len(x) % 8 for x in contigs) == list(range(8)) and set(np.concatenate(contigs).tolist()) == set(range(16))
    body = read_text(load_case("iupac")["paths"][0])
    assert all(ch in body for ch in b"Xx.")
    names, _ = parse_fasta([read_text(load_case("names")["paths"][0])])
    assert names == [b"gi|12345|ref|NC_000001.1|", b"dup", b"dup", b"name"]
    two = load_case("twofiles_gz")
    assert [open(p, "rb").read(2) == b"\x1f\x8b" for p in two["paths"]] == [True, False] and two["genome_files"] != sorted(two["genome_files"])
    edges = read_text(load_case("chunk_edges")["paths"][0])
    assert 250_000 < len(edges) < 400_000 and max(len(l) for l in edges.split(b"\n")) > 100_000


def test_new_symbols_are_exported_with_the_documented_signatures():
    from shrimp_amd import gmapper as gm
    L = gm.lib()
    out = subprocess.run(["nm", "-D", "--defined-only", gm.LIB_PATH], capture_output=True, text=True, check=True).stdout
    syms = {l.split()[-1] for l in out.splitlines() if " T " in l}
    hdr = " ".join(open(os.path.join(ROOT, "include", "gmapper_hip.h")).read().split())
    for sym, decl in (("gm_index_build_fasta", "int gm_index_build_fasta(gm_index_t **out, int device, int n_files, const char *const *paths, int n_seeds, const char *const *seeds, const gm_params_t *params);"),
                      ("gm_sam_header", "int gm_sam_header(const gm_index_t *ix, const char *rg_id, const char *rg_sample, const char *command_line, char **text, size_t *len);"),
                      ("gm_index_n_contigs", "int gm_index_n_contigs(const gm_index_t *ix);"),
                      ("gm_index_contig", "int gm_index_contig(const gm_index_t *ix, int c, const char **name, uint32_t *len);")):
        assert sym in syms and sym in gm.EXPORTS and hasattr(L, sym), sym
        assert decl in hdr, sym
    for m in ("from_fasta", "sam_header", "contigs"):
        assert hasattr(gm.Index, m)


def test_build_fasta_without_a_device_is_nodevice():
    """a device that is not there (device 0 on a machine without a GPU): GM_E_NODEVICE with the usual message, before any file is touched"""
    from shrimp_amd import gmapper as gm
    L = gm.lib()
    dev = L.gm_device_count()
    paths = (C.c_char_p * 1)(os.fsencode(load_case("ragged")["paths"][0]))
    h = C.c_void_p()
    assert L.gm_index_build_fasta(C.byref(h), dev, 1, paths, 0, None, None) == -1          # GM_E_NODEVICE
    assert b"no HIP device %d" % dev in L.gm_last_error() and not h.value
    with pytest.raises(gm.GmError, match="no HIP device"):
        gm.Index.from_fasta(load_case("ragged")["paths"], device=dev)


# ---- on the GPU ---------------------------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def gm():
    try:
        import torch
        torch.cuda.init()                       # (before the library's own HIP runtime: see tests/test_gpu_parity.py)
    except Exception:
        pass
    from shrimp_amd import gmapper
    if gmapper.lib().gm_device_count() < 1:
        pytest.fail("no HIP device: the product path has no CPU fallback")
    return gmapper


def _params(gm, c):
    return gm.default_params_cs() if c["colour"] else gm.default_params()


def _device_bytes(ix):
    import torch
    from shrimp_amd import parallel
    out = []
    for p, n in ix.device_arrays():
        out.append(torch.as_tensor(parallel._DevArray(p, n), device=torch.device("cuda", 0)).cpu().numpy().tobytes() if n else b"")
    return out


def _plain_copies(c, tmp_path):
    """the case's genome files as plain text (the fixtures keep most of them gzip-compressed): the read() path of the reader instead of gzread()"""
    out = []
    for k, p in enumerate(c["paths"]):
        q = str(tmp_path / ("plain%d_%s" % (k, os.path.basename(p).replace(".gz", ""))))
        with open(q, "wb") as f: f.write(read_text(p))
        out.append(q)
    return out


def _same_as_python_parsed(gm, c, ix):
    names, contigs = parse_fasta([read_text(p) for p in c["paths"]])
    assert ix.contigs() == [(n, len(x)) for n, x in zip(names, contigs)]
    ix2 = gm.Index(contigs, names=names, seeds=c["seeds"], params=_params(gm, c))
    a, b = _device_bytes(ix), _device_bytes(ix2)
    ix2.close()
    assert len(a) == len(b) == 2 + 3 * len(c["seeds"])
    for kind, (x, y) in enumerate(zip(a, b)):
        assert len(x) == len(y), (kind, len(x), len(y))
        if x != y:
            xa, ya = np.frombuffer(x, dtype=np.uint32), np.frombuffer(y, dtype=np.uint32)
            w = int(np.flatnonzero(xa != ya)[0])
            raise AssertionError("device array kind %d differs first at word %d: %08x, gm_index_build has %08x (%d words differ)" % (kind, w, xa[w], ya[w], int((xa != ya).sum())))


@pytest.mark.gpu
@pytest.mark.parametrize("name", CASES)
def test_fasta_index_equals_reference_files_and_packed_build(gm, name, tmp_path):
    """Index.from_fasta(files) -> save(): idx.genome and every idx.seed.N, decompressed, are the reference's byte for byte; every resident array equals that
    of gm_index_build on the contigs parsed in Python; contigs() gives the names and lengths"""
    c = load_case(name)
    for tag, paths in (("stored", c["paths"]), ("plain", _plain_copies(c, tmp_path))):      # the files as the binary got them (most of them gzip), and as plain text
        ix = gm.Index.from_fasta(paths, seeds=c["seeds"], params=_params(gm, c))
        try:
            _same_as_python_parsed(gm, c, ix)
            ix.save(str(tmp_path / tag))
        finally:
            ix.close()
        for suffix in [".genome"] + [".seed.%d" % k for k in range(len(c["seeds"]))]:
            with gzip.open(os.path.join(c["dir"], "idx" + suffix), "rb") as f: want = f.read()
            with gzip.open(str(tmp_path / (tag + suffix)), "rb") as f: got = f.read()
            assert got == want, (tag, suffix, len(got), len(want))


def _first_diff(a, b):
    la, lb = a.split(b"\n"), b.split(b"\n")
    for i, (x, y) in enumerate(zip(la, lb)):
        if x != y: return i, x[:300], y[:300]
    return min(len(la), len(lb)), b"<eof>", b"<eof>"


@pytest.mark.gpu
@pytest.mark.parametrize("name", CASES)
def test_mapping_on_the_fasta_built_index_is_the_reference_sam(gm, name):
    """reads.fa.gz through a session on the FASTA-built index: ix.sam_header() (no command line, so no @PG) + the records equal the reference's -L run"""
    c = load_case(name)
    p = _params(gm, c)
    ix = gm.Index.from_fasta(c["paths"], seeds=c["seeds"], params=p)
    s = gm.Session(ix, params=p, max_batch_reads=1024)
    try:
        got = ix.sam_header() + s.map_reads_file(c["reads_path"])
    finally:
        s.close(); ix.close()
    with gzip.open(os.path.join(c["dir"], "from_index.sam.gz"), "rb") as f: want = f.read()
    assert got == want, _first_diff(got, want)


@pytest.mark.gpu
def test_sam_header_rg_and_pg_lines(gm):
    """the @RG / @PG lines against the literal format strings of gmapper.c:3000,3007"""
    c = load_case("names")
    ix = gm.Index.from_fasta(c["paths"], seeds=c["seeds"])
    try:
        plain = ix.sam_header()
        full = ix.sam_header(rg_id="grp1", rg_sample="smp", command_line="gmapper-ls -N 2 reads.fa genome.fa")
        sq = b"".join(b"@SQ\tSN:%s\tLN:%u\n" % (n, l) for n, l in ix.contigs())
    finally:
        ix.close()
    assert plain == b"@HD\tVN:%s\tSO:%s\n" % (b"1.0", b"unsorted") + sq
    assert full == plain + b"@RG\tID:%s\tSM:%s\n" % (b"grp1", b"smp") + b"@PG\tID:%s\tVN:%s\tCL:%s\n" % (b"gmapper", b"2.2.3", b"gmapper-ls -N 2 reads.fa genome.fa")


def _chunk_sizes():
    text = read_text(load_case("chunk_edges")["paths"][0])
    h = text.index(b">edge1")                            # a header in the middle of the file: chunks that end just before / just behind its '>'
    return [4096, 4099, 65536, h - 1, h + 1, 77]


@pytest.mark.gpu
@pytest.mark.parametrize("chunk", _chunk_sizes())
def test_chunk_edges_do_not_show(gm, chunk, monkeypatch, tmp_path):
    """tiny chunk sizes (a knob of the tuning build), also sizes that are no multiple of 16: headers, '#' lines and line ends fall on chunk and workgroup edges;
    the resident arrays stay those of the Python-parsed build"""
    monkeypatch.setenv("GM_FASTA_CHUNK", str(chunk))
    c = load_case("chunk_edges")
    ix = gm.Index.from_fasta(_plain_copies(c, tmp_path), seeds=c["seeds"])
    monkeypatch.delenv("GM_FASTA_CHUNK")
    try:
        _same_as_python_parsed(gm, c, ix)
    finally:
        ix.close()
    # and the small cases, whose lines are short, at a chunk size below their longest line
    monkeypatch.setenv("GM_FASTA_CHUNK", str(chunk if chunk < 4099 else 101))
    for name in ("ragged", "iupac", "twofiles_gz"):
        c = load_case(name)
        ix = gm.Index.from_fasta(c["paths"], seeds=c["seeds"])
        try:
            _same_as_python_parsed(gm, c, ix)
        finally:
            ix.close()


@pytest.mark.gpu
@pytest.mark.parametrize("chunk", [None, 4099])
def test_thousands_of_short_contigs(gm, chunk, tmp_path, monkeypatch):
    """5 000 contigs of 1..60 bases on one or two lines each: far more than 1 024 '>' lines in one chunk (the records beyond those fetched with the state words
    come with a second copy), several in one lane's 16 bytes, many per tile in no fixed order; at a small chunk size the names straddle chunk edges"""
    rng = np.random.default_rng(7)
    T = np.frombuffer(LETTERS, dtype=np.uint8)
    lines = []
    for k in range(5000):
        t = T[rng.integers(0, 4, int(rng.integers(1, 61)), dtype=np.uint8)].tobytes()
        cut = int(rng.integers(0, len(t) + 1))
        lines += [b">s%d scaffold" % k] + [x for x in (t[:cut], t[cut:]) if x]
    path = str(tmp_path / "scaffolds.fa")
    with open(path, "wb") as f: f.write(b"\n".join(lines) + b"\n")
    c = {"paths": [path], "seeds": ["11110111", "1101011011"], "colour": False}
    if chunk: monkeypatch.setenv("GM_FASTA_CHUNK", str(chunk))
    ix = gm.Index.from_fasta(c["paths"], seeds=c["seeds"])
    if chunk: monkeypatch.delenv("GM_FASTA_CHUNK")
    try:
        assert len(ix.contigs()) == 5000
        _same_as_python_parsed(gm, c, ix)
    finally:
        ix.close()


@pytest.mark.gpu
def test_more_header_lines_than_records_is_an_error(gm, tmp_path, monkeypatch):
    """'>' lines of two bytes back to back: more of them in a chunk than its record list holds (chunk / 4 + 16).  No valid file does that (every contig needs a
    name and a base); the count is checked before any record is used"""
    path = str(tmp_path / "flood_genome.fa")
    with open(path, "wb") as f: f.write(b">c0\nACGT\n" + b">\n" * 300)
    monkeypatch.setenv("GM_FASTA_CHUNK", "128")
    with pytest.raises(gm.GmError, match="flood_genome.fa.*header lines"):
        gm.Index.from_fasta([path])
    monkeypatch.delenv("GM_FASTA_CHUNK")
    with pytest.raises(gm.GmError, match="flood_genome.fa"):                 # at the real chunk size: the empty header line
        gm.Index.from_fasta([path])
    good = load_case("twofiles_gz")
    ix = gm.Index.from_fasta(good["paths"], seeds=good["seeds"]); ix.close()


BAD_INPUTS = {
    "crlf": b">c1\r\nACGTACGTAC\r\nACGT\r\n",
    "digit": b">c1\nACGTACGTAC\nACG7ACGT\n",
    "empty_contig": b">c1\nACGTACGT\n>c2\n>c3\nACGT\n",
    "empty_last_contig": b">c1\nACGTACGT\n>c2\n",
    "no_header_first": b"ACGTACGT\n>c1\nACGT\n",
    "blank_first_line": b"\n>c1\nACGT\n",
    "mark_inside_a_line": b">c1\nACGT>ACGT\n",
    "tab_in_sequence": b">c1\nACGT\tACGT\n",
    "empty_file": b"",
}


@pytest.mark.gpu
@pytest.mark.parametrize("what", sorted(BAD_INPUTS) + ["missing_file", "truncated_gzip"])
def test_bad_genome_files_are_refused_and_the_device_stays_usable(gm, what, tmp_path):
    """each is rejected by an ordinary check (GM_E_ARG, the file named in gm_last_error()), nothing is indexed, and a good call on the same device succeeds after it"""
    path = str(tmp_path / (what + "_genome.fa"))
    if what == "truncated_gzip":                                            # a download cut in half: zlib inflates what is there and then reports no more bytes
        with open(load_case("chunk_edges")["paths"][0], "rb") as f: whole = f.read()
        assert whole[:2] == b"\x1f\x8b"
        with open(path, "wb") as f: f.write(whole[:len(whole) // 2])
    elif what != "missing_file":
        with open(path, "wb") as f: f.write(BAD_INPUTS[what])
    good = load_case("twofiles_gz")
    L = gm.lib()
    for files in ([path], [good["paths"][0], path]):                       # alone, and behind a good file
        arr = (C.c_char_p * len(files))(*[os.fsencode(x) for x in files]); h = C.c_void_p()
        rc = L.gm_index_build_fasta(C.byref(h), 0, len(files), arr, 0, None, None)
        assert rc == -2 and not h.value, (what, rc)                         # GM_E_ARG
        assert os.path.basename(path).encode() in L.gm_last_error(), L.gm_last_error()
        with pytest.raises(gm.GmError, match=what + "_genome.fa"):
            gm.Index.from_fasta(files)
    if what in ("crlf", "digit", "mark_inside_a_line", "tab_in_sequence"):
        msg = L.gm_last_error()
        bad_at = {"crlf": 15, "digit": 18, "mark_inside_a_line": 8, "tab_in_sequence": 8}[what]
        assert b"[c1]" in msg and (b"offset %d" % bad_at) in msg, msg
    ix = gm.Index.from_fasta(good["paths"], seeds=good["seeds"])
    assert [n for n, _ in ix.contigs()] == [b"zA", b"zB", b"aC"]
    ix.close()


@pytest.mark.gpu
def test_release_build_reads_genome_fasta_too():
    """the release build (TUNING=0: GM_FASTA_CHUNK is not read, the chunks have their real size) runs the file / array comparison for ragged and iupac, in a
    child interpreter with GM_LIB_PATH on libgmapper_hip_release.so"""
    rel = os.path.join(ROOT, "shrimp_amd", "libgmapper_hip_release.so")
    assert os.path.exists(rel), "make -C shrimp_amd/csrc release (or __graft_entry__.build()) has not run"
    env = dict(os.environ, GM_LIB_PATH=rel, GM_FASTA_CHUNK="64")          # (ignored by that build)
    p = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-x", "-m", "gpu", "-p", "no:cacheprovider",
                        "-k", "test_fasta_index_equals_reference_files_and_packed_build and (ragged or iupac)"],
                       capture_output=True, text=True, env=env, cwd=ROOT, timeout=900)
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-2000:]
    import re
    m = re.search(r"(\d+) passed", p.stdout)
    assert m and int(m.group(1)) == 2, p.stdout[-500:]
