"""The SAM record writer beyond its stack buffer: with read names of 7 000 characters every record is larger than the buffer a record is staged in, so each one
takes the grow-in-place path and hangs on the writer's size bound -- a branch no reference golden reaches.  The reference copies QNAME verbatim, so the expected
text is its golden for the fixture with only the QNAME field of every record replaced."""
import pytest
from tests import oracle_api as oa

pytestmark = pytest.mark.gpu

NAME_LEN = 7000


@pytest.fixture(scope="module")
def gm():
    try:                    # (torch's HIP runtime first, as in test_gpu_parity.py)
        import torch
        torch.cuda.init()
    except Exception:
        pass
    from shrimp_amd import gmapper
    if gmapper.lib().gm_device_count() < 1:
        pytest.fail("no HIP device: the product path has no CPU fallback")
    return gmapper


def _long(qname: bytes) -> bytes:
    """a name of NAME_LEN characters that still tells the reads apart"""
    return (qname + b".").ljust(NAME_LEN, b"n")


def _with_long_qnames(sam: bytes) -> bytes:
    out = []
    for line in sam.split(b"\n"):
        if line and not line.startswith(b"@"):
            q, rest = line.split(b"\t", 1)
            line = _long(q) + b"\t" + rest
        out.append(line)
    return b"\n".join(out)


def _first_diff(a: bytes, b: bytes):
    la, lb = a.split(b"\n"), b.split(b"\n")
    for i, (x, y) in enumerate(zip(la, lb)):
        if x != y:
            k = next((j for j, (c, d) in enumerate(zip(x, y)) if c != d), min(len(x), len(y)))
            return i, len(x), len(y), k, x[max(0, k - 40):k + 120], y[max(0, k - 40):k + 120]
    return min(len(la), len(lb)), len(la), len(lb)


def test_unpaired_records_beyond_the_stack_buffer(gm):
    """stress_60bp: 3 000 letter-space reads, mapped records on both strands"""
    contigs, reads, sam = oa.load_golden("stress_60bp")
    p = gm.default_params()
    ix = gm.Index(contigs, params=p)
    s = gm.Session(ix, params=p, max_batch_reads=4096)
    got = oa.sam_header(contigs) + s.map_reads(reads, names=[_long(b"r%d" % i) for i in range(len(reads))])
    s.close(); ix.close()
    want = _with_long_qnames(sam)
    assert got == want, _first_diff(got, want)


def test_colour_space_records_beyond_the_stack_buffer(gm):
    """stress_cs_60col_unal: colour-space records (CS / XX tags) and the unaligned record"""
    contigs, reads, sam = oa.load_golden("stress_cs_60col_unal")
    p = gm.default_params_cs()
    p.sam_unaligned = 1
    ix = gm.Index(contigs, params=p)
    s = gm.Session(ix, params=p, max_batch_reads=1024)
    got = oa.sam_header(contigs) + s.map_reads_cs(reads, names=[_long(b"r%d" % i) for i in range(len(reads))])
    s.close(); ix.close()
    want = _with_long_qnames(sam)
    assert got == want, _first_diff(got, want)


def test_paired_records_beyond_the_stack_buffer(gm):
    """stress_pairs_2x100: 1 200 pairs named <N>:1 / <N>:2, so that QNAME is <N>; mate fields, half-paired and unmapped-mate records"""
    g = oa.load_golden_pairs("stress_pairs_2x100")
    assert g["names1"][7] == b"q7:1" and g["names2"][7] == b"q7:2"             # the golden's QNAME of pair i is q<i>
    n = len(g["names1"])
    ix = gm.Index(g["contigs"], names=g["contig_names"])
    s = gm.Session(ix, max_batch_reads=4096)
    got = oa.sam_header(g["contigs"], g["contig_names"]) + s.map_pairs(g["m1"], g["m2"], [_long(b"q%d" % i) + b":1" for i in range(n)],
                                                                        [_long(b"q%d" % i) + b":2" for i in range(n)], mode=g["mode"],
                                                                        min_insert=g["ins"][0], max_insert=g["ins"][1])
    s.close(); ix.close()
    want = _with_long_qnames(g["sam"])
    assert got == want, _first_diff(got, want)
