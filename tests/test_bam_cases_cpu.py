"""CPU tests of the BAM writer of tests/bam_cases.py: every case's file is read back with gzip.decompress (it takes multi-member
streams: an independent check of the BGZF container), then by a minimal BAM reader of this file's own, which must return the
case's record dicts."""
import gzip
import struct

import pytest

import bam_cases as B
from util import pkg

_SIZE = {"A": 1, "c": 1, "C": 1, "s": 2, "S": 2, "i": 4, "I": 4, "f": 4}


def read_aux(b):
    out, p = [], 0
    while p < len(b):
        tag, ty = b[p:p + 2].decode(), chr(b[p + 2])
        p += 3
        if ty in _SIZE:
            v = struct.unpack_from(B._FIX[ty], b, p)[0]
            out.append((tag, ty, v.decode() if ty == "A" else v))
            p += _SIZE[ty]
        elif ty in "ZH":
            e = b.index(b"\0", p)
            out.append((tag, ty, b[p:e].decode()))
            p = e + 1
        else:
            assert ty == "B"
            sub, n = chr(b[p]), struct.unpack_from("<I", b, p + 1)[0]
            out.append((tag, ty, (sub, [struct.unpack_from(B._FIX[sub], b, p + 5 + i * _SIZE[sub])[0] for i in range(n)])))
            p += 5 + n * _SIZE[sub]
    return out


def read_bam(plain):
    assert plain[:4] == b"BAM\1"
    l_text = struct.unpack_from("<i", plain, 4)[0]
    p = 8 + l_text
    n_ref = struct.unpack_from("<i", plain, p)[0]
    p += 4
    names = []
    for _ in range(n_ref):
        ln = struct.unpack_from("<i", plain, p)[0]
        names.append(plain[p + 4:p + 4 + ln - 1].decode())
        p += 4 + ln + 4
    recs = []
    while p < len(plain):
        bs = struct.unpack_from("<I", plain, p)[0]
        ref, pos, l_name, mapq, _bin, n_cig, flag, l_seq = struct.unpack_from("<iiBBHHHI", plain, p + 4)
        q = p + 36
        name = plain[q:q + l_name - 1].decode()
        q += l_name
        cigar = list(struct.unpack_from("<%dI" % n_cig, plain, q))
        q += 4 * n_cig + (l_seq + 1) // 2 + l_seq
        recs.append(dict(name=name, ref=ref, flag=flag, cigar=cigar, seq_len=l_seq, aux=read_aux(plain[q:p + 4 + bs])))
        p += 4 + bs
    return names, recs


def normal(r):
    return dict(name=r["name"], ref=r.get("ref", 0), flag=r.get("flag", 0), cigar=list(r.get("cigar", [])), seq_len=r.get("seq_len", 0), aux=[tuple(a) for a in r.get("aux", [])])


@pytest.fixture(scope="module")
def cases():
    return B.all_cases(pkg.convert_limits()) + B.chunk_cases()[:2]


def test_every_case_reads_back(cases):
    assert len(cases) >= 30
    for c in cases:
        plain = gzip.decompress(B.bam_bytes(c))
        assert plain == B.plain_of(c), c["name"]
        names, recs = read_bam(plain)
        assert names == c["ref_names"] and recs == [normal(r) for r in c["records"]], c["name"]


def test_the_container_cases_hold_what_they_say():
    cs = {c["name"]: c for c in B.container_cases()}
    def blocks(buf):
        out, p = [], 0
        while p < len(buf):
            assert buf[p:p + 4] == b"\x1f\x8b\x08\x04" and buf[p + 12:p + 16] == b"BC\x02\x00"
            n = struct.unpack_from("<H", buf, p + 16)[0] + 1
            out.append(buf[p:p + n])
            p += n
        return out
    h = B.header_len(cs["record_split"])
    offs = B.stream_of(cs["record_split"])[1]
    bl = blocks(B.bam_bytes(cs["record_split"]))
    assert len(bl) == 3 and bl[-1] == B.BGZF_EOF and struct.unpack_from("<I", bl[0], len(bl[0]) - 4)[0] == h + offs[5] + 20
    bl = blocks(B.bam_bytes(cs["block_size_split"]))
    assert struct.unpack_from("<I", bl[0], len(bl[0]) - 4)[0] == h + offs[7] + 2
    bl = blocks(B.bam_bytes(cs["empty_block"]))
    assert [struct.unpack_from("<I", b, len(b) - 4)[0] for b in bl][1] == 0 and len(bl) == 4
    assert blocks(B.bam_bytes(cs["no_eof"]))[-1] != B.BGZF_EOF
    bl = blocks(B.bam_bytes(cs["stored_block"]))
    assert bl[1][18] == 1 and bl[0][18] != 1   # a stored deflate block: BFINAL = 1, BTYPE = 00


def test_the_tile_and_span_cases_stand_where_they_say():
    lim = pkg.convert_limits()
    T = lim["parse_tile"]
    starts = [B.stream_of(c)[1][2] for c in B.tile_edge_cases(lim)]
    assert starts == [T - 1, T - 2, T]
    c = B.span_cases(lim)[0]
    assert all(r["flag"] & 0x4 for r in c["records"][1:6]) and c["records"][0]["name"] == c["records"][6]["name"] and c["span_recs"] == [0, 1, 6]
    names = [r["name"] for r in B.name_cases()[0]["records"]]
    assert {len(n) + 1 for n in names} >= {2, 255} and names[4][:253] == names[5][:253] and names[4] != names[5] and names[8].startswith(names[7])
