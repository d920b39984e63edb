"""A BAM writer in plain Python and the cases of the `convert` tests.

A record is a dict: name (str, without the NUL), flag, ref, pos, mapq, cigar (list of u32 words), seq_len, aux (a list of
(tag, type, value): A c C s S i I f Z H as their Python values, B as (subtype, [values])).  Two keys exist for the malformed
cases only: "raw_tail" (bytes put behind the aux fields as they are) and "block_size" (the field as written, whatever the record
holds).  The layout is the SAM/BAM specification's, sections 4.1 (BGZF) and 4.2 (BAM): no BAM of a real aligner is at hand.

A case is a dict: records, ref_names, cuts (the offsets of the uncompressed file at which a new BGZF block begins), stored (the
indices of blocks written as stored deflate blocks), empty_after (indices of blocks behind which an empty block stands), eof
(write the EOF marker), span_recs (the record indices at which the spans of a device call begin)."""
import struct
import zlib

_FIX = {"A": "<c", "c": "<b", "C": "<B", "s": "<h", "S": "<H", "i": "<i", "I": "<I", "f": "<f"}
BGZF_EOF = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")
CHUNK_RUNS = 10001


def aux_bytes(aux):
    out = bytearray()
    for tag, ty, val in aux:
        out += tag.encode() + ty.encode()
        if ty in _FIX:
            out += struct.pack(_FIX[ty], val.encode() if ty == "A" else val)
        elif ty in "ZH":
            out += val.encode() + b"\0"
        elif ty == "B":
            sub, vals = val
            out += sub.encode() + struct.pack("<I", len(vals)) + b"".join(struct.pack(_FIX[sub], v) for v in vals)
        else:
            raise ValueError(ty)
    return bytes(out)


def record_bytes(r):
    name = r["name"].encode() + b"\0"
    cigar, l_seq = r.get("cigar", []), r.get("seq_len", 0)
    body = struct.pack("<iiBBHHHIiii", r.get("ref", 0), r.get("pos", 0), len(name), r.get("mapq", 0), 4680, len(cigar), r.get("flag", 0), l_seq, -1, -1, 0)
    body += name + b"".join(struct.pack("<I", c) for c in cigar) + bytes((l_seq + 1) // 2) + b"\xff" * l_seq
    body += aux_bytes(r.get("aux", [])) + r.get("raw_tail", b"")
    return struct.pack("<I", r.get("block_size", len(body))) + body


def header_bytes(ref_names, text=b"@HD\tVN:1.6\n"):
    out = b"BAM\1" + struct.pack("<i", len(text)) + text + struct.pack("<i", len(ref_names))
    for n in ref_names:
        out += struct.pack("<i", len(n) + 1) + n.encode() + b"\0" + struct.pack("<i", 1000)
    return out


def stream_of(case):
    """the record stream (what stands behind the BAM header) and every record's offset in it"""
    offs, out = [], bytearray()
    for r in case["records"]:
        offs.append(len(out))
        out += record_bytes(r)
    if case.get("stream_tail"):
        out += case["stream_tail"]
    return bytes(out), offs


def span_table(case):
    _, offs = stream_of(case)
    return [offs[i] for i in case.get("span_recs", [0])] if offs else ([0] if case.get("stream_tail") else [])


def bgzf_block(data, stored=False):
    if stored:
        comp = b"\x01" + struct.pack("<HH", len(data), len(data) ^ 0xFFFF) + data   # one final stored deflate block
    else:
        z = zlib.compressobj(6, zlib.DEFLATED, -15)
        comp = z.compress(data) + z.flush()
    head = b"\x1f\x8b\x08\x04" + bytes(4) + b"\x00\xff" + struct.pack("<H", 6) + b"BC" + struct.pack("<HH", 2, len(comp) + 25)
    return head + comp + struct.pack("<II", zlib.crc32(data) & 0xFFFFFFFF, len(data))


def plain_of(case):
    return header_bytes(case["ref_names"]) + stream_of(case)[0]


def bam_bytes(case):
    plain = plain_of(case)
    cuts = sorted(set(c for c in case.get("cuts", []) if 0 < c < len(plain)))
    edges = [0] + cuts + [len(plain)]
    for a, b in zip(list(edges), list(edges[1:])):   # a BGZF block holds at most 64 KiB
        edges += list(range(a + 60000, b, 60000))
    edges = sorted(set(edges))
    out = bytearray()
    for i, (a, b) in enumerate(zip(edges, edges[1:])):
        out += bgzf_block(plain[a:b], stored=i in case.get("stored", ()))
        if i in case.get("empty_after", ()):
            out += bgzf_block(b"")
    if case.get("eof", True):
        out += BGZF_EOF
    return bytes(out)


def header_len(case):
    return len(header_bytes(case["ref_names"]))


# ---------------------------------------------------------------------------------------------------------------- records
REFS = ["t%d" % i for i in range(7)]
CR, UR = "ACGTACGTACGTACGT", "TTGCAATTGCAA"


def rec(name, ref=0, flag=0, cr=CR, ur=UR, score=None, score_type="i", before=(), after=(), tags_last=False, **kw):
    aux = list(before)
    mine = ([("CR", "Z", cr)] if cr is not None else []) + ([("UR", "Z", ur)] if ur is not None else [])
    sc = [("AS", score_type, score)] if score is not None else []
    aux += (sc + list(after) + mine) if tags_last else (mine + sc + list(after))
    return dict(name=name, ref=ref, flag=flag, aux=aux, **kw)


def filler(nbytes, name="f", flag=0x4):
    """a record of exactly nbytes (>= 48), dropped by its flag unless told otherwise; it carries CR and UR like any other"""
    base = dict(name=name, flag=flag, ref=0, aux=[("CR", "Z", "A"), ("UR", "Z", "A"), ("XP", "Z", "")])
    pad = nbytes - len(record_bytes(base))
    assert pad >= 0, nbytes
    base["aux"][2] = ("XP", "Z", "x" * pad)
    return base


def case(name, records, **kw):
    c = dict(name=name, records=records, ref_names=kw.pop("ref_names", REFS), filters=kw.pop("filters", (False, True)))
    c.update(kw)
    return c


def scored(n, name, best_at=(0,), lo=-7, hi=30, **kw):
    return [rec(name, ref=i % len(REFS), flag=0x10 if i % 3 == 0 else 0, score=hi if i in best_at else lo - (i % 5), **kw) for i in range(n)]


def tile_edge_cases(lim):
    """a record that starts on the tile's last byte; a block_size field that straddles the tile's end (two bytes on each side)"""
    T = lim["parse_tile"]
    out = []
    for label, start in (("last_byte", T - 1), ("straddle", T - 2), ("exact", T)):
        recs = [rec("a0", score=3)]
        used = len(record_bytes(recs[0]))
        recs.append(filler(start - used))
        recs += [rec("edge", ref=2, score=5), rec("edge", ref=3, flag=0x10, score=9), rec("z", ref=1, score=1)]
        c = case("tile_" + label, recs)
        assert stream_of(c)[1][2] == start
        out.append(c)
    return out


def span_cases(lim):
    """spans that begin in the middle of a run; a whole span of flag-dropped records between two records of one name, so that the
    predecessor of the second lies two spans back"""
    recs = [rec("r", ref=1, score=4)] + [filler(200, name="d%d" % i) for i in range(5)] + [rec("r", ref=2, score=4, flag=0x10), rec("s", ref=3, score=1)]
    a = case("dropped_span_between", recs, span_recs=[0, 1, 6])
    recs = [rec("q%d" % (i // 3), ref=i % 7, score=i % 4) for i in range(60)]
    b = case("spans_inside_runs", recs, span_recs=[0, 1, 2, 4, 11, 30, 59])
    return [a, b]


def name_cases():
    n253 = "n" * 253
    recs = [rec("a"), rec("a", ref=1), rec("x" * 254, ref=2), rec("x" * 254, ref=3), rec(n253 + "A", ref=1), rec(n253 + "B", ref=2), rec(n253 + "B", ref=4),
            rec("pre", ref=1), rec("prefix", ref=2), rec("prefi", ref=3), rec("A", ref=1), rec("B", ref=2), rec("A", ref=3)]
    return [case("names", [dict(r, aux=r["aux"] + [("AS", "c", 1)]) for r in recs])]


def run_length_cases(lim):
    L = lim["lane_alns"]
    recs = []
    for k, n in enumerate([1, 2, 63, 64, 65, L - 1, L, L + 1]):
        recs += scored(n, "run%d" % k, best_at=(0, n - 1) if n > 2 else (0,))
    a = case("run_lengths", recs, span_recs=[0, 70, 140])
    n = 3000
    b = case("long_run_across_tiles", [rec("pre", score=1)] + scored(n, "big", best_at=(7, 1500, n - 1)) + [rec("post", score=2)], span_recs=[0, 900, 2200])
    return [a, b]


def score_cases():
    def run(name, scores, ty="i"):
        return [rec(name, ref=i % 7, score=s, score_type=ty) for i, s in enumerate(scores)]
    recs = run("first", [9, 1, 2]) + run("last", [1, 2, 9]) + run("tied", [5, 9, 9, 1, 9]) + run("neg", [-5, -2, -9, -2])
    recs += run("c", [-3, 4], "c") + run("C", [200, 100], "C") + run("s", [-300, 300], "s") + run("S", [60000, 1], "S") + run("i", [-70000, 70000], "i") + run("I", [70000, 5], "I")
    recs += run("wrap", [4294967295, 4294967294, 7], "I")   # as i32: -1, -2, 7
    recs += run("wrap2", [4294967295, 4294967294], "I")   # -1 beats -2
    return [case("scores", recs)]


def aux_cases():
    arrays = [("X" + s, "B", (s, [1, 2, 3] if s != "f" else [1.5, 2.5])) for s in "cCsSiIf"]
    recs = [rec("first_tags", score=1), rec("last_tags", ref=1, score=2, tags_last=True, before=[("NH", "C", 3), ("XA", "A", "q")])]
    recs += [rec("arrays", ref=2, score=1, before=arrays + [("XZ", "Z", "CR:Z:TTTT"), ("XH", "H", "1AE3"), ("XE", "B", ("i", []))])]
    recs += [rec("decoys", ref=3, score=3, before=[("CB", "Z", "GGGGGGGGGGGGGGGG"), ("UB", "Z", "CCCCCCCCCCCC"), ("Xf", "f", 1.25), ("Xs", "s", -2), ("XS", "S", 9)])]
    a = case("aux", recs)
    b = case("no_aux_on_a_follower", [rec("h", ref=1), dict(name="h", ref=2, flag=0x10, aux=[]), rec("k", ref=3)], filters=(False,))
    return [a, b]


def sequence_cases():
    out = []
    lens = (1, 4, 5, 8, 9, 16, 17, 32)
    for n, m in zip(lens, lens[::-1]):   # (the UMI runs through the widths the other way round)
        cr, ur = ("ACGT" * 8)[:n], ("GATC" * 8)[:m]
        out.append(case("lengths_%d_%d" % (n, len(ur)), [rec("a", cr=cr, ur=ur, score=1), rec("b", ref=1, cr=cr[::-1], ur=ur[::-1], score=2, flag=0x10)]))
    recs = [rec("ok"), rec("n_first", ref=1, cr="N" + CR[1:]), rec("n_last", ref=2, ur=UR[:-1] + "N"), rec("n_both", ref=3, cr="N" + CR[1:], ur="N" + UR[1:]),
            rec("longer", ref=4, cr=CR + "G", ur=UR + "T"), rec("shorter", ref=5, cr=CR[:-1], ur=UR[:-2])]
    out.append(case("n_and_lengths", [dict(r, aux=r["aux"] + [("AS", "C", 1)]) for r in recs]))
    recs = [rec("a", ref=1), rec("nn_bc", ref=2, cr="NN" + CR[2:]), rec("nn_bc", ref=3, cr="NN" + CR[2:]), rec("b", ref=3), rec("nn_umi", ref=4, ur="N" + UR[1:-1] + "N"), rec("c", ref=5),
            rec("a", ref=1), rec("nn", ref=2, cr="ANNA" + CR[4:]), rec("a", ref=6)]   # two surviving runs of one name around a dropped one stay two runs
    out.append(case("two_n", recs, two_n=True, filters=(False,)))
    recs = [rec("a", ref=1, score=1), rec("nn", ref=2, cr="NN" + CR[2:]), rec("nn", ref=2, cr="NN" + CR[2:]), rec("b", ref=3, score=2)]   # no AS is asked of a dropped run
    out.append(case("two_n_without_scores", recs, two_n=True, filters=(True,)))
    return out


def flag_cases():
    recs = [rec("u", flag=0x4, cr="ACGTA", ur="TTG"), rec("a", ref=1, cr="GGGTA", ur="CAT"), rec("a", ref=2, flag=0x800, cr="GGGTA", ur="CAT"), rec("a", ref=3, flag=0x804, cr="GGGTA", ur="CAT"),
            rec("a", ref=4, flag=0x100, cr="GGGTA", ur="CAT"), rec("a", ref=5, flag=0x10, cr="GGGTA", ur="CAT"), rec("b", ref=6, flag=0x110 | 0x1 | 0x40, cr="TTTTA", ur="AAA")]
    a = case("flags", recs, filters=(False,))   # the first record is unmapped yet sets the lengths 5 and 3
    b = case("all_dropped", [rec("u%d" % i, flag=0x4 if i % 2 else 0x800) for i in range(9)])
    return [a, b]


def chunk_cases():
    out = []
    for n in (10000, 10001, 10002, 20002, 20003):
        recs = [rec("r%d" % i, ref=i % 7, cr=CR[:8], ur=UR[:6], flag=0x10 if i % 2 else 0) for i in range(n)]
        recs.insert(5000, rec("r4999", ref=3, cr=CR[:8], ur=UR[:6]))   # one run of two
        out.append(case("runs_%d" % n, recs, filters=(False,), span_recs=list(range(0, n, 997))))
    recs = [rec("r%d" % i, ref=i % 7, cr=CR[:8], ur=UR[:6]) for i in range(10003)]
    recs[10000] = rec("r10000", cr="NN" + CR[2:8], ur=UR[:6])   # the dropped run stands where a chunk would end: the next run still joins chunk 0
    out.append(case("dropped_run_on_the_boundary", recs, two_n=True, filters=(False,), span_recs=[0, 4000, 10000, 10001]))
    return out


def shape_cases():
    recs = [rec("a", ref=0, cigar=[], seq_len=0), rec("b", ref=0, cigar=[(10 << 4), (2 << 4) | 1, (5 << 4)], seq_len=17), rec("b", ref=0, cigar=[(8 << 4)], seq_len=8, flag=0x10)]
    a = case("one_reference", recs, ref_names=["only"], filters=(False,))
    b = case("last_reference", [rec("a", ref=len(REFS) - 1), rec("a", ref=0)], filters=(False,))
    return [a, b]


def container_cases():
    recs = [rec("q%d" % (i // 2), ref=i % 7, score=i % 3) for i in range(40)]
    base = case("container", recs)
    h = header_len(base)
    offs = stream_of(base)[1]
    out = [dict(base, name="record_split", cuts=[h + offs[5] + 20]), dict(base, name="block_size_split", cuts=[h + offs[7] + 2]),
           dict(base, name="header_split", cuts=[3, h - 2]), dict(base, name="empty_block", cuts=[h + offs[9]], empty_after=[0]),
           dict(base, name="no_eof", eof=False), dict(base, name="stored_block", cuts=[h + offs[3], h + offs[20] + 7], stored=[1])]
    return out


MALFORMED = ("block_size_too_small", "block_size_below_fixed", "aux_short_of_the_end", "aux_string_without_nul", "block_size_past_the_stream", "stream_ends_inside_block_size")


def error_cases():
    """(case, filter_best, code name, record index named): one case per sentence of the error list"""
    good = [rec("a", ref=1, score=1), rec("a", ref=2, score=2), rec("b", ref=3, score=3)]
    def with_bad(bad, at=2):
        r = list(good)
        r.insert(at, bad)
        return r
    out = [
        (case("ref_negative", with_bad(rec("c", ref=-1, score=1))), False, "BAD_INPUT", 2),
        (case("ref_too_large", with_bad(rec("c", ref=len(REFS), score=1))), False, "BAD_INPUT", 2),
        (case("head_without_cr", with_bad(rec("c", cr=None, score=1))), False, "BAD_INPUT", 2),
        (case("head_without_ur", with_bad(rec("c", ur=None, score=1), at=3)), False, "BAD_INPUT", 3),
        (case("cr_not_z", with_bad(dict(name="c", ref=1, aux=[("CR", "i", 5), ("UR", "Z", UR)]))), False, "BAD_INPUT", 2),
        (case("ur_not_z", with_bad(dict(name="c", ref=1, aux=[("CR", "Z", CR), ("UR", "A", "x")]))), False, "BAD_INPUT", 2),
        (case("bad_base", with_bad(rec("c", cr=CR[:-1] + "a", score=1))), False, "BAD_INPUT", 2),
        (case("bad_base_umi", with_bad(rec("c", ur="ACGU" + UR[4:], score=1))), False, "BAD_INPUT", 2),
        (case("no_score", with_bad(rec("a", ref=4), at=1)), True, "BAD_INPUT", 1),
        (case("float_score", with_bad(rec("a", ref=4, score=1.0, score_type="f"), at=1)), True, "BAD_INPUT", 1),
        (case("block_size_too_small", with_bad(dict(rec("c", score=1, seq_len=9), block_size=40))), False, "BAD_INPUT", 2),
        (case("block_size_below_fixed", with_bad(dict(rec("c", score=1), block_size=12))), False, "BAD_INPUT", 2),
        (case("aux_short_of_the_end", with_bad(dict(rec("c", score=1), raw_tail=b"XY"))), False, "BAD_INPUT", 2),
        (case("aux_string_without_nul", with_bad(dict(rec("c", score=1), raw_tail=b"XYZabc"))), False, "BAD_INPUT", 2),
        (case("block_size_past_the_stream", good + [dict(rec("c", score=1), block_size=4000)]), False, "BAD_INPUT", 3),
        (case("stream_ends_inside_block_size", good, stream_tail=b"\x30\x00"), False, "BAD_INPUT", 3),
    ]
    return out


def device_cases(lim):
    """the cases that differ in their record stream: what the device entry is run on"""
    out = tile_edge_cases(lim) + span_cases(lim) + name_cases() + run_length_cases(lim) + score_cases() + aux_cases() + sequence_cases() + flag_cases()
    return out + shape_cases()


def all_cases(lim):
    """... and the container cases: one record stream cut into BGZF blocks in six ways, which only a reader of the file sees"""
    return device_cases(lim) + container_cases()
