"""A bit-level deflate writer and the cases of the BGZF inflater's tests.  zlib never writes most of the format's edges - a code
of 15 bits, a single distance code, a repeat of code lengths that runs from the length alphabet into the distance alphabet, a
stored block behind five pending bits - so the payloads here are spelled out: deflate blocks from explicit element lists and,
for dynamic blocks, explicit code lengths, explicit code-length items and an explicit HCLEN.

A block is ("stored", data[, opts]), ("fixed", elems[, opts]) or ("dynamic", elems, opts).  An element is ("lit", byte),
("copy", len, dist), and for the malformed cases ("litsym", symbol), ("distsym", symbol) - the symbol's code and nothing else -
and ("bits", value, n).  Options of a dynamic block: lit_lens / dist_lens ({symbol: length}; default: a complete code over the
symbols the elements use), nlen / ndist (HLIT + 257, HDIST + 1; default: the smallest that hold the lengths), items (the
code-length items: an int 0..15, or (16, rep), (17, rep), (18, rep); default: a greedy run-length encoding), cl_lens ({code-length
symbol: length}; default: a complete code over the items' symbols), hclen (HCLEN + 4; default: the smallest).  Options of any
block: eob=False (no end-of-block code), and of a stored block: len / nlen (the fields as written), final (BFINAL as written).

HCLEN = 4 sends lengths for the code-length symbols 16, 17, 18 and 0 alone: such a block can spell no length but 0, so it has no
end-of-block code and cannot be valid.  It stands among CORRUPT; the smallest valid HCLEN, 5 (all codes of 8 bits), among VALID."""
import struct
import zlib

import numpy as np

import inflate_judge as ij

CL_ORDER = ij.CL_ORDER


class BitWriter:
    def __init__(self):
        self.bits = []

    def put(self, v, n):            # a value, lowest bit first
        self.bits += [(v >> k) & 1 for k in range(n)]

    def put_code(self, code, n):    # a Huffman code, its first bit first
        self.bits += [(code >> (n - 1 - k)) & 1 for k in range(n)]

    def align(self):
        self.bits += [0] * (-len(self.bits) % 8)

    def bytes(self):
        b = self.bits + [0] * (-len(self.bits) % 8)
        return bytes(sum(b[i + k] << k for k in range(8)) for i in range(0, len(b), 8))


def canonical(lens):
    """{symbol: (code, length)} of RFC 1951 3.2.2 for lens, a list"""
    count = [0] * 16
    for l in lens:
        count[l] += 1
    count[0] = 0
    code, nxt = 0, [0] * 16
    for l in range(1, 16):
        code = (code + count[l - 1]) << 1
        nxt[l] = code
    out = {}
    for s, l in enumerate(lens):
        if l:
            out[s] = (nxt[l], l)
            nxt[l] += 1
    return out


def complete_lens(symbols):
    """{symbol: length} of a complete code over the symbols (one symbol: a single code of length 1)"""
    symbols = sorted(symbols)
    n = len(symbols)
    if n == 1:
        return {symbols[0]: 1}
    k = n.bit_length() - 1
    r = n - (1 << k)
    return {s: (k + 1 if i < 2 * r else k) for i, s in enumerate(symbols)}


def chain_lens(symbols):
    """16 symbols with lengths 1, 2, ..., 14, 15, 15: complete, and two codes of 15 bits (the last two symbols)"""
    assert len(symbols) == 16
    return {s: min(i + 1, 15) for i, s in enumerate(symbols)}


def len_symbol(n):
    for s in range(28, -1, -1):
        if ij.LEN_BASE[s] <= n and (s == 28 or n - ij.LEN_BASE[s] < 1 << ij.LEN_EXTRA[s]):
            return 257 + s, n - ij.LEN_BASE[s], ij.LEN_EXTRA[s]
    raise ValueError(n)


def dist_symbol(d):
    for s in range(29, -1, -1):
        if ij.DIST_BASE[s] <= d:
            return s, d - ij.DIST_BASE[s], ij.DIST_EXTRA[s]
    raise ValueError(d)


def greedy_items(seq):
    out, i = [], 0
    while i < len(seq):
        v, j = seq[i], i
        while j < len(seq) and seq[j] == v:
            j += 1
        run = j - i
        if v == 0 and run >= 3:
            rep = min(run, 138)
            out.append((18, rep) if rep >= 11 else (17, rep))
            i += rep
        elif v and run >= 4:
            rep = min(run - 1, 6)
            out += [v, (16, rep)]
            i += 1 + rep
        else:
            out.append(v)
            i += 1
    return out


def expand_items(items):
    seq = []
    for it in items:
        if isinstance(it, int):
            seq.append(it)
        elif it[0] == 16:
            seq += [seq[-1]] * it[1]
        else:
            seq += [0] * it[1]
    return seq


def as_list(d, n):
    return [d.get(s, 0) for s in range(n)]


def deflate(blocks, tail=b""):
    """(payload, the bytes it holds, pending): pending[i] = the bits that wait in front of stored block i's byte edge"""
    w, out, pending = BitWriter(), bytearray(), []
    for bi, blk in enumerate(blocks):
        kind, body = blk[0], blk[1]
        opts = dict(blk[2]) if len(blk) > 2 else {}
        final = opts.get("final", 1 if bi == len(blocks) - 1 else 0)
        w.put(final, 1)
        w.put({"stored": 0, "fixed": 1, "dynamic": 2, "reserved": 3}[kind], 2)
        if kind == "reserved":
            continue
        if kind == "stored":
            pending.append(len(w.bits) % 8)
            w.align()
            n = opts.get("len", len(body))
            w.put(n, 16)
            w.put(opts.get("nlen", n ^ 0xFFFF), 16)
            for b in body:
                w.put(b, 8)
            out += body
            continue
        elems = list(body)
        if kind == "fixed":
            lit_code, dist_code = canonical(ij.FIXED_LITLEN), canonical(ij.FIXED_DIST)
        else:
            used_l = {256} | {e[1] for e in elems if e[0] in ("lit", "litsym")} | {len_symbol(e[1])[0] for e in elems if e[0] == "copy"}
            used_d = {dist_symbol(e[2])[0] for e in elems if e[0] == "copy"} | {e[1] for e in elems if e[0] == "distsym"}
            lit_lens = opts.get("lit_lens") if opts.get("lit_lens") is not None else complete_lens(used_l | ({0, 1} - used_l if len(used_l) < 2 else set()))
            dist_lens = opts.get("dist_lens") if opts.get("dist_lens") is not None else (complete_lens(used_d) if used_d else {})
            nlen = opts.get("nlen", max(257, max(lit_lens, default=0) + 1))
            ndist = opts.get("ndist", max(1, max(dist_lens, default=0) + 1))
            seq = as_list(lit_lens, nlen) + as_list(dist_lens, ndist)
            items = opts.get("items")
            if items is None:
                items = greedy_items(seq)
            elif opts.get("check_items", True):
                assert expand_items(items) == seq, "the items do not spell the lengths"
            cl_used = {it if isinstance(it, int) else it[0] for it in items}
            cl_lens = opts.get("cl_lens") if opts.get("cl_lens") is not None else complete_lens(cl_used | ({0, 18} - cl_used if len(cl_used) < 2 else set()))
            hclen = opts.get("hclen", max(4, max(CL_ORDER.index(s) for s in cl_lens) + 1))
            w.put(nlen - 257, 5)
            w.put(ndist - 1, 5)
            w.put(hclen - 4, 4)
            for i in range(hclen):
                w.put(cl_lens.get(CL_ORDER[i], 0), 3)
            cl_code = canonical(as_list(cl_lens, 19))
            for it in items:
                s = it if isinstance(it, int) else it[0]
                assert s < 16 or {16: 3, 17: 3, 18: 11}[s] <= it[1] <= {16: 6, 17: 10, 18: 138}[s], it
                w.put_code(*cl_code[s])
                if s == 16:
                    w.put(it[1] - 3, 2)
                elif s == 17:
                    w.put(it[1] - 3, 3)
                elif s == 18:
                    w.put(it[1] - 11, 7)
            lit_code, dist_code = canonical(as_list(lit_lens, 288)), canonical(as_list(dist_lens, 32))
        for e in elems:
            if e[0] == "lit":
                w.put_code(*lit_code[e[1]])
                out.append(e[1])
            elif e[0] == "copy":
                s, x, xb = len_symbol(e[1])
                w.put_code(*lit_code[s])
                w.put(x, xb)
                s, x, xb = dist_symbol(e[2])
                w.put_code(*dist_code[s])
                w.put(x, xb)
                for _ in range(e[1]):
                    out.append(out[-e[2]])
            elif e[0] == "litsym":
                w.put_code(*lit_code[e[1]])
            elif e[0] == "distsym":
                w.put_code(*dist_code[e[1]])
            else:
                w.put(e[1], e[2])
        if opts.get("eob", True):
            w.put_code(*lit_code[256])
    return w.bytes() + tail, bytes(out), pending


def bgzf_wrap(body, crc, isize):
    head = b"\x1f\x8b\x08\x04" + bytes(4) + b"\x00\xff" + struct.pack("<H", 6) + b"BC" + struct.pack("<HH", 2, len(body) + 25)
    return head + body + struct.pack("<II", crc & 0xFFFFFFFF, isize)


class Payload:
    """a BGZF block: the deflate payload, the bytes it holds (where it decodes), and the trailer as written"""

    def __init__(self, body, data, isize=None, crc=None, pending=()):
        self.body, self.data, self.pending = bytes(body), bytes(data), list(pending)
        self.isize = len(self.data) if isize is None else isize
        self.crc = zlib.crc32(self.data) & 0xFFFFFFFF if crc is None else crc

    def block(self):
        return bgzf_wrap(self.body, self.crc, self.isize)


def P(blocks, tail=b"", **kw):
    body, data, pending = deflate(blocks, tail)
    return Payload(body, data, pending=pending, **kw)


def zlib_payload(data, level=6, strategy=zlib.Z_DEFAULT_STRATEGY):
    z = zlib.compressobj(level, zlib.DEFLATED, -15, 9, strategy)
    return Payload(z.compress(data) + z.flush(), data)


class Case:
    def __init__(self, name, payloads, bad=None, code=None):
        self.name, self.payloads, self.bad, self.code = name, payloads, bad, code
        self.file = b"".join(p.block() for p in payloads)
        self.data = b"".join(p.data for p in payloads) if bad is None else None


def rnd(n, seed):
    return bytes(np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8))


def lits(b):
    return [("lit", x) for x in b]


# ---------------------------------------------------------------------------------------------------------------- the valid cases
def _repeat_crossings():
    """three dynamic blocks whose code-length items run from the length alphabet into the distance alphabet: 16, 17, 18"""
    text = lits(b"abab")
    four = {97: 2, 98: 2, 256: 2, 257: 2}
    a = ("dynamic", text + [("copy", 3, 2)], dict(lit_lens=four, dist_lens={0: 2, 1: 2, 2: 2, 3: 2}, nlen=258, ndist=4,
                                                   items=[(18, 97), 2, 2, (18, 138), (18, 157 - 138), 2, (16, 5)]))
    b = ("dynamic", text + [("copy", 3, 4)], dict(lit_lens=four, dist_lens={2: 1, 3: 1}, nlen=260, ndist=4,
                                                   items=[(18, 97), 2, 2, (18, 138), (18, 157 - 138), 2, 2, (17, 4), 1, 1]))
    c = ("dynamic", text + [("copy", 3, 5)], dict(lit_lens=four, dist_lens={3: 1, 4: 1}, nlen=270, ndist=5,
                                                   items=[(18, 97), 2, 2, (18, 138), (18, 157 - 138), 2, 2, (18, 15), 1, 1]))
    return P([a, b, c])


def _stored_after_pending_bits():
    """a stored block behind a fixed block of k literals of 9 bits, k = 0..7: its header ends 1..7 bits into a byte, and on a byte's edge"""
    out = [P([("fixed", lits(bytes([200 + k] * k))), ("stored", b"stored-%d" % k), ("fixed", lits(b"!"))]) for k in range(8)]
    assert sorted(p.pending[0] for p in out) == list(range(8))
    return out


def valid_cases():
    big = rnd(32768, 7)
    chain_l = chain_lens([100, 101, 102, 103, 104, 105, 106, 107, 108, 109, 110, 256, 257, 258, 97, 259])      # 97 and 259 (length 5): 15 bits
    chain_d = chain_lens(list(range(16))[::-1][2:] + [15, 14])                                                   # distance symbols 15 and 14: 15 bits
    out = [
        Case("lengths 3 and 258", [P([("fixed", lits(b"abc") + [("copy", 3, 3), ("copy", 258, 1), ("copy", 258, 6)])])]),
        Case("distances 1 and 32768, 13 extra bits", [P([("stored", big), ("fixed", [("copy", 10, 32768), ("copy", 5, 1), ("copy", 4, 30000), ("copy", 7, 24577), ("copy", 9, 32768)])])]),
        Case("overlaps", [P([("fixed", lits(bytes(range(70))) + [("copy", 258, 1), ("copy", 100, 2), ("copy", 200, 63), ("copy", 200, 64), ("copy", 200, 65), ("copy", 66, 65),
                                                                   ("copy", 65, 64), ("copy", 64, 63), ("copy", 3, 2), ("copy", 257, 256)])])]),
        Case("codes of 15 bits", [P([("stored", rnd(300, 3)), ("dynamic", lits(b"adaaemn") + [("copy", 5, 129), ("copy", 3, 200), ("copy", 4, 1), ("copy", 5, 256)] + lits(b"a"),
                                                                 dict(lit_lens=chain_l, dist_lens=chain_d))])]),
        Case("a single distance code", [P([("dynamic", lits(b"xyz") + [("copy", 20, 1), ("lit", 65), ("copy", 3, 1)], dict(dist_lens={0: 1}))])]),
        Case("no distance code", [P([("dynamic", lits(b"only literals, no distance code at all"), dict(dist_lens={}))])]),
        Case("repeats across the alphabets", [_repeat_crossings()]),
        Case("HCLEN 5", [P([("dynamic", lits(b"\x01\x02hello\xff"), dict(lit_lens={s: 8 for s in range(1, 257)}, dist_lens={}, items=[0, 8] + [(16, 6)] * 42 + [(16, 3), 0], hclen=5,
                                                                         cl_lens={16: 1, 0: 2, 8: 2}))])]),
        Case("HCLEN 19", [P([("dynamic", lits(b"abcabc") + [("copy", 6, 3)], dict(hclen=19))])]),
        Case("an empty stored block between two others", [P([("fixed", lits(b"left")), ("stored", b""), ("fixed", lits(b"right") + [("copy", 4, 9)])])]),
        Case("a stored block after pending bits", _stored_after_pending_bits()),
        Case("three blocks of three types", [P([("stored", b"stored bytes "), ("fixed", lits(b"fixed ") + [("copy", 6, 6)]), ("dynamic", lits(b"dynamic") + [("copy", 12, 20)], {})])]),
        Case("ISIZE 0, 1 and 65536", [P([("fixed", [])]), P([("stored", b"")]), P([("fixed", lits(b"x"))]), P([("stored", b"y")]),
                                      P([("stored", rnd(30000, 5)), ("fixed", [("copy", 258, 30000)] * 137 + [("copy", 190, 100)])]), P([("fixed", lits(b"ab") + [("copy", 258, 2)] * 253 + [("copy", 257, 2), ("copy", 3, 2)])])]),
        Case("a copy and a literal end at ISIZE", [P([("fixed", lits(b"ab") + [("copy", 30, 2)])]), P([("fixed", lits(b"ab") + [("copy", 30, 2), ("lit", 99)])])]),
        Case("bytes behind the final block", [P([("fixed", lits(b"tail"))], tail=b"\xff\x00 not looked at"), P([("stored", b"s")], tail=b"\x07"), zlib_payload(b"z" * 500)]),
    ]
    assert len(out[12].payloads[4].data) == 65536 and len(out[12].payloads[5].data) == 65536
    return out


VALID = valid_cases()

# ---------------------------------------------------------------------------------------------------------------- the corrupt cases
GOOD = [P([("fixed", lits(b"good block ") + [("copy", 11, 11)])]), zlib_payload(b"another good block, and more of it, and more of it" * 3)]


def corrupt_payloads():
    """{code: a payload that is refused with it}"""
    whole = P([("fixed", lits(b"cut off in the middle of a literal"))])
    two = {97: 1, 256: 1}
    ok16 = P([("fixed", lits(b"0123456789abcdef"))])
    return {
        ij.BITS_RUN_OUT: Payload(whole.body[:9], b"", isize=whole.isize, crc=whole.crc),
        ij.RESERVED_TYPE: P([("fixed", lits(b"ab"), dict(final=0)), ("reserved", None)], isize=2),
        ij.STORED_LEN_DISAGREES: P([("stored", b"abcde", dict(nlen=0x1234))]),
        ij.STORED_PAST_BODY: P([("stored", b"abcde", dict(len=10))], isize=10),
        ij.BAD_CODE_LENGTH_SET: P([("dynamic", lits(b"a"), dict(lit_lens=two, dist_lens={}, items=[(16, 3)] + [0] * 255, check_items=False, cl_lens={0: 1, 16: 1}))], isize=1),
        ij.BAD_LITLEN_SET: P([("dynamic", lits(b"a"), dict(lit_lens={97: 2, 256: 2}, dist_lens={}))], isize=1),
        ij.BAD_DIST_SET: P([("dynamic", lits(b"a"), dict(lit_lens=two, dist_lens={0: 2}))], isize=1),
        ij.NO_END_OF_BLOCK: P([("dynamic", [], dict(lit_lens={}, dist_lens={}, nlen=257, ndist=1, items=[(18, 138), (18, 120)], cl_lens={18: 1, 0: 1}, hclen=4, eob=False))], isize=0),
        ij.LITLEN_SYMBOL: P([("fixed", lits(b"ab") + [("litsym", 286)])], isize=2),
        ij.DIST_SYMBOL: P([("fixed", lits(b"abcd") + [("litsym", 257), ("distsym", 30)])], isize=7),
        ij.DIST_PAST_START: P([("fixed", lits(b"a") + [("litsym", 257), ("distsym", 1)] + lits(b"b"))], isize=5),
        ij.OUTPUT_PAST_ISIZE: Payload(ok16.body, b"", isize=15, crc=ok16.crc),
        ij.OUTPUT_SHORT: Payload(ok16.body, b"", isize=17, crc=ok16.crc),
        ij.CRC_MISMATCH: Payload(ok16.body, ok16.data, crc=ok16.crc ^ 0x00100000),
        ij.UNUSED_CODE: P([("dynamic", lits(b"abc") + [("litsym", 257), ("bits", 0x7FFF, 15)], dict(lit_lens={97: 2, 98: 2, 99: 2, 256: 3, 257: 3}, dist_lens={}))], tail=b"\xff\xff", isize=6),
    }


CORRUPT_PAYLOADS = corrupt_payloads()
CORRUPT = [Case("code %d: %s" % (code, ij.CODE_NAMES[code]), [GOOD[code % 2]] * (1 + code % 3) + [p, GOOD[0]], bad=1 + code % 3, code=code)
           for code, p in sorted(CORRUPT_PAYLOADS.items())]
CORRUPT.append(Case("two bad blocks", [GOOD[0], GOOD[1], CORRUPT_PAYLOADS[ij.DIST_PAST_START], GOOD[0], CORRUPT_PAYLOADS[ij.RESERVED_TYPE]], bad=2, code=ij.DIST_PAST_START))
CORRUPT.append(Case("two bad blocks, a CRC first", [GOOD[0], CORRUPT_PAYLOADS[ij.CRC_MISMATCH], CORRUPT_PAYLOADS[ij.BITS_RUN_OUT]], bad=1, code=ij.CRC_MISMATCH))


def all_payloads():
    return [p for c in VALID for p in c.payloads] + [p for _, p in sorted(CORRUPT_PAYLOADS.items())] + GOOD


# ---------------------------------------------------------------------------------------------------------------- the mutations
N_MUTATIONS = 10_000
_STORED_ONLY = [P([("stored", rnd(n, n))]) for n in (1, 9, 60, 200)] + [P([("stored", rnd(40, 1)), ("stored", b""), ("stored", rnd(50, 2))])]


def mutation_base():
    """the payloads that are mutated: every case's of at most 400 bytes, and a few of stored blocks alone"""
    base = [p for p in all_payloads() if len(p.body) <= 400] + _STORED_ONLY
    return list({(p.body, p.isize): p for p in base}.values())


def mutate(rng, p):
    """(body, isize) of a mutation of p.  The mix keeps both verdicts in play: bytes appended behind the final block and flips
    inside the bytes of a stored block leave a payload valid, a cut, another ISIZE and flips anywhere mostly do not."""
    b = bytearray(p.body)
    isize = p.isize
    kind = int(rng.integers(0, 10))
    if kind == 0 and len(b) > 1:
        del b[int(rng.integers(1, len(b))):]                                             # cut off
    elif kind <= 2:
        b += rng.integers(0, 256, int(rng.integers(1, 6)), dtype=np.uint8).tobytes()     # bytes behind the end
    elif kind == 3:
        isize = max(0, min(65536, isize + int(rng.integers(-3, 4))))                     # the trailer says another length
    elif kind <= 5 and len(b) > 5 and b[0] & 6 == 0:
        for _ in range(int(rng.integers(1, 4))):                                         # flips behind a leading stored block's header
            b[int(rng.integers(5, len(b)))] ^= 1 << int(rng.integers(0, 8))
    else:
        for _ in range(int(rng.integers(1, 4))):
            if b:
                i = int(rng.integers(0, len(b)))
                b[i] = int(rng.integers(0, 256)) if rng.integers(0, 2) else b[i] ^ (1 << int(rng.integers(0, 8)))
    return bytes(b), isize


_MUTATIONS = {}


def mutations():
    """N_MUTATIONS seeded mutations, (body, isize) each, and the judge's Tally of each: made once a process"""
    if not _MUTATIONS:
        base = mutation_base()
        rng = np.random.default_rng(19510)
        muts = [mutate(rng, base[int(rng.integers(0, len(base)))]) for _ in range(N_MUTATIONS)]
        _MUTATIONS["m"] = muts, [ij.inflate(b, n) for b, n in muts]
    return _MUTATIONS["m"]
