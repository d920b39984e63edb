"""Snappy frame streams built from explicit element lists, for the decoders' tests: what a stream holds is what the list says, not
what some encoder chose.  An element is ("lit", bytes) or ("lit", bytes, form) - form 0 the inline length, 1..4 that many length
bytes - or ("copy", form, off, len) with form 1, 2 or 4 offset bytes.  VALID and CORRUPT are the cases; CHUNKS_ONLY are bodies that
no frame stream can carry (the plan takes a chunk's length from the body's own uvarint), for the element parser alone."""
from dataclasses import dataclass, field

import numpy as np

import snappy_judge as sj

# the codes of csrc/afq_snappy_elem.h
OK, LITERAL_PAST_BODY, OFFSET_ZERO, OFFSET_PAST_START, OUTPUT_PAST_ULEN, TAG_CUT_OFF, OUTPUT_SHORT, LENGTH_DISAGREES, CRC_MISMATCH = range(9)


def uvarint(n):
    out = bytearray()
    while n >= 0x80:
        out.append((n & 0x7F) | 0x80)
        n >>= 7
    out.append(n)
    return bytes(out)


def lit_forms(n):
    """the forms that can write a literal of n bytes"""
    return [f for f in (0, 1, 2, 3, 4) if (n <= 60 if f == 0 else n - 1 < 256 ** f)]


def enc_lit(data, form=None):
    n = len(data)
    assert n >= 1
    if form is None:
        form = lit_forms(n)[0]
    assert form in lit_forms(n), (n, form)
    if form == 0:
        return bytes([(n - 1) << 2]) + data
    return bytes([(59 + form) << 2]) + (n - 1).to_bytes(form, "little") + data


def enc_copy(form, off, n):
    if form == 1:
        assert 4 <= n <= 11 and 0 <= off < 2048
        return bytes([1 | ((n - 4) << 2) | ((off >> 8) << 5), off & 0xFF])
    assert form in (2, 4) and 1 <= n <= 64 and 0 <= off < 256 ** form
    return bytes([((n - 1) << 2) | (2 if form == 2 else 3)]) + off.to_bytes(form, "little")


def block(elems, declared=None):
    """(raw block, the bytes it stands for).  Elements that cannot be carried out (offset 0, offset past the start) produce nothing:
    such a block is for the corrupt cases, which give `declared` themselves."""
    body, out = bytearray(), bytearray()
    for e in elems:
        if e[0] == "lit":
            body += enc_lit(e[1], e[2] if len(e) > 2 else None)
            out += e[1]
        elif e[0] == "raw":   # bytes of the block as they are, producing nothing
            body += e[1]
        else:
            _, form, off, n = e
            body += enc_copy(form, off, n)
            if 0 < off <= len(out):
                for _ in range(n):
                    out.append(out[-off])
    return uvarint(len(out) if declared is None else declared) + bytes(body), bytes(out)


def frame(t, body):
    return bytes([t]) + len(body).to_bytes(3, "little") + body


@dataclass
class DataChunk:
    compressed: bool
    body: bytes          # the raw block, or the stored bytes
    data: bytes          # what the CRC is taken of (a corrupt case may lie)
    crc_xor: int = 0
    ulen: int = -1       # what a plan would say: the body's uvarint, or the stored length (CHUNKS_ONLY overrides it)

    def frame(self):
        crc = sj.mask_crc(sj.crc32c(self.data)) ^ self.crc_xor
        return frame(0 if self.compressed else 1, crc.to_bytes(4, "little") + self.body)

    def planned_ulen(self):
        if self.ulen >= 0:
            return self.ulen
        return sj._uvarint(self.body, 0)[0] if self.compressed else len(self.body)


def compressed(elems, declared=None, data=None, **kw):
    body, out = block(elems, declared)
    return DataChunk(True, body, out if data is None else data, **kw)


def stored(data, **kw):
    return DataChunk(False, bytes(data), bytes(data), **kw)


@dataclass
class Case:
    name: str
    parts: list                      # DataChunk, or bytes that go into the stream as they are (identifier, skippable chunks)
    bad: int = -1                    # corrupt: the index of the lowest data chunk that must be refused ...
    code: int = OK                   # ... and why
    chunks: list = field(init=False)
    stream: bytes = field(init=False)
    data: bytes = field(init=False)

    def __post_init__(self):
        self.chunks = [p for p in self.parts if isinstance(p, DataChunk)]
        self.stream = sj.STREAM_ID + b"".join(p.frame() if isinstance(p, DataChunk) else p for p in self.parts)
        self.data = b"".join(c.data for c in self.chunks) if self.bad < 0 else b""


def rnd(n, seed):
    return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8).tobytes()


def run_elems(n, seed, period=37):
    """elements for n > 0 bytes: a literal of min(n, period) random bytes, then copies from `period` back, 64 at a time"""
    first = min(n, period)
    el = [("lit", rnd(first, seed))]
    n -= first
    while n:
        k = min(n, 64)
        el.append(("copy", 2, period, k))
        n -= k
    return el


def _valid():
    cases = []
    # every literal length form at 1, 60, 61, 256, 257, 65 536
    for n in (1, 60, 61, 256, 257, 65536):
        for f in lit_forms(n):
            cases.append(Case(f"literal {n} form {f}", [compressed([("lit", rnd(n, n + f), f)])]))
    # copy form 1 at len 4 and 11, off 1 and 2047
    for n in (4, 11):
        for off in (1, 2047):
            cases.append(Case(f"copy1 len {n} off {off}", [compressed([("lit", rnd(2047, off)), ("copy", 1, off, n)])]))
    # copy form 2 at len 1 and 64, off 1 and 65 535 (64 bytes from 65 535 back would end behind a chunk's 65 536: not a case)
    for n, off in ((1, 1), (64, 1), (1, 65535)):
        cases.append(Case(f"copy2 len {n} off {off}", [compressed([("lit", rnd(max(off, 3), n + off)), ("copy", 2, off, n)])]))
    cases.append(Case("copy4 in range", [compressed([("lit", rnd(40000, 4)), ("copy", 4, 39999, 64), ("copy", 4, 1, 3)])]))
    for off in (1, 2, 3, 4, 7, 63, 64, 65):
        for n in (64, 5):
            cases.append(Case(f"copy off {off} len {n}", [compressed([("lit", rnd(70, off + n)), ("copy", 2, off, n), ("lit", b"z")])]))
    cases.append(Case("off == len", [compressed([("lit", rnd(9, 1)), ("copy", 2, 9, 9), ("copy", 1, 5, 5)])]))
    cases.append(Case("off == w", [compressed([("lit", rnd(50, 2)), ("copy", 2, 50, 64), ("copy", 2, 114, 20)])]))
    # chunk lengths, stored and compressed
    for n in (0, 1, 63, 64, 65, 4095, 4096, 65535, 65536):
        cases.append(Case(f"stored {n}", [stored(rnd(n, n))]))
        cases.append(Case(f"compressed {n}", [compressed(run_elems(n, n) if n else [])]))
    # a body longer than its output, and longer than any window of it: one-byte literals in the longest form
    cases.append(Case("body longer than output", [compressed([("lit", bytes([i & 0xFF]), 4) for i in range(3000)])]))
    cases.append(Case("elements across many windows", [compressed([e for i in range(600) for e in (("lit", rnd(61 + i % 5, i), 2 + i % 3), ("copy", 2, 1 + i % 61, 1 + i % 64))])]))
    # chunks cut at 60 000, and at 4097: out_off walks through every residue of 16
    d = rnd(3 * 60000 + 123, 60)
    cases.append(Case("cut at 60000", [(stored if k & 1 else (lambda x: compressed([("lit", x)])))(d[a:a + 60000]) for k, a in enumerate(range(0, len(d), 60000))]))
    cases.append(Case("cut at 4097", [compressed(run_elems(4097, k, 24 + k)) if k % 3 else stored(rnd(4097, k)) for k in range(17)]))
    skip = frame(0x80, b"skip me") + frame(0xFE, b"\0" * 13) + frame(0xFD, b"")
    cases.append(Case("skippable and padding", [compressed(run_elems(500, 1)), skip, stored(b"xyz"), frame(0xFE, b""), compressed(run_elems(70, 2)), skip]))
    cases.append(Case("second identifier", [compressed(run_elems(300, 3)), sj.STREAM_ID, stored(rnd(100, 4)), sj.STREAM_ID]))
    cases.append(Case("identifier alone", []))
    cases.append(Case("300 small chunks", [compressed(run_elems(1 + k % 90, k, 1 + k % 11)) if k % 4 else stored(rnd(k % 7, k)) for k in range(300)]))
    return cases


def _good(k):
    return compressed(run_elems(200 + k, k))


def _corrupt():
    L = ("lit", b"abcdefgh")
    bad = {
        "offset 0": (compressed([L, ("copy", 2, 0, 4)], declared=12), OFFSET_ZERO),
        "offset beyond the bytes produced": (compressed([L, ("copy", 2, 9, 4)], declared=12), OFFSET_PAST_START),
        "offset beyond, four bytes": (compressed([L, ("copy", 4, 0x80000000, 4)], declared=12), OFFSET_PAST_START),
        "literal past the body": (compressed([L, ("raw", bytes([9 << 2]) + b"123456789")], declared=18), LITERAL_PAST_BODY),
        "long literal past the body": (compressed([L, ("raw", bytes([63 << 2]) + b"\xff\xff\xff\xff" + b"xy")], declared=65536), LITERAL_PAST_BODY),
        "literal length cut off": (compressed([L, ("raw", bytes([62 << 2]) + b"\x01\x00")], declared=10), TAG_CUT_OFF),
        "copy offset cut off": (compressed([L, ("raw", bytes([(3 << 2) | 2, 4]))], declared=12), TAG_CUT_OFF),
        "copy4 offset cut off": (compressed([L, ("raw", bytes([(3 << 2) | 3, 4, 0, 0]))], declared=12), TAG_CUT_OFF),
        "output past ulen, a copy": (compressed([L, ("copy", 2, 8, 5)], declared=12), OUTPUT_PAST_ULEN),
        "output past ulen, a literal": (compressed([L, L], declared=15), OUTPUT_PAST_ULEN),
        "an element behind the last byte": (compressed([L, ("lit", b"e")], declared=8), OUTPUT_PAST_ULEN),
        "output short of ulen": (compressed([L, ("copy", 2, 8, 3)], declared=12), OUTPUT_SHORT),
        "a length and nothing else": (compressed([], declared=5), OUTPUT_SHORT),
        "stored payload bit": (DataChunk(False, b"stored byter", b"stored bytes"), CRC_MISMATCH),
        "CRC bit": (compressed(run_elems(4000, 9), crc_xor=1 << 17), CRC_MISMATCH),
        "CRC bit, stored": (stored(rnd(70000 - 65536 + 1, 9), crc_xor=1), CRC_MISMATCH),
    }
    cases = [Case(name, [_good(0), stored(b"in front"), c, _good(1)], bad=2, code=code) for name, (c, code) in bad.items()]
    first, second = bad["CRC bit"][0], bad["offset 0"][0]
    cases.append(Case("two bad chunks", [_good(0)] * 5 + [first] + [_good(1)] * 40 + [second, _good(2)], bad=5, code=CRC_MISMATCH))
    cases.append(Case("two bad chunks, the other order", [_good(0)] * 3 + [second] + [_good(1)] * 40 + [first, _good(2)], bad=3, code=OFFSET_ZERO))
    return cases


VALID = _valid()
CORRUPT = _corrupt()
# (chunk, code): bodies whose own uvarint is not what the plan says - malformed, or another number
CHUNKS_ONLY = [
    (compressed([("lit", b"abcdefgh")], declared=9, ulen=8), LENGTH_DISAGREES),
    (compressed([("lit", b"abcdefgh")], declared=7, ulen=8), LENGTH_DISAGREES),
    (DataChunk(True, b"\x88\x80\x80\x80\x80\x00" + enc_lit(b"abcdefgh"), b"abcdefgh", ulen=8), LENGTH_DISAGREES),   # six bytes of uvarint
    (DataChunk(True, b"\x88\x80", b"", ulen=8), LENGTH_DISAGREES),                                                    # cut off
    (DataChunk(True, b"", b"", ulen=0), LENGTH_DISAGREES),
]


def judge_chunk(c):
    """(True, crc32c of the bytes) where the judge decodes chunk c to its planned length, else (False, None).  The CRC is the plain
    one of the decoded bytes, not compared with anything: the frame's checksum is the frame reader's business."""
    ulen = c.planned_ulen()
    if not c.compressed:
        return (True, sj.crc32c(c.body)) if len(c.body) == ulen else (False, None)
    try:
        want, _ = sj._uvarint(c.body, 0)
        if want != ulen:
            return False, None
        return True, sj.crc32c(sj.raw_decode(c.body))
    except sj.SnappyJudgeError:
        return False, None


# ------------------------------------------------------------------------------------------------ output at and across byte 2^32
# A stream whose decoded bytes cross byte 2^32 (tests/test_gpu_snappy_decode.py decodes it, tests/test_snappy_far_stream_cpu.py
# holds its plan): a first chunk, a LOW GROUP of small mixed chunks, some 65 535 chunks of 65 536 zero bytes (one frame, repeated),
# a shorter chunk of zeros that brings the output to where the FAR GROUP must begin, and the far group - forty small mixed chunks,
# one of them (the STRADDLER, larger) begins `before` bytes in front of byte 2^32.  The far chunks behind the straddler are the
# low group's twins: low chunk j lies exactly 2^32 below far chunk j + 1 behind the straddler, has its length and other bytes, and
# the first chunk (random bytes) lies 2^32 below the straddler's bytes from byte 2^32 on.  A decoder that drops the high half of an
# out_off therefore writes over the low group, and what is read back of [0, 2^21) differs from what the stream says.
FAR = 1 << 32
FAR_LOW, FAR_GROUP, FAR_STRADDLER = 10, 40, 5   # chunks of the low group, of the far group, the straddler's place in the far group
FAR_STREAMS = {   # name: (the straddler of a seed, its elements' output lengths as (kind, n), `before`)
    "in a literal": (lambda seed: compressed([("lit", rnd(4097, seed))]), [("lit", 4097)], 1003),
    "in a copy": (lambda seed: compressed(run_elems(4097, seed, 29)), [("lit", 29)] + [("copy", 64)] * 63 + [("copy", 36)], 2048),
    "start on": (lambda seed: stored(rnd(4097, seed)), [("stored", 4097)], 0),
}


def mixed_kinds(seed=0):
    """forty compressed chunks of run elements (1 .. 40 bytes, periods 1 .. 5) and five stored ones (0 .. 4 bytes)"""
    return [compressed(run_elems(1 + k, seed + k, 1 + k % 5)) for k in range(40)] + [stored(rnd(k, seed + k)) for k in range(5)]


def zeros_chunk(n):
    """n >= 1 zero bytes: one literal of a byte, then copies from 1 back, 64 at a time"""
    return compressed([("lit", b"\0")] + [("copy", 2, 1, min(64, n - 1 - a)) for a in range(0, n - 1, 64)])


class FarStream:
    """runs: [(group, DataChunk, count)] in stream order; first[r] / out_off[r]: the index and output offset of run r's first chunk"""

    def __init__(self, name):
        make, self.straddler_elems, self.before = FAR_STREAMS[name]
        self.name = name
        far_kinds, low_kinds = mixed_kinds(0), mixed_kinds(1000)
        far = [far_kinds[(7 * j) % len(far_kinds)] for j in range(FAR_GROUP)]
        far[FAR_STRADDLER] = make(77)
        low = [low_kinds[(7 * j) % len(low_kinds)] for j in range(FAR_STRADDLER + 1, FAR_STRADDLER + 1 + FAR_LOW)]
        first = stored(rnd(len(far[FAR_STRADDLER].data) - self.before, 78))
        self.filler = zeros_chunk(65536)
        front = len(first.data) + sum(len(c.data) for c in low)
        gap = FAR - self.before - sum(len(c.data) for c in far[:FAR_STRADDLER]) - front
        self.n_fillers, short = divmod(gap, 65536)
        self.runs = [("first", first, 1)] + [("low", c, 1) for c in low] + [("filler", self.filler, self.n_fillers)]
        self.runs += [("short filler", zeros_chunk(short), 1)] if short else []
        self.runs += [("far", c, 1) for c in far]
        self.first, self.out_off, i, o = [], [], 0, 0
        for _, c, count in self.runs:
            self.first.append(i), self.out_off.append(o)
            i, o = i + count, o + count * len(c.data)
        self.n_chunks, self.total = i, o

    def stream(self, crc_flip=None):
        """the stream's bytes; crc_flip = (chunk index, bit): that chunk's CRC with the bit flipped"""
        parts = [sj.STREAM_ID]
        for (_, c, count), i in zip(self.runs, self.first):
            if crc_flip is not None and crc_flip[0] == i:
                assert count == 1
                c = DataChunk(c.compressed, c.body, c.data, crc_xor=1 << crc_flip[1])
            parts.append(c.frame() * count)
        return b"".join(parts)

    def group(self, name):
        """[(chunk index, out_off, chunk)] of the single chunks of a group"""
        return [(i, o, c) for (g, c, count), i, o in zip(self.runs, self.first, self.out_off) if g == name and count == 1]

    def straddler(self):
        return self.group("far")[FAR_STRADDLER]

    def elem_at(self, byte):
        """(kind, first output byte, length) of the straddler's element that produces output byte `byte` of the straddler"""
        at = 0
        for kind, n in self.straddler_elems:
            if at <= byte < at + n:
                return kind, at, n
            at += n
        raise ValueError(byte)

    def window(self, a, b, truncated=False):
        """bytes [a, b) of the output as the stream says them, zeros behind `total`.  truncated: as a decoder leaves them that writes
        every chunk, in stream order, at out_off mod 2^32 (the model of a dropped high half; a window of it is sparse, like this one)."""
        out = bytearray(b - a)
        for (_, c, count), o in zip(self.runs, self.out_off):
            u = len(c.data)
            if not u:
                continue
            if count > 1:   # the fillers end below 2^32, truncated or not: only those that touch the window are visited
                assert o + count * u <= FAR
                starts = [o + k * u for k in range(max(0, (a - o) // u), min(count, -(-(b - o) // u)))]
            else:
                starts = [o % FAR if truncated else o]
            for s in starts:
                x, y = max(a, s), min(b, s + u)
                if x < y:
                    out[x - a:y - a] = c.data[x - s:y - s]
        return bytes(out)

    def tallies(self):
        """n_blocks, n_blocks_stored, n_literal_bytes, n_copies: the judge's tallies of each distinct chunk times how often it occurs"""
        t, seen = dict(n_blocks=0, n_blocks_stored=0, n_literal_bytes=0, n_copies=0), {}
        for _, c, count in self.runs:
            if id(c) not in seen:
                s = sj.decode(sj.STREAM_ID + c.frame())
                assert s.data == c.data and s.n_chunks == 1
                seen[id(c)] = s
            s = seen[id(c)]
            t["n_blocks"] += count
            t["n_blocks_stored"] += count * s.n_stored
            t["n_literal_bytes"] += count * s.literal_bytes
            t["n_copies"] += count * s.copies
        return t
