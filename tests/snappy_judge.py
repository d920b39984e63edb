"""A snappy frame-stream reader written from the format descriptions alone (snappy's format_description.txt and
framing_format.txt): plain Python, no share in the library's decoder or its encoder.  It accepts what the descriptions allow the
library's streams to hold and refuses the rest, and it tallies what a stream is made of, to hold against afq_snappy_stats."""
from dataclasses import dataclass, field

STREAM_ID = b"\xff\x06\x00\x00sNaPpY"
MAX_CHUNK = 65536


class SnappyJudgeError(ValueError):
    pass


def _crc_table():
    t = []
    for i in range(256):
        c = i
        for _ in range(8):
            c = (c >> 1) ^ 0x82F63B78 if c & 1 else c >> 1
        t.append(c)
    return t


_T = _crc_table()


def crc32c(data) -> int:
    c = 0xFFFFFFFF
    for b in bytes(data):
        c = _T[(c ^ b) & 0xFF] ^ (c >> 8)
    return c ^ 0xFFFFFFFF


def mask_crc(c: int) -> int:
    return (((c >> 15) | (c << 17)) + 0xA282EAD8) & 0xFFFFFFFF


def _uvarint(b, p):
    v, s = 0, 0
    while True:
        if p >= len(b):
            raise SnappyJudgeError("raw block: truncated length")
        x = b[p]
        p += 1
        v |= (x & 0x7F) << s
        if not x & 0x80:
            return v, p
        s += 7
        if s > 32:
            raise SnappyJudgeError("raw block: length varint too long")


def raw_decode(block, tally=None) -> bytes:
    """One raw snappy block -> its bytes.  Refuses an offset of 0, an offset beyond the bytes produced so far, a produced length
    other than the declared one and bytes behind the last element.  tally: a dict whose "literal_bytes" and "copies" are added to."""
    b = bytes(block)
    want, p = _uvarint(b, 0)
    out = bytearray()
    lit = copies = 0
    while p < len(b):
        if len(out) >= want:
            raise SnappyJudgeError("raw block: trailing bytes behind the declared length")
        tag = b[p]
        p += 1
        kind = tag & 3
        if kind == 0:
            n = tag >> 2
            if n >= 60:
                k = n - 59
                if p + k > len(b):
                    raise SnappyJudgeError("raw block: truncated literal length")
                n = int.from_bytes(b[p:p + k], "little")
                p += k
            n += 1
            if p + n > len(b):
                raise SnappyJudgeError("raw block: truncated literal")
            out += b[p:p + n]
            p += n
            lit += n
            continue
        if kind == 1:
            if p + 1 > len(b):
                raise SnappyJudgeError("raw block: truncated copy")
            n = 4 + ((tag >> 2) & 7)
            off = ((tag >> 5) << 8) | b[p]
            p += 1
        elif kind == 2:
            if p + 2 > len(b):
                raise SnappyJudgeError("raw block: truncated copy")
            n = 1 + (tag >> 2)
            off = int.from_bytes(b[p:p + 2], "little")
            p += 2
        else:
            if p + 4 > len(b):
                raise SnappyJudgeError("raw block: truncated copy")
            n = 1 + (tag >> 2)
            off = int.from_bytes(b[p:p + 4], "little")
            p += 4
        if off == 0:
            raise SnappyJudgeError("raw block: copy offset 0")
        if off > len(out):
            raise SnappyJudgeError("raw block: copy offset beyond the bytes produced so far")
        copies += 1
        if off >= n:
            out += out[len(out) - off:len(out) - off + n]
        else:
            for _ in range(n):
                out.append(out[-off])
    if len(out) != want:
        raise SnappyJudgeError(f"raw block: {len(out)} bytes produced, {want} declared")
    if tally is not None:
        tally["literal_bytes"] = tally.get("literal_bytes", 0) + lit
        tally["copies"] = tally.get("copies", 0) + copies
    return bytes(out)


@dataclass
class Chunk:
    type: int          # 0x00 compressed, 0x01 stored
    body: bytes        # the raw block, or the bytes themselves
    data: bytes        # the uncompressed bytes


@dataclass
class Stream:
    data: bytes = b""
    chunks: list = field(default_factory=list)
    n_chunks: int = 0
    n_stored: int = 0
    literal_bytes: int = 0
    copies: int = 0
    n_identifiers: int = 0


def parse_frames(stream):
    """(type, body) of every frame chunk.  The first chunk must be the stream identifier; types 0x02..0x7f are refused."""
    b = bytes(stream)
    p, first, out = 0, True, []
    while p < len(b):
        if p + 4 > len(b):
            raise SnappyJudgeError("frame: truncated chunk header")
        t = b[p]
        n = int.from_bytes(b[p + 1:p + 4], "little")
        p += 4
        if p + n > len(b):
            raise SnappyJudgeError("frame: truncated chunk")
        if first and t != 0xFF:
            raise SnappyJudgeError("frame: the first chunk is not the stream identifier")
        first = False
        if t == 0xFF and b[p - 4:p + n] != STREAM_ID:
            raise SnappyJudgeError("frame: bad stream identifier")
        if 0x02 <= t <= 0x7F:
            raise SnappyJudgeError(f"frame: reserved unskippable chunk type {t:#x}")
        out.append((t, b[p:p + n]))
        p += n
    if first:
        raise SnappyJudgeError("frame: the first chunk is not the stream identifier")
    return out


def decode(stream, keep_chunks: bool = False) -> Stream:
    """The whole stream: identifier, 0x00 and 0x01 data chunks, padding (0xfe) and skippable (0x80..0xfd) chunks; every data chunk's
    masked CRC-32C is checked against its uncompressed bytes, and more than 65536 of those are refused."""
    s = Stream()
    parts = []
    tally = {}
    for t, body in parse_frames(stream):
        if t == 0xFF:
            s.n_identifiers += 1
            continue
        if t >= 0x80:
            continue   # padding and skippable chunks
        if len(body) < 4:
            raise SnappyJudgeError("frame: data chunk shorter than its checksum")
        crc = int.from_bytes(body[:4], "little")
        if t == 0x00:
            want, _ = _uvarint(body, 4)
            if want > MAX_CHUNK:
                raise SnappyJudgeError("frame: a chunk of more than 65536 uncompressed bytes")
            data = raw_decode(body[4:], tally)
        else:
            data = body[4:]
            if len(data) > MAX_CHUNK:
                raise SnappyJudgeError("frame: a chunk of more than 65536 uncompressed bytes")
            s.n_stored += 1
        if mask_crc(crc32c(data)) != crc:
            raise SnappyJudgeError("frame: checksum mismatch")
        s.n_chunks += 1
        parts.append(data)
        if keep_chunks:
            s.chunks.append(Chunk(t, body[4:], data))
    s.data = b"".join(parts)
    s.literal_bytes, s.copies = tally.get("literal_bytes", 0), tally.get("copies", 0)
    return s
