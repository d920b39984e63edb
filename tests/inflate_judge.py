"""A plain-Python inflate, written from RFC 1951 alone: ints, lists and dicts, no zlib inside.  It is the judge of the device
BGZF inflater (csrc/afq_inflate.hip) and of its parser on the host (csrc/afq_inflate_elem.h through tests/inflate_elem_check.cpp):
the bytes, the tallies and, for a payload that is refused, the code that says why - the numbers of afq::InflateCode.

The stream is read bit by bit, a Huffman code is walked one bit at a time through a dict of (length, code), so nothing here
shares a trick with the code it judges.  Where the RFC leaves a verdict open, the verdict is zlib's (tests/test_inflate_judge_cpu.py
holds the judge against zlib.decompressobj(-15) on every case and on seeded mutations): an over-subscribed set of code lengths is
refused; an incomplete one too, unless it is a single code of length 1 or - for distances - no code at all; a block without an
end-of-block code is refused; bytes behind the final block are not looked at."""
import struct

(OK, BITS_RUN_OUT, RESERVED_TYPE, STORED_LEN_DISAGREES, STORED_PAST_BODY, BAD_CODE_LENGTH_SET, BAD_LITLEN_SET, BAD_DIST_SET, NO_END_OF_BLOCK,
 LITLEN_SYMBOL, DIST_SYMBOL, DIST_PAST_START, OUTPUT_PAST_ISIZE, OUTPUT_SHORT, CRC_MISMATCH, UNUSED_CODE, CODE_COUNT) = range(17)
CODE_NAMES = ["ok", "bits run out", "reserved block type", "stored length disagrees", "stored bytes past the body", "bad code-length set", "bad literal/length set",
              "bad distance set", "no end-of-block code", "literal/length symbol 286 or 287", "distance symbol 30 or 31", "distance in front of the block",
              "output past ISIZE", "output short of ISIZE", "CRC mismatch", "bits that are no code"]
# what afq_bgzf_inflate_device says in the brackets of "the deflate stream is corrupt or longer than ISIZE (...)"
WORDS = {BITS_RUN_OUT: "the bits run out", RESERVED_TYPE: "a block of the reserved type", STORED_LEN_DISAGREES: "a stored block's length is not its complement's",
         STORED_PAST_BODY: "a stored block runs past the payload", BAD_CODE_LENGTH_SET: "bad code lengths", BAD_LITLEN_SET: "a bad literal/length code",
         BAD_DIST_SET: "a bad distance code", NO_END_OF_BLOCK: "no end-of-block code", LITLEN_SYMBOL: "literal/length symbol 286 or 287",
         DIST_SYMBOL: "distance symbol 30 or 31", DIST_PAST_START: "a copy from in front of the block", OUTPUT_PAST_ISIZE: "more bytes than ISIZE",
         UNUSED_CODE: "bits that are no code of the set"}

CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LEN_EXTRA = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]
DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289, 16385, 24577]
DIST_EXTRA = [0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13]

_CRC_TABLE = []
for _i in range(256):
    _c = _i
    for _ in range(8):
        _c = (_c >> 1) ^ 0xEDB88320 if _c & 1 else _c >> 1
    _CRC_TABLE.append(_c)


def crc32(data):
    """gzip's CRC-32 (RFC 1952, section 8)"""
    c = 0xFFFFFFFF
    for b in data:
        c = _CRC_TABLE[(c ^ b) & 255] ^ (c >> 8)
    return c ^ 0xFFFFFFFF


class Refused(Exception):
    def __init__(self, code):
        Exception.__init__(self, CODE_NAMES[code])
        self.code = code


class Tally:
    """code: OK or why the payload is refused; data: the bytes (of a payload that decodes); the deflate blocks by type; literals and
    copies of the fixed and dynamic blocks; produced: the bytes the stream held when it ended or was refused"""

    def __init__(self):
        self.code, self.data, self.produced = OK, b"", 0
        self.n_stored = self.n_fixed = self.n_dynamic = self.n_literals = self.n_copies = 0


class _Bits:
    def __init__(self, body):
        self.body, self.at = body, 0   # at: the next bit's index

    def take(self, n):
        if self.at + n > 8 * len(self.body):
            raise Refused(BITS_RUN_OUT)
        v = 0
        for k in range(n):
            i = self.at + k
            v |= ((self.body[i >> 3] >> (i & 7)) & 1) << k
        self.at += n
        return v


def code_book(lens, refused, may_be_empty=False):
    """{(length, code): symbol} of the canonical code of RFC 1951 3.2.2; zlib's verdicts on the set"""
    count = [0] * 16
    for l in lens:
        count[l] += 1
    count[0] = 0
    left = 1
    for l in range(1, 16):
        left = 2 * left - count[l]
        if left < 0:
            raise Refused(refused)
    used = sum(count)
    if used == 0:
        if may_be_empty:
            return {}
        raise Refused(refused)
    if left > 0 and not (used == 1 and count[1] == 1):
        raise Refused(refused)
    code, next_code = 0, [0] * 16
    for l in range(1, 16):
        code = (code + count[l - 1]) << 1
        next_code[l] = code
    book = {}
    for s, l in enumerate(lens):
        if l:
            book[(l, next_code[l])] = s
            next_code[l] += 1
    return book


def _symbol(bits, book):
    code, body, at, end = 0, bits.body, bits.at, 8 * len(bits.body)
    for l in range(1, 16):
        if at >= end:
            raise Refused(BITS_RUN_OUT)
        code = code << 1 | ((body[at >> 3] >> (at & 7)) & 1)
        at += 1
        s = book.get((l, code))
        if s is not None:
            bits.at = at
            return s
    raise Refused(UNUSED_CODE)


FIXED_LITLEN = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
FIXED_DIST = [5] * 32


def _dynamic_books(bits):
    nlen, ndist, ncl = bits.take(5) + 257, bits.take(5) + 1, bits.take(4) + 4
    if nlen > 286:
        raise Refused(BAD_LITLEN_SET)
    if ndist > 30:
        raise Refused(BAD_DIST_SET)
    cl = [0] * 19
    for i in range(ncl):
        cl[CL_ORDER[i]] = bits.take(3)
    cl_book = code_book(cl, BAD_CODE_LENGTH_SET)
    if len(cl_book) < 2:
        raise Refused(BAD_CODE_LENGTH_SET)   # (an incomplete code-length code is refused even where it is a single code)
    lens = []
    while len(lens) < nlen + ndist:
        s = _symbol(bits, cl_book)
        if s < 16:
            lens.append(s)
            continue
        if s == 16:
            if not lens:
                raise Refused(BAD_CODE_LENGTH_SET)
            rep, val = 3 + bits.take(2), lens[-1]
        elif s == 17:
            rep, val = 3 + bits.take(3), 0
        else:
            rep, val = 11 + bits.take(7), 0
        if len(lens) + rep > nlen + ndist:
            raise Refused(BAD_CODE_LENGTH_SET)
        lens += [val] * rep
    if lens[256] == 0:
        raise Refused(NO_END_OF_BLOCK)
    return code_book(lens[:nlen], BAD_LITLEN_SET), code_book(lens[nlen:], BAD_DIST_SET, may_be_empty=True)


def inflate(body, isize, crc=None):
    """the payload of a BGZF block against its trailer -> Tally"""
    t = Tally()
    out = []
    bits = _Bits(body)
    try:
        while True:
            final, btype = bits.take(1), bits.take(2)
            if btype == 3:
                raise Refused(RESERVED_TYPE)
            if btype == 0:
                bits.at = (bits.at + 7) & ~7
                n, nn = bits.take(16), bits.take(16)
                if n != nn ^ 0xFFFF:
                    raise Refused(STORED_LEN_DISAGREES)
                at = bits.at >> 3
                if n > len(body) - at:
                    raise Refused(STORED_PAST_BODY)
                if n > isize - len(out):
                    raise Refused(OUTPUT_PAST_ISIZE)
                out += body[at:at + n]
                bits.at += 8 * n
                t.n_stored += 1
            else:
                if btype == 1:
                    litlen, dist = code_book(FIXED_LITLEN, BAD_LITLEN_SET), code_book(FIXED_DIST, BAD_DIST_SET)
                    t.n_fixed += 1
                else:
                    litlen, dist = _dynamic_books(bits)
                    t.n_dynamic += 1
                while True:
                    s = _symbol(bits, litlen)
                    if s < 256:
                        if len(out) >= isize:
                            raise Refused(OUTPUT_PAST_ISIZE)
                        out.append(s)
                        t.n_literals += 1
                    elif s == 256:
                        break
                    elif s >= 286:
                        raise Refused(LITLEN_SYMBOL)
                    else:
                        n = LEN_BASE[s - 257] + bits.take(LEN_EXTRA[s - 257])
                        d = _symbol(bits, dist)
                        if d >= 30:
                            raise Refused(DIST_SYMBOL)
                        d = DIST_BASE[d] + bits.take(DIST_EXTRA[d])
                        if d > len(out):
                            raise Refused(DIST_PAST_START)
                        if n > isize - len(out):
                            raise Refused(OUTPUT_PAST_ISIZE)
                        for _ in range(n):
                            out.append(out[-d])
                        t.n_copies += 1
            if final:
                break
        if len(out) != isize:
            raise Refused(OUTPUT_SHORT)
        t.data = bytes(out)
        if crc is not None and crc32(t.data) != crc:
            raise Refused(CRC_MISMATCH)
    except Refused as e:
        t.code, t.data = e.code, b""
    t.produced = len(out)
    return t


def blocks_of(data):
    """the BGZF blocks of a well-formed container: (payload, crc, isize) each"""
    out, p = [], 0
    while p < len(data):
        xlen = struct.unpack_from("<H", data, p + 10)[0]
        bsize, e = None, p + 12
        while e + 4 <= p + 12 + xlen:
            si, sl = data[e:e + 2], struct.unpack_from("<H", data, e + 2)[0]
            if si == b"BC" and sl == 2:
                bsize = struct.unpack_from("<H", data, e + 4)[0]
            e += 4 + sl
        end = p + bsize + 1
        crc, isize = struct.unpack_from("<II", data, end - 8)
        out.append((data[p + 12 + xlen:end - 8], crc, isize))
        p = end
    return out


def inflate_file(data):
    """a BGZF file -> (bytes, stats as afq_inflate_stats, None), or (None, None, (lowest bad block, its Tally))"""
    st = dict(n_in=len(data), n_out=0, n_blocks=0, n_blocks_empty=0, n_stored=0, n_fixed=0, n_dynamic=0, n_literals=0, n_copies=0)
    out = bytearray()
    for i, (body, crc, isize) in enumerate(blocks_of(data)):
        t = inflate(body, isize, crc)
        if t.code:
            return None, None, (i, t)
        out += t.data
        st["n_blocks"] += 1
        st["n_blocks_empty"] += isize == 0
        for k in ("n_stored", "n_fixed", "n_dynamic", "n_literals", "n_copies"):
            st[k] += getattr(t, k)
    st["n_out"] = len(out)
    return bytes(out), st, None
