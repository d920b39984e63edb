// afq_inflate_elem.h — the parser of a raw deflate stream (RFC 1951) of at most 65536 bytes of output, the payload of a BGZF
// block, for the host and the device alike (k_bgzf_inflate of afq_inflate.hip; tests/inflate_elem_check.cpp runs it under the host
// sanitizers).  One call of inflate_next looks at what comes next in the stream and either hands out what may be moved - a
// literal byte, a copy (len, dist), a run of stored bytes and where they start in the body - or the stream's end, or a code.
// Every check stands in front of what it guards: the bit reader fetches a byte of the body only below in_len; a copy is handed
// out only with 1 <= dist <= produced and len <= isize - produced, a literal only with produced < isize, a stored run only
// with all of it inside the body and inside the output; the decode tables are built only from code lengths that zlib's
// inflate_table would take (an over-subscribed set is refused, an incomplete one too unless it is a single code of length 1 or
// no distance code at all), and a lookup stays inside them whatever bits it is given.  A loop that moves only what it is handed
// cannot leave the body, the output or the tables, whatever the body holds.
//
// The body is read through a source `src`: src.byte(i) for i < in_len, src.le32(i) for i + 4 <= in_len (the four bytes at i,
// little endian), so that the device can serve it from a staged window.
#pragma once
#include <cstdint>

#ifndef AFQ_HD
#if defined(__HIPCC__) || defined(__CUDACC__)
#define AFQ_HD __host__ __device__ __forceinline__
#else
#define AFQ_HD inline
#endif
#endif
// on the device every lane of the wave parses the same stream: what comes out of a table is made wave-uniform, so that the
// parser's state stays in scalar registers
#if defined(__HIP_DEVICE_COMPILE__)
#define AFQ_INFLATE_UNI(v) ((uint32_t)__builtin_amdgcn_readfirstlane((int)(v)))
#else
#define AFQ_INFLATE_UNI(v) ((uint32_t)(v))
#endif

namespace afq {

// what is wrong with a block (the low byte of the decoder's status word, the block's index above it)
enum InflateCode : uint32_t {
    kInflateOk = 0,
    kInflateBitsRunOut = 1,           // the body ends inside a header, a code or its extra bits
    kInflateReservedType = 2,         // BTYPE 3
    kInflateStoredLenDisagrees = 3,   // a stored block's LEN is not the complement of its NLEN
    kInflateStoredPastBody = 4,       // a stored block's bytes do not all lie inside the body
    kInflateBadCodeLengthSet = 5,     // the code-length code is over-subscribed or incomplete; repeat 16 with nothing before it; a repeat past HLIT + HDIST
    kInflateBadLitLenSet = 6,         // more than 286 literal/length symbols; their code is over-subscribed or incomplete
    kInflateBadDistSet = 7,           // more than 30 distance symbols; their code is over-subscribed or incomplete
    kInflateNoEndOfBlock = 8,         // symbol 256 has no code
    kInflateLitLenSymbol = 9,         // literal/length symbol 286 or 287 (a fixed block can spell them)
    kInflateDistSymbol = 10,          // distance symbol 30 or 31
    kInflateDistPastStart = 11,       // a copy from in front of the block
    kInflateOutputPastIsize = 12,     // a literal, copy or stored run would produce bytes behind ISIZE
    kInflateOutputShort = 13,         // the final block ends with fewer bytes produced than ISIZE
    kInflateCrcMismatch = 14,         // the bytes decode; their CRC-32 is not the trailer's
    kInflateUnusedCode = 15,          // bits that spell no code of an incomplete set (a single code of length 1, no distance code)
    kInflateCodeCount
};

constexpr uint32_t kInflateMaxOut = 65536;     // ISIZE of a BGZF block at the most
constexpr uint32_t kInflateFastBits = 10;      // the first-level lookup; longer codes walk the canonical code bit by bit
constexpr uint32_t kInflateClFastBits = 7;     // the code-length code: every code fits
constexpr uint32_t kInflateMaxLitLen = 288, kInflateMaxDist = 32, kInflateMaxBits = 15;

// a canonical Huffman code ready to be read: fast[next bits] = symbol << 4 | length for codes of at most fast_bits bits (0: none),
// and for all codes count[length] and the symbols sorted by (length, symbol)
struct InflateTables {
    uint16_t lit_fast[1u << kInflateFastBits], dist_fast[1u << kInflateFastBits];   // (dist_fast holds the code-length code while a dynamic header is read)
    uint16_t lit_count[16], dist_count[16], cl_count[16];
    uint16_t lit_sorted[kInflateMaxLitLen], dist_sorted[kInflateMaxDist], cl_sorted[20];
    uint16_t work[32];   // a build's: where a length's symbols go next, its next code
    uint8_t lens[kInflateMaxLitLen + kInflateMaxDist], cl_lens[20];
};

struct InflateBits { uint64_t buf; uint32_t cnt, pos; };   // cnt bits wait in buf (above them: zero), body[pos] is the next byte to fetch

struct InflateState {
    InflateBits b;
    uint32_t in_len, isize, produced;
    uint32_t in_block, final_seen;                             // inside a fixed or dynamic block; BFINAL was set on the block read last
    uint32_t n_stored, n_fixed, n_dynamic, n_literals, n_copies;   // deflate blocks by type; literals and copies of fixed and dynamic blocks
};

enum InflateKind : uint32_t { kInflateLiteral = 0, kInflateCopy = 1, kInflateStoredRun = 2, kInflateEnd = 3 };
struct InflateStep {
    uint32_t code;   // kInflateOk, or why nothing may move
    uint32_t kind;
    uint32_t lit;    // literal: the byte
    uint32_t len;    // copy: 3..258; stored run: 1..65535 - bytes produced
    uint32_t dist;   // copy: 1..produced back
    uint32_t src;    // stored run: its first byte's index in the body
};

AFQ_HD void inflate_begin(InflateState& S, uint32_t in_len, uint32_t isize) {
    S.b.buf = 0; S.b.cnt = 0; S.b.pos = 0;
    S.in_len = in_len; S.isize = isize; S.produced = 0; S.in_block = 0; S.final_seen = 0;
    S.n_stored = S.n_fixed = S.n_dynamic = S.n_literals = S.n_copies = 0;
}

// at least 32 bits wait behind this, or all that the body still has
template <class Src>
AFQ_HD void inflate_fill(Src& src, InflateBits& b, uint32_t in_len) {
    if (b.cnt > 32) return;
    if (in_len - b.pos >= 4) {   // (pos <= in_len)
        b.buf |= (uint64_t)src.le32(b.pos) << b.cnt;
        b.pos += 4; b.cnt += 32;
        return;
    }
    while (b.pos < in_len) {   // at most 3 bytes
        b.buf |= (uint64_t)src.byte(b.pos) << b.cnt;
        b.pos += 1; b.cnt += 8;
    }
}
// n <= 32 bits behind a fill; false: the body has fewer
AFQ_HD bool inflate_take(InflateBits& b, uint32_t n, uint32_t& v) {
    if (n > b.cnt) return false;
    v = (uint32_t)(b.buf & ((1ull << n) - 1));
    b.buf >>= n; b.cnt -= n;
    return true;
}

// The tables of n <= 288 code lengths (each <= 15).  0: built; 1: over-subscribed; 2: incomplete - `single`: it is one code of
// length 1, and the tables are built; 3: no code at all (nothing is built but the zeroed fast table and counts).
AFQ_HD uint32_t inflate_build(const uint8_t* lens, uint32_t n, uint16_t* fast, uint32_t fast_bits, uint16_t* count, uint16_t* sorted, uint16_t* work, bool& single) {
    single = false;
    for (uint32_t l = 0; l <= kInflateMaxBits; ++l) count[l] = 0;
    for (uint32_t s = 0; s < n; ++s) {
        const uint32_t l = AFQ_INFLATE_UNI(lens[s]) & 15u;
        count[l] = (uint16_t)(AFQ_INFLATE_UNI(count[l]) + 1);
    }
    for (uint32_t i = 0; i < (1u << fast_bits); ++i) fast[i] = 0;
    uint16_t *offs = work, *next = work + 16;   // (a code of l bits is below 2^l)
    int32_t left = 1;
    uint32_t code = 0, used = 0;
    for (uint32_t l = 1; l <= kInflateMaxBits; ++l) {
        const uint32_t c = AFQ_INFLATE_UNI(count[l]);
        left = left * 2 - (int32_t)c;
        if (left < 0) return 1;
        offs[l] = (uint16_t)used; next[l] = (uint16_t)code;
        used += c;
        code = (code + c) << 1;
    }
    if (used == 0) return 3;
    single = used == 1 && AFQ_INFLATE_UNI(count[1]) == 1;
    if (left > 0 && !single) return 2;
    for (uint32_t s = 0; s < n; ++s) {
        const uint32_t l = AFQ_INFLATE_UNI(lens[s]) & 15u;
        if (!l) continue;
        const uint32_t at = AFQ_INFLATE_UNI(offs[l]), c = AFQ_INFLATE_UNI(next[l]);
        offs[l] = (uint16_t)(at + 1); next[l] = (uint16_t)(c + 1);
        sorted[at] = (uint16_t)s;   // (at < used <= n)
        if (l > fast_bits) continue;
        uint32_t r = 0;   // the code as the stream spells it: its first bit lowest
        for (uint32_t k = 0; k < l; ++k) r |= ((c >> k) & 1u) << (l - 1 - k);
        for (uint32_t i = r; i < (1u << fast_bits); i += 1u << l) fast[i] = (uint16_t)(s << 4 | l);
    }
    return left > 0 ? 2 : 0;
}

// the symbol that the waiting bits spell (behind a fill), dropped from them; or kInflateBitsRunOut, kInflateUnusedCode
AFQ_HD uint32_t inflate_symbol(InflateBits& b, const uint16_t* fast, uint32_t fast_bits, const uint16_t* count, const uint16_t* sorted, uint32_t n_sorted, uint32_t& sym) {
    const uint32_t e = AFQ_INFLATE_UNI(fast[(uint32_t)b.buf & ((1u << fast_bits) - 1)]);
    if (e) {
        const uint32_t l = e & 15u;
        if (l > b.cnt) return kInflateBitsRunOut;
        b.buf >>= l; b.cnt -= l;
        sym = e >> 4;
        return kInflateOk;
    }
    uint32_t code = 0, first = 0, index = 0;
    uint64_t bits = b.buf;
    for (uint32_t l = 1; l <= kInflateMaxBits; ++l) {
        if (l > b.cnt) return kInflateBitsRunOut;
        code |= (uint32_t)bits & 1u;
        bits >>= 1;
        const uint32_t c = AFQ_INFLATE_UNI(count[l]);
        if (code - first < c && index + (code - first) < n_sorted) {   // (code >= first, or the difference wraps and is no count)
            sym = AFQ_INFLATE_UNI(sorted[index + (code - first)]);
            b.buf >>= l; b.cnt -= l;
            return kInflateOk;
        }
        index += c; first = (first + c) << 1; code <<= 1;
    }
    return kInflateUnusedCode;
}

// the header of a dynamic block behind its three bits: HLIT, HDIST, HCLEN, the code-length code, the lengths, both tables
template <class Src>
AFQ_HD uint32_t inflate_dynamic_header(Src& src, InflateState& S, InflateTables& T) {
    uint32_t v = 0;
    inflate_fill(src, S.b, S.in_len);
    if (!inflate_take(S.b, 14, v)) return kInflateBitsRunOut;
    const uint32_t nlen = (v & 31u) + 257, ndist = ((v >> 5) & 31u) + 1, ncl = (v >> 10) + 4;
    if (nlen > 286) return kInflateBadLitLenSet;
    if (ndist > 30) return kInflateBadDistSet;
    for (uint32_t i = 0; i < 19; ++i) T.cl_lens[i] = 0;
    for (uint32_t i = 0; i < ncl; ++i) {
        inflate_fill(src, S.b, S.in_len);
        if (!inflate_take(S.b, 3, v)) return kInflateBitsRunOut;
        // 16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15: five bits a place
        const uint32_t at = i < 12 ? (uint32_t)((0x22CAA324E804A30ull >> (5 * i)) & 31u) : (uint32_t)((0x3C2E1346Cull >> (5 * (i - 12))) & 31u);
        T.cl_lens[at] = (uint8_t)v;
    }
    bool single = false;
    if (inflate_build(T.cl_lens, 19, T.dist_fast, kInflateClFastBits, T.cl_count, T.cl_sorted, T.work, single) != 0) return kInflateBadCodeLengthSet;
    uint32_t have = 0, prev = 0;
    while (have < nlen + ndist) {
        uint32_t sym = 0;
        inflate_fill(src, S.b, S.in_len);
        if (const uint32_t rc = inflate_symbol(S.b, T.dist_fast, kInflateClFastBits, T.cl_count, T.cl_sorted, 19, sym)) return rc;
        if (sym < 16) { T.lens[have++] = (uint8_t)sym; prev = sym; continue; }
        uint32_t rep = 0, val = 0;
        if (sym == 16) {
            if (!have) return kInflateBadCodeLengthSet;
            if (!inflate_take(S.b, 2, v)) return kInflateBitsRunOut;
            rep = 3 + v; val = prev;
        } else if (sym == 17) {
            if (!inflate_take(S.b, 3, v)) return kInflateBitsRunOut;
            rep = 3 + v;
        } else {
            if (!inflate_take(S.b, 7, v)) return kInflateBitsRunOut;
            rep = 11 + v;
        }
        if (rep > nlen + ndist - have) return kInflateBadCodeLengthSet;
        for (uint32_t k = 0; k < rep; ++k) T.lens[have++] = (uint8_t)val;
        prev = val;
    }
    if (AFQ_INFLATE_UNI(T.lens[256]) == 0) return kInflateNoEndOfBlock;
    const uint32_t rl = inflate_build(T.lens, nlen, T.lit_fast, kInflateFastBits, T.lit_count, T.lit_sorted, T.work, single);
    if (rl == 1 || rl == 3 || (rl == 2 && !single)) return kInflateBadLitLenSet;
    const uint32_t rd = inflate_build(T.lens + nlen, ndist, T.dist_fast, kInflateFastBits, T.dist_count, T.dist_sorted, T.work, single);
    if (rd == 1 || (rd == 2 && !single)) return kInflateBadDistSet;   // (3: literals only)
    return kInflateOk;
}

AFQ_HD void inflate_fixed_tables(InflateTables& T) {
    for (uint32_t s = 0; s < 288; ++s) T.lens[s] = (uint8_t)(s < 144 ? 8 : s < 256 ? 9 : s < 280 ? 7 : 8);
    for (uint32_t s = 0; s < 32; ++s) T.lens[288 + s] = 5;
    bool single = false;
    (void)inflate_build(T.lens, 288, T.lit_fast, kInflateFastBits, T.lit_count, T.lit_sorted, T.work, single);
    (void)inflate_build(T.lens + 288, 32, T.dist_fast, kInflateFastBits, T.dist_count, T.dist_sorted, T.work, single);
}

// What comes next in the stream.  Behind a code nothing more may be asked of the state.
template <class Src>
AFQ_HD InflateStep inflate_next(Src& src, InflateState& S, InflateTables& T) {
    InflateStep e{kInflateOk, kInflateEnd, 0, 0, 0, 0};
    uint32_t v = 0;
    for (;;) {
        if (!S.in_block) {
            if (S.final_seen) {   // what lies behind the final block is not looked at
                if (S.produced != S.isize) e.code = kInflateOutputShort;
                return e;
            }
            inflate_fill(src, S.b, S.in_len);
            if (!inflate_take(S.b, 3, v)) { e.code = kInflateBitsRunOut; return e; }
            S.final_seen = v & 1u;
            const uint32_t type = v >> 1;
            if (type == 3) { e.code = kInflateReservedType; return e; }
            if (type == 0) {
                (void)inflate_take(S.b, S.b.cnt & 7u, v);   // to the byte's edge
                inflate_fill(src, S.b, S.in_len);
                if (!inflate_take(S.b, 32, v)) { e.code = kInflateBitsRunOut; return e; }
                const uint32_t len = v & 0xFFFFu;
                if (len != (~(v >> 16) & 0xFFFFu)) { e.code = kInflateStoredLenDisagrees; return e; }
                const uint32_t at = S.b.pos - S.b.cnt / 8;   // the waiting bits are whole bytes of the body: they go back to it
                if (len > S.in_len - at) { e.code = kInflateStoredPastBody; return e; }
                if (len > S.isize - S.produced) { e.code = kInflateOutputPastIsize; return e; }
                S.b.buf = 0; S.b.cnt = 0; S.b.pos = at + len;
                S.n_stored += 1;
                if (!len) continue;
                S.produced += len;
                e.kind = kInflateStoredRun; e.len = len; e.src = at;
                return e;
            }
            if (type == 1) { inflate_fixed_tables(T); S.n_fixed += 1; }
            else {
                if (const uint32_t rc = inflate_dynamic_header(src, S, T)) { e.code = rc; return e; }
                S.n_dynamic += 1;
            }
            S.in_block = 1;
        }
        uint32_t sym = 0;
        inflate_fill(src, S.b, S.in_len);
        if (const uint32_t rc = inflate_symbol(S.b, T.lit_fast, kInflateFastBits, T.lit_count, T.lit_sorted, kInflateMaxLitLen, sym)) { e.code = rc; return e; }
        if (sym < 256) {
            if (S.produced >= S.isize) { e.code = kInflateOutputPastIsize; return e; }
            S.produced += 1; S.n_literals += 1;
            e.kind = kInflateLiteral; e.lit = sym;
            return e;
        }
        if (sym == 256) { S.in_block = 0; continue; }
        if (sym >= 286) { e.code = kInflateLitLenSymbol; return e; }
        // lengths 3..258: symbols 257..264 one each, then groups of four with 1..5 extra bits, 285 is 258
        uint32_t len, xb;
        sym -= 257;
        if (sym < 8) { len = 3 + sym; xb = 0; }
        else if (sym == 28) { len = 258; xb = 0; }
        else { xb = (sym >> 2) - 1; len = 3 + ((4 + (sym & 3u)) << xb); }
        if (!inflate_take(S.b, xb, v)) { e.code = kInflateBitsRunOut; return e; }
        len += v;
        inflate_fill(src, S.b, S.in_len);
        if (const uint32_t rc = inflate_symbol(S.b, T.dist_fast, kInflateFastBits, T.dist_count, T.dist_sorted, kInflateMaxDist, sym)) { e.code = rc; return e; }
        if (sym >= 30) { e.code = kInflateDistSymbol; return e; }
        // distances 1..32768: symbols 0..3 one each, then pairs with 1..13 extra bits
        uint32_t dist;
        if (sym < 4) { dist = 1 + sym; xb = 0; }
        else { xb = (sym >> 1) - 1; dist = 1 + ((2 + (sym & 1u)) << xb); }
        if (!inflate_take(S.b, xb, v)) { e.code = kInflateBitsRunOut; return e; }
        dist += v;
        if (dist > S.produced) { e.code = kInflateDistPastStart; return e; }
        if (len > S.isize - S.produced) { e.code = kInflateOutputPastIsize; return e; }
        S.produced += len; S.n_copies += 1;
        e.kind = kInflateCopy; e.len = len; e.dist = dist;
        return e;
    }
}

// the codes' words, for the sentences of the entry points
inline const char* inflate_code_words(uint32_t code) {
    switch (code) {
        case kInflateBitsRunOut: return "the bits run out";
        case kInflateReservedType: return "a block of the reserved type";
        case kInflateStoredLenDisagrees: return "a stored block's length is not its complement's";
        case kInflateStoredPastBody: return "a stored block runs past the payload";
        case kInflateBadCodeLengthSet: return "bad code lengths";
        case kInflateBadLitLenSet: return "a bad literal/length code";
        case kInflateBadDistSet: return "a bad distance code";
        case kInflateNoEndOfBlock: return "no end-of-block code";
        case kInflateLitLenSymbol: return "literal/length symbol 286 or 287";
        case kInflateDistSymbol: return "distance symbol 30 or 31";
        case kInflateDistPastStart: return "a copy from in front of the block";
        case kInflateOutputPastIsize: return "more bytes than ISIZE";
        case kInflateUnusedCode: return "bits that are no code of the set";
        default: return "";
    }
}

}  // namespace afq
