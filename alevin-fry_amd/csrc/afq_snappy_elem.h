// afq_snappy_elem.h — the element parser of a raw snappy block, for the host and the device alike (k_snappy_decode of
// afq_snappy.hip; tests/snappy_elem_check.cpp runs it under the host sanitizers).  One call looks at one element and either
// hands out what may be moved - kind, length, offset, where a literal's bytes start, where the next element starts - or a code.
// Every check stands in front of the byte it guards: a byte of the body is fetched only below in_len, and an element is handed
// out only if all of it lies inside the body and all it produces lies inside [0, ulen) with its source inside [0, w).  A loop
// that moves only what it is handed cannot leave either buffer, whatever the body holds.
//
// The body is read through `byte(i)`, i < in_len, so that the device can serve it from a staged window.
#pragma once
#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define AFQ_HD __host__ __device__ __forceinline__
#else
#define AFQ_HD inline
#endif

namespace afq {

// what is wrong with a chunk (the low byte of the decoder's status word, the chunk's index above it)
enum SnappyDecodeCode : uint32_t {
    kSnappyOk = 0,
    kSnappyLiteralPastBody = 1,    // a literal's bytes do not all lie inside the body
    kSnappyOffsetZero = 2,         // a copy from 0 back
    kSnappyOffsetPastStart = 3,    // a copy from further back than bytes were produced
    kSnappyOutputPastUlen = 4,     // an element would produce bytes behind the declared length
    kSnappyTagCutOff = 5,          // the bytes a tag announces (length bytes, offset bytes) are not all there
    kSnappyOutputShort = 6,        // the body ends with fewer bytes produced than declared
    kSnappyLengthDisagrees = 7,    // the body's own uvarint is malformed or is not the planned length
    kSnappyCrcMismatch = 8,        // the bytes decode; their masked CRC-32C is not the chunk's
    kSnappyCodeCount
};
constexpr uint32_t kSnappyElemMaxHeader = 5;   // a tag and at most 4 bytes behind it

struct SnappyElem {
    uint32_t code;     // kSnappyOk, or why nothing may move
    uint32_t copy;     // 0: literal, 1: copy
    uint32_t len;      // bytes produced, >= 1
    uint32_t off;      // copy: 1..w back from w
    uint32_t src;      // literal: its first byte's index in the body
    uint32_t next;     // the next element's index in the body
};

// The body's leading uvarint: at most 5 bytes.  Returns the index behind it, 0 where it is malformed or cut off.
template <class Byte>
AFQ_HD uint32_t snappy_elem_length(Byte&& byte, uint32_t in_len, uint64_t& declared) {
    declared = 0;
    for (uint32_t i = 0; i < 5; ++i) {
        if (i >= in_len) return 0;
        const uint32_t b = byte(i);
        declared |= (uint64_t)(b & 0x7fu) << (7 * i);
        if (!(b & 0x80u)) return i + 1;
    }
    return 0;
}

// The element at p < in_len, with w <= ulen <= 65536 bytes produced so far.
template <class Byte>
AFQ_HD SnappyElem snappy_elem_parse(Byte&& byte, uint32_t in_len, uint32_t p, uint32_t w, uint32_t ulen) {
    SnappyElem e{kSnappyOk, 0, 0, 0, 0, 0};
    const uint32_t left = in_len - p;          // >= 1
    const uint32_t tag = byte(p);
    const uint32_t kind = tag & 3u;
    if (kind == 0) {
        uint32_t len = tag >> 2, extra = 0;
        if (len >= 60) {
            extra = len - 59;                   // 1..4 length bytes
            if (1 + extra > left) { e.code = kSnappyTagCutOff; return e; }
            len = 0;
            for (uint32_t i = 0; i < extra; ++i) len |= (uint32_t)byte(p + 1 + i) << (8 * i);
        }
        // len + 1 bytes; len may be 2^32 - 1, so it is compared before 1 is added
        const uint32_t room = left - 1 - extra;
        if (len >= room) { e.code = kSnappyLiteralPastBody; return e; }
        if (len >= ulen - w) { e.code = kSnappyOutputPastUlen; return e; }
        e.len = len + 1;
        e.src = p + 1 + extra;
        e.next = e.src + e.len;
        return e;
    }
    const uint32_t extra = kind == 1 ? 1u : kind == 2 ? 2u : 4u;
    if (1 + extra > left) { e.code = kSnappyTagCutOff; return e; }
    uint32_t len, off;
    if (kind == 1) {
        len = 4 + ((tag >> 2) & 7u);
        off = ((tag >> 5) << 8) | byte(p + 1);
    } else {
        len = 1 + (tag >> 2);
        off = 0;
        for (uint32_t i = 0; i < extra; ++i) off |= (uint32_t)byte(p + 1 + i) << (8 * i);
    }
    if (off == 0) { e.code = kSnappyOffsetZero; return e; }
    if (off > w) { e.code = kSnappyOffsetPastStart; return e; }
    if (len > ulen - w) { e.code = kSnappyOutputPastUlen; return e; }
    e.copy = 1; e.len = len; e.off = off;
    e.next = p + 1 + extra;
    return e;
}

}  // namespace afq
