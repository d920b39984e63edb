// afq_snappy_plan.h — the plan of a snappy frame stream: one walk over the 4-byte chunk headers, shared by the host decoder
// (afq_host.cpp) and the device decoder (afq_snappy_frame_decode_device, afq_api_collate.cpp).  Host code only.
#pragma once
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

// uncompressed length of a raw snappy block (leading uvarint); returns false on a malformed prefix
inline bool snappy_raw_length(const uint8_t* in, size_t n, uint64_t& ulen, size_t& hdr) {
    ulen = 0; int shift = 0; size_t p = 0;
    for (;;) { if (p >= n || shift > 35) return false; const uint8_t b = in[p++]; ulen |= (uint64_t)(b & 0x7F) << shift; if (!(b & 0x80)) break; shift += 7; }
    hdr = p;
    return true;
}

// Snappy frame format.  The data chunks of a frame are independent (<= 64 KiB of output each), so the stream is
// planned in one cheap pass over the chunk headers and decoded by several threads.
struct SnappyChunk { size_t in_off, in_len; uint64_t out_off, ulen; uint32_t crc; bool compressed; };
inline bool snappy_frame_plan(const uint8_t* in, size_t n, std::vector<SnappyChunk>& chunks, uint64_t& total, std::string& err) {
    size_t p = 0;
    total = 0;
    bool first = true;
    while (p < n) {
        if (p + 4 > n) { err = "truncated snappy frame header"; return false; }
        if (first && in[p] != 0xff) { err = "snappy stream does not start with its stream identifier"; return false; }   // as snap::read::FrameDecoder
        first = false;
        const uint8_t type = in[p];
        const size_t len = in[p + 1] | ((size_t)in[p + 2] << 8) | ((size_t)in[p + 3] << 16);
        p += 4;
        if (p + len > n) { err = "truncated snappy frame chunk"; return false; }
        if (type == 0xff) { if (len != 6 || std::memcmp(in + p, "sNaPpY", 6) != 0) { err = "bad snappy stream identifier"; return false; } }
        else if (type == 0x00 || type == 0x01) {
            if (len < 4) { err = "snappy chunk too short"; return false; }
            SnappyChunk c;
            c.crc = in[p] | ((uint32_t)in[p + 1] << 8) | ((uint32_t)in[p + 2] << 16) | ((uint32_t)in[p + 3] << 24);
            c.in_off = p + 4; c.in_len = len - 4; c.out_off = total; c.compressed = type == 0x00;
            if (c.compressed) { size_t h; if (!snappy_raw_length(in + c.in_off, c.in_len, c.ulen, h)) { err = "corrupt snappy block"; return false; } }
            else c.ulen = c.in_len;
            if (c.ulen > 65536) { err = "snappy chunk larger than the frame format's 65536-byte limit"; return false; }
            total += c.ulen;
            chunks.push_back(c);
        } else if (type >= 0x02 && type <= 0x7f) { err = "unskippable reserved snappy chunk"; return false; }
        // 0x80..0xfe: skippable / padding
        p += len;
    }
    return true;
}
