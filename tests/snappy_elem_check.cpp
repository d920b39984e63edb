// snappy_elem_check.cpp — csrc/afq_snappy_elem.h on the host: the device decoder's element parser with a serial executor that
// moves exactly what the parser hands out, byte by byte.  Body and output live in heap blocks of exactly in_len and ulen bytes, so
// that a sanitizer build (tests/test_snappy_elem_cpu.py) sees any byte the parser lets through that it should not have.
//
//   snappy_elem_check FILE      FILE: u32 count, then per chunk u32 ulen, u32 compressed, u32 in_len, in_len bytes
//   -> a line per chunk: "ok <crc32c of the bytes, hex>" or "err <code>"
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <memory>
#include <vector>

#include "../alevin-fry_amd/csrc/afq_snappy_elem.h"

using namespace afq;

static uint32_t crc32c(const uint8_t* p, size_t n) {
    uint32_t c = ~0u;
    for (size_t i = 0; i < n; ++i) {
        c ^= p[i];
        for (int k = 0; k < 8; ++k) c = (c & 1u) ? (c >> 1) ^ 0x82F63B78u : c >> 1;
    }
    return ~c;
}

// 0 and the bytes in out[0, ulen), or the code
static uint32_t decode_chunk(const uint8_t* body, uint32_t in_len, bool compressed, uint8_t* out, uint32_t ulen) {
    if (ulen > 65536) return kSnappyLengthDisagrees;
    if (!compressed) {
        if (in_len != ulen) return kSnappyLengthDisagrees;
        for (uint32_t i = 0; i < ulen; ++i) out[i] = body[i];
        return kSnappyOk;
    }
    auto byte = [&](uint32_t i) -> uint32_t { return body[i]; };
    uint64_t declared = 0;
    uint32_t p = snappy_elem_length(byte, in_len, declared), w = 0;
    if (!p || declared != ulen) return kSnappyLengthDisagrees;
    while (p < in_len) {
        const SnappyElem e = snappy_elem_parse(byte, in_len, p, w, ulen);
        if (e.code) return e.code;
        if (!e.copy) for (uint32_t i = 0; i < e.len; ++i) out[w + i] = body[e.src + i];
        else for (uint32_t i = 0; i < e.len; ++i) out[w + i] = out[w - e.off + i];
        w += e.len;
        p = e.next;
    }
    return w == ulen ? kSnappyOk : kSnappyOutputShort;
}

int main(int argc, char** argv) {
    if (argc != 2) { std::fprintf(stderr, "usage: snappy_elem_check FILE\n"); return 2; }
    std::FILE* f = std::fopen(argv[1], "rb");
    if (!f) { std::perror(argv[1]); return 2; }
    uint32_t count = 0;
    if (std::fread(&count, 4, 1, f) != 1) return 2;
    for (uint32_t k = 0; k < count; ++k) {
        uint32_t h[3];
        if (std::fread(h, 4, 3, f) != 3) { std::fprintf(stderr, "chunk %u: truncated header\n", k); return 2; }
        const uint32_t ulen = h[0], in_len = h[2];
        std::unique_ptr<uint8_t[]> body(new uint8_t[in_len]), out(new uint8_t[ulen <= 65536 ? ulen : 0]);
        if (in_len && std::fread(body.get(), 1, in_len, f) != in_len) { std::fprintf(stderr, "chunk %u: truncated body\n", k); return 2; }
        const uint32_t code = decode_chunk(body.get(), in_len, h[1] != 0, out.get(), ulen);
        if (code) std::printf("err %u\n", code);
        else std::printf("ok %08x\n", crc32c(out.get(), ulen));
    }
    std::fclose(f);
    return 0;
}
