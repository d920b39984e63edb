// inflate_elem_check.cpp — csrc/afq_inflate_elem.h on the host: the device inflater's parser with a serial executor that moves
// exactly what the parser hands out, byte by byte.  Payload, output and decode tables live in heap blocks of exactly in_len, isize
// and sizeof(InflateTables) bytes, so that a sanitizer build (tests/test_inflate_elem_cpu.py) sees any byte the parser lets
// through that it should not have.
//
//   inflate_elem_check FILE      FILE: u32 count, then per payload u32 isize, u32 in_len, in_len bytes
//   -> a line per payload: "ok <crc32 of the bytes, hex> <stored> <fixed> <dynamic> <literals> <copies>" or "err <code> <bytes produced>"
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <memory>

#include "../alevin-fry_amd/csrc/afq_inflate_elem.h"

using namespace afq;

static uint32_t crc32_of(const uint8_t* p, size_t n) {
    uint32_t c = ~0u;
    for (size_t i = 0; i < n; ++i) {
        c ^= p[i];
        for (int k = 0; k < 8; ++k) c = (c & 1u) ? (c >> 1) ^ 0xEDB88320u : c >> 1;
    }
    return ~c;
}

struct HeapSrc {
    const uint8_t* body;
    uint32_t byte(uint32_t i) { return body[i]; }
    uint32_t le32(uint32_t i) { return (uint32_t)body[i] | (uint32_t)body[i + 1] << 8 | (uint32_t)body[i + 2] << 16 | (uint32_t)body[i + 3] << 24; }
};

// 0 and the bytes in out[0, isize), or the code
static uint32_t inflate_payload(const uint8_t* body, uint32_t in_len, uint8_t* out, uint32_t isize, InflateState& S) {
    std::unique_ptr<InflateTables> T(new InflateTables);
    HeapSrc src{body};
    inflate_begin(S, in_len, isize);
    if (isize > kInflateMaxOut) return kInflateOutputPastIsize;
    uint32_t w = 0;
    for (;;) {
        const InflateStep e = inflate_next(src, S, *T);
        if (e.code) return e.code;
        if (e.kind == kInflateEnd) return kInflateOk;
        if (e.kind == kInflateLiteral) out[w++] = (uint8_t)e.lit;
        else if (e.kind == kInflateCopy) { for (uint32_t i = 0; i < e.len; ++i) out[w + i] = out[w - e.dist + i]; w += e.len; }
        else { for (uint32_t i = 0; i < e.len; ++i) out[w + i] = body[e.src + i]; w += e.len; }
        if (w != S.produced) return 255;   // (the executor and the parser count alike)
    }
}

int main(int argc, char** argv) {
    if (argc != 2) { std::fprintf(stderr, "usage: inflate_elem_check FILE\n"); return 2; }
    std::FILE* f = std::fopen(argv[1], "rb");
    if (!f) { std::perror(argv[1]); return 2; }
    uint32_t count = 0;
    if (std::fread(&count, 4, 1, f) != 1) return 2;
    for (uint32_t k = 0; k < count; ++k) {
        uint32_t h[2];
        if (std::fread(h, 4, 2, f) != 2) { std::fprintf(stderr, "payload %u: truncated header\n", k); return 2; }
        const uint32_t isize = h[0], in_len = h[1];
        std::unique_ptr<uint8_t[]> body(new uint8_t[in_len]), out(new uint8_t[isize <= kInflateMaxOut ? isize : 0]);
        if (in_len && std::fread(body.get(), 1, in_len, f) != in_len) { std::fprintf(stderr, "payload %u: truncated body\n", k); return 2; }
        InflateState S;
        const uint32_t code = inflate_payload(body.get(), in_len, out.get(), isize, S);
        if (code) std::printf("err %u %u\n", code, S.produced);
        else std::printf("ok %08x %u %u %u %u %u\n", crc32_of(out.get(), isize), S.n_stored, S.n_fixed, S.n_dynamic, S.n_literals, S.n_copies);
    }
    std::fclose(f);
    return 0;
}
