// afq_bgzf_plan.h — the plan of a BGZF file (SAM/BAM specification, section 4.1): one hop over the block headers by BSIZE of the
// BC extra field, shared by the host inflate of `convert` (afq_host.cpp) and the device inflate (afq_bgzf_inflate_device,
// afq_api_inflate.cpp).  Host code only.
#pragma once
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

struct afq_ctx;

struct BgzfBlock { size_t data_off, data_len; uint64_t out_off; uint32_t isize, crc; };

// false: `err` says which block is refused and why
inline bool bgzf_plan(const uint8_t* in, size_t n, std::vector<BgzfBlock>& blocks, uint64_t& total, std::string& err) {
    auto le16 = [](const uint8_t* p) -> uint32_t { return (uint32_t)p[0] | (uint32_t)p[1] << 8; };
    auto le32 = [](const uint8_t* p) -> uint32_t { uint32_t v; std::memcpy(&v, p, 4); return v; };
    total = 0;
    for (size_t p = 0; p < n;) {
        const std::string at = "BGZF block " + std::to_string(blocks.size()) + ": ";
        if (n - p < 18) { err = at + "truncated: " + std::to_string(n - p) + " bytes where a block header has 18"; return false; }
        const uint8_t* h = in + p;
        if (h[0] != 0x1f || h[1] != 0x8b || h[2] != 8 || !(h[3] & 4)) { err = at + "bad gzip magic (1f 8b 08 with an extra field is expected)"; return false; }
        const size_t xlen = le16(h + 10);
        if (n - p < 12 + xlen) { err = at + "truncated inside the extra field"; return false; }
        long bsize = -1;
        for (size_t e = 12; e + 4 <= 12 + xlen;) {
            const size_t slen = le16(h + e + 2);
            if (h[e] == 'B' && h[e + 1] == 'C' && slen == 2 && e + 6 <= 12 + xlen) bsize = (long)le16(h + e + 4);
            e += 4 + slen;
        }
        if (bsize < 0) { err = at + "no BC extra field: not a BGZF block"; return false; }
        const size_t blk = (size_t)bsize + 1;
        if (blk < 12 + xlen + 8) { err = at + "BSIZE is smaller than the block's own header and trailer"; return false; }
        if (n - p < blk) { err = at + "truncated: the block has " + std::to_string(blk) + " bytes, the file " + std::to_string(n - p) + " more"; return false; }
        BgzfBlock b{p + 12 + xlen, blk - (12 + xlen) - 8, total, le32(h + blk - 4), le32(h + blk - 8)};
        if (b.isize > 65536) { err = at + "ISIZE " + std::to_string(b.isize) + " is above the 65536 bytes of a BGZF block"; return false; }
        total += b.isize;
        blocks.push_back(b);
        p += blk;
    }
    return true;
}

// afq_api_inflate.cpp, for afq_convert_with: bytes [from, from + n) of what afq_bgzf_inflate_device left resident on the context
// (out_on_device = 1, the same shift) to host memory.  Not exported.
__attribute__((visibility("hidden"))) int afq_bgzf_resident_to_host(afq_ctx* ctx, uint32_t shift, uint64_t from, uint8_t* dst, uint64_t n);
