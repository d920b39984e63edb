// afq_inflate.hip — k_bgzf_inflate: the BGZF blocks of a planned file on the device -> their inflated bytes (the plan is the
// host's hop over the block headers, afq_bgzf_plan.h).  ONE WAVE per BGZF block (a workgroup is one wave and takes one block),
// laid out as k_snappy_decode is: the block's output is built in LDS, at most 65536 bytes staged at the destination's residue,
// and its payload is read through an LDS window, so no symbol waits for global memory and a copy reads LDS, never bytes this
// kernel has written to memory.  The symbol loop is the wave's: every lane runs the parser of afq_inflate_elem.h on the same
// bits - its state is wave-uniform and lives in scalar registers, the decode tables (a 10-bit first-level lookup for each
// alphabet, the canonical counts and sorted symbols for longer codes) in LDS - and nothing moves that the parser has not
// handed out: lane 0 stores a literal, the wave moves a copy 64 bytes a trip (a copy with dist < len reads start + i mod dist,
// all of it in front of the copy's own bytes), a stored run goes from the window to the output.  Then the CRC-32 of the staged
// bytes by slices (wave_crc of afq_block_codec.h, gzip's polynomial) against the trailer's, and the write-out with 16-byte
// stores.  A block that is refused writes nothing and enters `index << 8 | code` into the status word by atomicMin: the
// lowest bad block is named whatever the schedule; one that ends short of ISIZE also enters `index << 32 | bytes produced`
// into the word behind it, for the host door's sentence.
#include <hip/hip_runtime.h>

#include "afq_block_codec.h"
#include "afq_common.h"
#include "afq_inflate_elem.h"
#include "afq_kernels.h"
#include "afq_prims.h"
#include "afq_rad_walk.h"

namespace afq {

namespace {

// the payload through the window: body[wbase, wend) stands at sw
struct WindowSrc {
    uint4* s_in;
    const uint8_t* body;
    uint32_t in_len, lane;
    uint32_t wbase, wend;
    const uint8_t* sw;
    __device__ __forceinline__ void stage(uint32_t at) {   // at < in_len
        const uint32_t n = min(kInflateWindow, in_len - at);
        sw = window_fill(s_in, body + at, n, lane, kInflateThreads);
        wbase = at; wend = at + n;
    }
    __device__ __forceinline__ uint32_t byte(uint32_t i) {   // i < in_len
        if (i < wbase || i >= wend) stage(i);
        return uni(sw[i - wbase]);
    }
    // (aligned words of the window; of what lies behind wend nothing is kept)
    __device__ __forceinline__ uint32_t le32(uint32_t i) {   // i + 4 <= in_len
        if (i < wbase || i + 4 > wend) stage(i);
        const uint32_t o = (uint32_t)(sw - (const uint8_t*)s_in) + (i - wbase);
        const uint32_t* t = (const uint32_t*)s_in;
        const uint32_t x = o >> 2, sh = o & 3u;
        const uint32_t w0 = t[x], w1 = t[x + 1];
        return uni(sh ? __builtin_amdgcn_alignbyte(w1, w0, sh) : w0);
    }
};

__global__ __launch_bounds__(kInflateThreads) void k_bgzf_inflate(const uint8_t* __restrict__ in, const BgzfDecBlock* __restrict__ plan, uint64_t first_index,
                                                                  uint8_t* __restrict__ dst, unsigned long long* __restrict__ status, unsigned long long* __restrict__ stats) {
    __shared__ uint4 s_out[(kInflateMaxOut + 16) / 16];
    __shared__ uint4 s_in[(kInflateWindow + 32) / 16];   // (+ the residue of the payload's address, + the word le32 touches behind the window)
    __shared__ uint32_t s_tab[256];
    __shared__ InflateTables s_huff;
    static_assert(sizeof(s_out) + sizeof(s_in) + sizeof(s_tab) + sizeof(InflateTables) == kInflateLds, "afq_inflate_limits reports the workgroup's LDS");
    static_assert(sizeof(InflateTables) % 4 == 0, "the tables are whole words");
    const uint32_t lane = threadIdx.x;
    const BgzfDecBlock c = plan[blockIdx.x];
    uint8_t* d = dst + c.out_off;
    const uint32_t in_len = uni(c.in_len), isize = uni(c.isize);
    uint8_t* so = (uint8_t*)s_out + ((uintptr_t)d & 15);   // so[i] is output byte i
    crc_table_fill<kCrc32Poly>(s_tab, lane);
    uint32_t code = kInflateOk;
    InflateState S;
    inflate_begin(S, in_len, min(isize, kInflateMaxOut));
    WindowSrc src{s_in, in + c.in_off, in_len, lane, 0, 0, (const uint8_t*)s_in};
    if (isize > kInflateMaxOut) code = kInflateOutputPastIsize;   // (the plan refuses it)
    uint32_t w = 0;   // bytes moved: S.produced in front of a step
    while (!code) {
        const InflateStep e = inflate_next(src, S, s_huff);
        code = uni(e.code);
        if (code) break;
        const uint32_t kind = uni(e.kind);
        if (kind == kInflateEnd) break;
        if (kind == kInflateLiteral) {
            if (lane == 0) so[w] = (uint8_t)e.lit;   // w < isize
            w += 1;
        } else if (kind == kInflateCopy) {
            const uint32_t len = uni(e.len), dist = uni(e.dist);   // 1 <= dist <= w, w + len <= isize
            const uint8_t* from = so + (w - dist);
            if (dist >= len) {
                for (uint32_t i = lane; i < len; i += kInflateThreads) so[w + i] = from[i];
            } else {
                // i mod dist for i < len <= 258, dist < 258: (i + 0.5) / dist is at least 1 / 516 from an integer, far more than
                // the reciprocal's error, so the quotient is exact
                const float r = __builtin_amdgcn_rcpf((float)dist);
                for (uint32_t i = lane; i < len; i += kInflateThreads) so[w + i] = from[i - dist * (uint32_t)(((float)i + 0.5f) * r)];
            }
            w += len;
        } else {
            const uint32_t len = uni(e.len), src0 = uni(e.src);   // [src0, src0 + len) lies in the payload, [w, w + len) below isize
            for (uint32_t done = 0; done < len;) {
                const uint32_t at = src0 + done;
                if (at < src.wbase || at >= src.wend) src.stage(at);
                const uint32_t k = min(len - done, src.wend - at);
                for (uint32_t i = lane; i < k; i += kInflateThreads) so[w + done + i] = src.sw[at - src.wbase + i];
                done += k;
            }
            w += len;
        }
        gpl_wave_lds_sync();   // one wave: its LDS operations complete in order; this keeps the compiler to that order
    }
    __syncthreads();
    if (!code && wave_crc<kCrc32Poly>(so, isize, crc_slice_lds(isize), nullptr, s_tab, lane) != c.crc) code = kInflateCrcMismatch;
    if (code) {
        if (lane == 0) {
            atomicMin(status, (unsigned long long)(first_index + blockIdx.x) << 8 | code);
            if (code == kInflateOutputShort) atomicMin(status + 1, (unsigned long long)(first_index + blockIdx.x) << 32 | S.produced);
        }
        return;
    }
    staged_write_out(d, so, isize, lane, kInflateThreads);
    if (lane < 7) {
        const uint32_t v = lane == 0 ? 1u : lane == 1 ? (isize ? 0u : 1u) : lane == 2 ? S.n_stored : lane == 3 ? S.n_fixed : lane == 4 ? S.n_dynamic : lane == 5 ? S.n_literals : S.n_copies;
        if (v) atomicAdd(&stats[lane], (unsigned long long)v);
    }
}

}  // namespace

void launch_bgzf_inflate(hipStream_t s, const uint8_t* in, const BgzfDecBlock* plan, uint32_t n_blocks, uint64_t first_index, uint8_t* dst, uint64_t* status, uint64_t* stats) {
    if (n_blocks) AFQ_LAUNCH(k_bgzf_inflate, n_blocks, kInflateThreads, s, in, plan, first_index, dst, (unsigned long long*)status, (unsigned long long*)stats);
}

}  // namespace afq
