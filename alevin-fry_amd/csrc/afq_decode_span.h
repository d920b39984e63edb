// afq_decode_span.h — which dwords a wave of the scattering decoder (k_decode_recs, BINS != 0) loads for its slabs, as a pure
// function.  A wave's slabs are consecutive slabs of one cell's chunk, so every row it will stage - four rows of 64 dwords a slab
// and the 64-dword halo behind its last slab - is one contiguous span of the chunk, requested in one go in front of the slab loop.
// A dword at or past the chunk's end (nwords) is not read and counts as zero; rows past the halo of the wave's last slab are not
// read at all.  Plain C++ as well as HIP: the CPU suite compiles it on its own and performs the loads on a heap array of exactly
// nwords dwords under the sanitizers (tests/test_decode_span_cpu.py).
#pragma once
#include <cstdint>

#ifdef __HIPCC__
#define AFQ_SPAN_FN __host__ __device__ inline
#else
#define AFQ_SPAN_FN inline
#endif

namespace afq {

constexpr uint32_t kSpanSlabWords = 256;   // = kSlabWords
constexpr uint32_t kSpanRowWords = 64;     // a row: one dword a lane
constexpr uint32_t kSpanSlabRows = kSpanSlabWords / kSpanRowWords;
// rows a span of `slabs` slabs stages: the slabs' own and one halo row
constexpr uint32_t span_max_rows(uint32_t slabs) { return slabs * kSpanSlabRows + 1; }

struct SpanLoad {
    uint32_t index;   // dword index into the chunk
    bool load;        // false: nothing is read, the value is 0
};

// Rows the wave loads: none without a slab.
AFQ_SPAN_FN uint32_t span_rows(uint32_t n_slabs) { return n_slabs ? n_slabs * kSpanSlabRows + 1 : 0u; }

// One past the last dword the wave loads: the end of its last halo, or the chunk's end.  `first` is the first dword of the wave's
// first slab, a multiple of kSpanSlabWords below nwords where there is a slab (a cell has ceil(nwords / 256) slabs); nwords <= 2^30,
// so nothing here wraps.
AFQ_SPAN_FN uint32_t span_limit(uint32_t nwords, uint32_t first, uint32_t n_slabs) {
    const uint32_t end = first + span_rows(n_slabs) * kSpanRowWords;
    return n_slabs == 0 ? 0u : end < nwords ? end : nwords;
}

// The fast path's one wave-uniform test: all `max_slabs` slabs are there and the whole span lies inside the chunk, so that every
// lane loads every row.
AFQ_SPAN_FN bool span_is_whole(uint32_t nwords, uint32_t first, uint32_t n_slabs, uint32_t max_slabs) {
    return n_slabs == max_slabs && first + span_max_rows(max_slabs) * kSpanRowWords <= nwords;
}

// The load of (row, lane) of the span.
AFQ_SPAN_FN SpanLoad span_load(uint32_t nwords, uint32_t first, uint32_t n_slabs, uint32_t row, uint32_t lane) {
    const uint32_t i = first + row * kSpanRowWords + lane;
    return SpanLoad{i, i < span_limit(nwords, first, n_slabs)};
}

}  // namespace afq
