// afq_chunk_table.h — the checks every entry point makes of a caller's chunk table (offsets into a byte buffer, an 8-byte
// `nbytes, nrec` header at each), written so that no sum of caller-supplied numbers can wrap.  Plain C++, no HIP: the CPU
// suite compiles it on its own (tests/test_host_cpu.py).
#pragma once
#include <cstdint>

namespace afq {

enum ChunkFault { kChunkOk = 0, kChunkOffset, kChunkSize, kChunkRecords };

// Does an 8-byte header at `off` lie inside [0, n_bytes)?
inline bool chunk_header_inside(uint64_t off, uint64_t n_bytes) { return !(n_bytes < 8 || off > n_bytes - 8); }

// Stage A, before any byte is read: the first chunk whose header does not lie inside the buffer, or n.
inline uint32_t first_chunk_outside(const uint64_t* chunk_off, uint32_t n, uint64_t n_bytes) {
    uint32_t i = 0;
    while (i < n && chunk_header_inside(chunk_off[i], n_bytes)) ++i;
    return i;
}

// Stage B, on a fetched header: does the chunk lie inside the buffer (kChunkSize), and can it hold nrec records of at least
// min_rec bytes each behind its header (kChunkRecords)?
inline ChunkFault check_chunk_header(uint64_t off, uint32_t nbytes, uint32_t nrec, uint64_t n_bytes, uint32_t min_rec) {
    if (!chunk_header_inside(off, n_bytes) || nbytes < 8 || nbytes > n_bytes - off) return kChunkSize;
    return (uint64_t)nrec * min_rec > nbytes - 8u ? kChunkRecords : kChunkOk;   // (both factors are below 2^32)
}

}  // namespace afq
