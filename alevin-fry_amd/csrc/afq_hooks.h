// afq_hooks.h — the ONE place the library reads test hooks from the environment.
//
// AFQ_TEST_<NAME>: routing overrides and sizes that tests/ flips to reach every code path on inputs of a few thousand reads
// (which decoder, which parsimony route, how small a slab or a pool, where a range is cut).  A hook forces a route that
// production takes on some input of its own, never one it does not have; it changes WHICH path computes the rows, never the
// rows: every one of them is exercised by a parity test against the oracle.  Among them:
//   AFQ_TEST_POOL_WORDS=n        the parsimony pool is planned at n (12..32) words per read instead of 24: graphs outgrow it
//   AFQ_TEST_POOL_ROOM_WORDS=n   the device holds a parsimony pool of at most n words: run_range refuses a larger one with
//                                AFQ_ERR_OOM before it allocates, and finish_range's room check answers as such a device would -
//                                the no-room re-runs of a range whose graphs outgrew its pool, on a test box that always has room
//   AFQ_TEST_ROWS_DELAY_US=n     a range's rows start across the link n microseconds after they were enqueued on the copy stream (a
//                                host function in front of them): the stand-in for a slow link, under which the next range of the
//                                slot would compact into row buffers still being read unless it waits for rows_done
//   AFQ_TEST_CONVERT_SPAN_BYTES=n  afq_convert cuts the record stream into spans of about n bytes instead of 64 KiB: several spans, and
//                                span starts at chosen records, in a BAM of a few kilobytes (the RAD written does not depend on it)
//   AFQ_TEST_SNAPPY_DEC_ROOM_BYTES=n  afq_snappy_frame_decode_device answers as a device with at most n bytes free would: its AFQ_ERR_OOM
//                                with the sizes, before any allocation or launch - on a test box that always has room
//   AFQ_TEST_INFLATE_ROOM_BYTES=n  afq_bgzf_inflate_device answers likewise: AFQ_ERR_OOM with the sizes for what it still has to allocate
// Rounds 1-4 had grown 36 getenv() sites, two thirds of them measurement switches whose alternative had been measured and not
// kept; those alternatives are gone, as are (round 7) the last hooks that selected one and the per-phase clock builds (a
// measurement build is `make variant DEFS=...` of a scratch copy), and what is left besides the hooks is:
//   AFQ_EM_ORDER=canonical   the sequential f32 EM of rounds 1-3, bit-identical to the reference's arithmetic
//   AFQ_HOST_TIMING=1        where the host side of a batch spends its time, on stderr
#pragma once
#include <stdlib.h>
#include <string.h>

namespace afq {

inline const char* test_hook(const char* name) {
    char k[64] = "AFQ_TEST_";
    strncat(k, name, sizeof(k) - strlen(k) - 1);
    return getenv(k);
}
inline long test_hook_long(const char* name, long dflt) { const char* e = test_hook(name); return e ? atol(e) : dflt; }
inline bool test_hook_is(const char* name, const char* v) { const char* e = test_hook(name); return e && !strcmp(e, v); }
// AFQ_TEST_POOL_ROOM_WORDS: 0 (unset) = the device's own free memory decides
inline unsigned long long pool_room_words() { const long v = test_hook_long("POOL_ROOM_WORDS", 0); return v > 0 ? (unsigned long long)v : 0ull; }
inline bool em_order_canonical() { const char* e = getenv("AFQ_EM_ORDER"); return e && !strcmp(e, "canonical"); }

}  // namespace afq
