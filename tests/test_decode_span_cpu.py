"""CPU test of the scattering decoder's span load plan (csrc/afq_decode_span.h): a wave of k_decode_recs requests every row its
slabs will stage in front of its slab loop, and this header says which dwords those are.  A stand-alone program walks every chunk
length, every span start the tile table can hold for that length and every slab count, performs the planned loads on a heap array
of exactly the chunk's dwords under the address and undefined-behaviour sanitizers, and compares each slab's staged image with the
slab-at-a-time loader's (a dword below the chunk's end, zero from there on)."""
import os
import subprocess

from util import ROOT

SAN_MAIN = r'''
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include "afq_decode_span.h"
using namespace afq;

constexpr uint32_t kSlab = 256, kStage = 320, kWaveSlabs = 4, kTileSlabs = 4 * kWaveSlabs;
static_assert(kSlab == kSpanSlabWords && kStage == kSlab + kSpanRowWords && span_max_rows(kWaveSlabs) == 17, "the kernel's constants");

static void fail(const char* what, uint32_t nwords, uint32_t first, uint32_t slabs, uint32_t a, uint32_t b) {
    std::printf("%s: nwords %u first %u slabs %u (%u, %u)\n", what, nwords, first, slabs, a, b);
    std::exit(1);
}

// the slab-at-a-time loader (k_decode_recs' issue_slab_loads): dword i of the chunk where i < nwords, else 0
static uint32_t slab_word(const uint32_t* w, uint32_t nwords, uint32_t s0, uint32_t il) {
    const uint32_t i = s0 + il;
    return i < nwords ? w[i] : 0u;
}

int main() {
    unsigned long long loads = 0, spans = 0, whole = 0;
    for (uint32_t nwords = 6; nwords <= 5 * 1024 + 330; ++nwords) {
        uint32_t* w = static_cast<uint32_t*>(std::malloc(4ull * nwords));   // exactly the chunk: one dword further is the sanitizer's
        for (uint32_t i = 0; i < nwords; ++i) w[i] = (i * 2654435761u) | 1u;   // (never zero: a skipped load shows)
        const uint32_t cell_slabs = (nwords + kSlab - 1) / kSlab;   // as the host counts them
        // a wave's first slab: tile t, wave v -> min(cell_slabs, 16 t + 4 v), its last min(cell_slabs, first + 4); tiles as k_slab_setup writes them
        const uint32_t tiles = (cell_slabs + kTileSlabs - 1) / kTileSlabs;
        for (uint32_t t = 0; t < tiles; ++t)
            for (uint32_t v = 0; v < 4; ++v) {
                const uint32_t a = std::min(cell_slabs, t * kTileSlabs + v * kWaveSlabs);
                const uint32_t first = a * kSlab;
                // every slab count, the wave's own among them (fewer: a shorter span of the same chunk; more: slabs past the chunk's end)
                for (uint32_t slabs = 0; slabs <= kWaveSlabs; ++slabs) {
                    ++spans;
                    const uint32_t rows = span_rows(slabs);
                    if (rows != (slabs ? 4 * slabs + 1 : 0)) fail("rows", nwords, first, slabs, rows, 0);
                    uint32_t sp[17][64];
                    const bool all = span_is_whole(nwords, first, slabs, kWaveSlabs);
                    if (all != (slabs == kWaveSlabs && first + 17 * 64 <= nwords)) fail("whole", nwords, first, slabs, all, 0);
                    whole += all;
                    for (uint32_t r = 0; r < 17; ++r)
                        for (uint32_t l = 0; l < 64; ++l) {
                            const SpanLoad ld = span_load(nwords, first, slabs, r, l);
                            if (ld.index != first + r * 64 + l) fail("index", nwords, first, slabs, r, l);
                            if (ld.load && r >= rows) fail("a row past the last halo is loaded", nwords, first, slabs, r, l);
                            if (all && !ld.load) fail("the straight-line path skips a load", nwords, first, slabs, r, l);
                            // the straight-line path loads without looking at ld.load
                            sp[r][l] = (all || ld.load) ? w[ld.index] : 0u;
                            loads += (all || ld.load);
                        }
                    for (uint32_t k = 0; k < slabs; ++k)   // slab k stages rows 4k .. 4k+4 of the span
                        for (uint32_t il = 0; il < kStage; ++il) {
                            const uint32_t got = sp[4 * k + il / 64][il % 64], want = slab_word(w, nwords, first + k * kSlab, il);
                            if (got != want) fail("stage image", nwords, first, slabs, k, il);
                        }
                }
            }
        std::free(w);
    }
    std::printf("clean %llu spans %llu whole %llu loads\n", spans, whole, loads);
    return 0;
}
'''


def test_span_load_plan_under_the_sanitizers(tmp_path):
    """a stand-alone program with its own main over csrc/afq_decode_span.h, built with -fsanitize=address,undefined and run here
    (nothing is loaded into python under a sanitizer)"""
    src = tmp_path / "span.cpp"
    src.write_text(SAN_MAIN)
    exe = tmp_path / "span"
    csrc = os.path.join(ROOT, "alevin-fry_amd", "csrc")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", csrc, "-o", str(exe), str(src)], check=True, capture_output=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.startswith("clean "), r.stdout + r.stderr
    spans, whole, loads = (int(x) for x in r.stdout.split()[1::2])
    assert spans > 0 and 0 < whole < spans and loads > 0   # (both paths were walked)
