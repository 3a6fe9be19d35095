// Stand-alone check of kws::PackPool (keyword-spotting_amd/csrc/kws_pack_pool.h), built by tests/test_pack_pool_cpu.py as host
// code under the thread sanitizer and under the address + undefined-behaviour sanitizers.  Pools of 0, 1, 3, 5 and 64 threads
// copy buffers around the pool's 1 MiB threshold and around the sizes the ingest tests use (33 and 40 clips of 32000 bytes),
// three times each on the same pool, into a destination with 32 guard bytes on either side: every copy must equal its
// source and no guard byte may move.  Exit status 0: all good; 1: a mismatch (printed to stderr).
#include <cstdint>
#include <cstdio>
#include <vector>

#include "kws_pack_pool.h"

namespace {

constexpr size_t GUARD = 32;
constexpr unsigned char GUARD_BYTE = 0xA5, STALE_BYTE = 0x5A;

// a byte pattern that differs between positions 4096 apart (the slice granule) and between repeats
unsigned char pattern(size_t i, unsigned salt) { return (unsigned char)((i * 2654435761u + (i >> 12) * 97u + salt * 131u) >> 7); }

int check(kws::PackPool& pool, int threads, size_t bytes, int repeat) {
    std::vector<unsigned char> src(bytes + 1), dst(bytes + 2 * GUARD);  // + 1: a real pointer for the copy of 0 bytes too
    for (size_t i = 0; i < bytes; ++i) src[i] = pattern(i, (unsigned)(threads * 8 + repeat));
    for (size_t i = 0; i < dst.size(); ++i) dst[i] = i < GUARD || i >= GUARD + bytes ? GUARD_BYTE : STALE_BYTE;
    pool.copy(dst.data() + GUARD, src.data(), bytes);
    int bad = 0;
    for (size_t i = 0; i < GUARD; ++i)
        if (dst[i] != GUARD_BYTE || dst[GUARD + bytes + i] != GUARD_BYTE) ++bad;
    if (bad) std::fprintf(stderr, "threads %d, %zu bytes, repeat %d: %d guard bytes moved\n", threads, bytes, repeat, bad);
    for (size_t i = 0; i < bytes; ++i)
        if (dst[GUARD + i] != src[i]) {
            std::fprintf(stderr, "threads %d, %zu bytes, repeat %d: byte %zu is %02x, not %02x\n", threads, bytes, repeat, i,
                         dst[GUARD + i], src[i]);
            return bad + 1;
        }
    return bad;
}

}  // namespace

int main() {
    const int pools[] = {0, 1, 3, 5, 64};
    const size_t MiB = (size_t)1 << 20;
    const size_t sizes[] = {0, 1, 4095, MiB - 1, MiB, MiB + 1, (size_t)33 * 32000 + 2, (size_t)40 * 32000};
    int bad = 0, copies = 0;
    for (int threads : pools) {
        kws::PackPool pool(threads);
        if (pool.size() > threads) {
            std::fprintf(stderr, "a pool of %d threads reports %d\n", threads, pool.size());
            ++bad;
        }
        for (size_t bytes : sizes)
            for (int repeat = 0; repeat < 3; ++repeat, ++copies) bad += check(pool, threads, bytes, repeat);
    }
    // a pool that is created and destroyed without a job (a context that never ingests a large chunk)
    { kws::PackPool idle(5); }
    std::printf("pack_pool_check: %d copies, %d failures\n", copies, bad);
    return bad ? 1 : 0;
}
