// kmc_walk_uniform.h -- batches whose reads all have the same length: the walk kernel's tile geometry in closed form.
//
// Plain C++ (a host compiler builds it for tests/test_walk_uniform_host.py); kmc_walk.hip.h uses the same functions on the device.
//
// The walk kernel's lanes read two offsets per tile and read, vstart[r] and vend[r].  When every read of a batch has
// the same length L, read r is bases [r * L, (r + 1) * L) and neither array has anything to say.  The host can see that
// without touching the device: max_read_len is >= every read's length (the caller's promise, include/kmc.h, or the
// maximum the device computed), so n_bases == n_reads * max_read_len forces every read to be exactly that long.
#pragma once
#include <stdint.h>

#ifdef __HIPCC__
#define KMC_UNI_FN __host__ __device__ inline
#else
#define KMC_UNI_FN inline
#endif

#define KMC_WALK_MAX_READ 416

// Is the batch uniform with length max_read_len?  (By division: n_reads * max_read_len could wrap.)  Reads longer than
// KMC_WALK_MAX_READ are walked as overlapping pieces and are never uniform.
KMC_UNI_FN bool kmc_walk_uniform(uint64_t n_reads, uint64_t n_bases, uint64_t max_read_len) {
    return max_read_len >= 1 && max_read_len <= KMC_WALK_MAX_READ && n_reads >= 1 &&
           n_bases % n_reads == 0 && n_bases / n_reads == max_read_len;
}

// What a lane holds of tile `tile` (reads 64 * tile ... 64 * tile + 63): its own read [a, e), and the wave's byte range
// [A, B) with its first 16-byte piece A16 and its number of pieces.
struct KmcWalkTile {
    uint64_t a, e, A, B, A16;
    uint32_t n_pieces, have;
};

// From the offsets (vstart = offsets, vend = offsets + 1 for short reads): lanes past the last read hold the last end
// twice; A is lane 0's start, B lane 63's end.  The kernel gets A and B by wave shuffles; this is the same in one place.
KMC_UNI_FN KmcWalkTile kmc_walk_tile_ragged(const uint64_t* vstart, const uint64_t* vend, uint64_t n_reads, uint64_t tile, uint32_t lane) {
    KmcWalkTile t;
    const uint64_t r0 = tile * 64, r = r0 + lane, r63 = r0 + 63;
    t.have = r < n_reads ? 1u : 0u;
    t.e = vend[t.have ? r : n_reads - 1];
    t.a = t.have ? vstart[r] : t.e;
    t.A = r0 < n_reads ? vstart[r0] : vend[n_reads - 1];
    t.B = vend[r63 < n_reads ? r63 : n_reads - 1];
    t.A16 = t.A & ~15ull;
    t.n_pieces = (uint32_t)((t.B - t.A16 + 15) >> 4);
    return t;
}

// The same for a uniform batch of reads of L bases, nothing loaded.
KMC_UNI_FN KmcWalkTile kmc_walk_tile_uniform(uint64_t n_reads, uint32_t L, uint64_t tile, uint32_t lane) {
    KmcWalkTile t;
    const uint64_t r0 = tile * 64 < n_reads ? tile * 64 : n_reads;
    const uint64_t r1 = n_reads - r0 < 64 ? n_reads : r0 + 64;   // r0 + nr
    const uint64_t r = r0 + lane;
    t.have = r < r1 ? 1u : 0u;
    t.a = (t.have ? r : n_reads) * L;
    t.e = t.have ? t.a + L : t.a;
    t.A = r0 * L;
    t.B = r1 * L;
    t.A16 = t.A & ~15ull;
    t.n_pieces = (uint32_t)((t.B - t.A16 + 15) >> 4);
    return t;
}
