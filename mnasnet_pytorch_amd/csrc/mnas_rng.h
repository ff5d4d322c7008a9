// Counter-based random numbers for kernels whose output a CPU test must be able to state exactly: Philox4x32-10 (Salmon, Moraes,
// Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3", SC'11).  128-bit counter, 64-bit key, ten rounds, no state: the four
// output words are a pure function of (counter, key), the same on the host and on the device (include/mnas.h "device random
// numbers" states the rounds and three known answers; tests/erase_ref.py restates them in numpy).
#pragma once
#include <stdint.h>

#ifndef __host__
#define __host__
#define __device__
#endif

#define MNAS_PHILOX_M0 0xD2511F53u
#define MNAS_PHILOX_M1 0xCD9E8D57u
#define MNAS_PHILOX_W0 0x9E3779B9u
#define MNAS_PHILOX_W1 0xBB67AE85u

// The four output words for counter {c0, c1, c2, c3} and key {k0, k1}.  Each round: c' = {hi(M1 c2) ^ c1 ^ k0, lo(M1 c2),
// hi(M0 c0) ^ c3 ^ k1, lo(M0 c0)}, then the key moves on by the Weyl increments.  Scalars throughout: nothing here is an array a
// compiler could place in memory.
__host__ __device__ static inline void mnas_philox4x32_10_words(uint32_t& c0, uint32_t& c1, uint32_t& c2, uint32_t& c3, uint32_t k0,
                                                                uint32_t k1) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint64_t p0 = (uint64_t)MNAS_PHILOX_M0 * c0, p1 = (uint64_t)MNAS_PHILOX_M1 * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
        c0 = n0;
        c1 = (uint32_t)p1;
        c2 = n2;
        c3 = (uint32_t)p0;
        k0 += MNAS_PHILOX_W0;
        k1 += MNAS_PHILOX_W1;
    }
}
