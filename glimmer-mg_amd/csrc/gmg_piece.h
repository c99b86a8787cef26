// gmg_piece.h -- up to 16 bases of a packed batch as one word, read upwards or downwards: the piece the gathers that build new
// batches (gmg_extract.hip, gmg_splice.hip) assemble their output words from.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

// nb (1 .. 16) bases of a read whose base 0 is job-wide base S, from position p on, as 2-bit codes from bit 0: upwards p, p + 1, ...
// or downwards p, p - 1, ...  The caller keeps the piece inside the read; what the window holds beyond it (the neighbouring
// reads' bases, the guard words) is masked out here.
__device__ __forceinline__ uint32_t ext_piece(const uint32_t *__restrict__ src, uint64_t S, uint32_t p, bool down, bool comp, unsigned nb)
{
    uint32_t x;
    if (!down) {
        const uint64_t sg = S + p;
        const uint64_t w0 = sg >> 4;
        x = (uint32_t)(((uint64_t)src[w0] | ((uint64_t)src[w0 + 1] << 32)) >> (2u * (unsigned)(sg & 15)));
    } else {
        // the 16 bases that END at S + p (word -1 is the guard in front of the batch): base S + p lands in the top two bits;
        // bit reversal turns the order of the bases AND of the two bits of every base, the second of which is undone
        const int64_t lo = (int64_t)(S + p) - 15;
        const int64_t w0 = lo >> 4;
        x = (uint32_t)(((uint64_t)src[w0] | ((uint64_t)src[w0 + 1] << 32)) >> (2u * (unsigned)(lo & 15)));
        x = __brev(x);
        x = ((x >> 1) & 0x55555555u) | ((x & 0x55555555u) << 1);
    }
    if (comp) x ^= 0xffffffffu;
    return x & (nb >= 16 ? 0xffffffffu : ((1u << (2 * nb)) - 1u));
}
