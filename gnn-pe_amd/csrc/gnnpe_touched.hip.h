// gnnpe_touched.hip.h -- what gnnpe_touched.hip (libgnnpe_hip.so) shares with the set kernels of gnnpe_standing.hip
// (libgnnpe_online.so, which links the former): the mask of a bitmap row's last word and the ordered compaction of a row.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace gnnpe {

// the bits of word w of a row that stand for vertices below n
__device__ __forceinline__ uint32_t sets_word_below_n(uint32_t x, uint64_t w, uint64_t words, uint32_t n)
{
    const uint32_t tail = n & 31u;
    return tail && w == words - 1 ? x & ((1u << tail) - 1u) : x;
}

// k_sets_members of gnnpe_touched.hip on the stream: the ascending ids below n of the `words`-word bitmap row d_row into d_out (at
// most cap of them), their number into *d_total if that is given.  Waits for nothing.
hipError_t sets_members_launch(hipStream_t stream, const uint32_t *d_row, uint64_t words, uint32_t n, uint32_t *d_out, uint64_t cap,
                               unsigned long long *d_total);

}  // namespace gnnpe
