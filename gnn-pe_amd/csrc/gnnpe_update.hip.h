// gnnpe_update.hip.h -- what the two translation units that change the resident graph share (gnnpe_update.hip: edge batches and
// relabels; gnnpe_update_vertices.hip: vertex batches): the loader's kernels they launch, the identity map, the spare-buffer
// helpers; the event timers and the whole-graph check are gnnpe_launch_timer.hip.h's.
#pragma once

#include "gnnpe_common.h"
#include "gnnpe_launch_timer.hip.h"

namespace gnnpe {

// gnnpe_kernels.hip.h (compiled into gnnpe_engine.hip): used as they are
__global__ void k_offsets_to_start_deg(uint32_t n, const uint32_t *__restrict__ offs, uint32_t *__restrict__ start,
                                       uint32_t *__restrict__ deg, uint8_t *__restrict__ present);
__global__ void k_gather_u32(uint64_t cnt, const uint32_t *__restrict__ idx, const uint32_t *__restrict__ table,
                             uint32_t *__restrict__ out);

// the map of the empty batch (entries, or vertices): everything stays where it is
static __global__ void k_map_identity(uint32_t entries, uint32_t *__restrict__ map)
{
    for (uint64_t j = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; j < entries; j += (uint64_t)gridDim.x * blockDim.x) map[j] = (uint32_t)j;
}

static inline void swap_buffers(DevBuf &a, DevBuf &b)
{
    std::swap(a.p, b.p);
    std::swap(a.bytes, b.bytes);
}

// room for `need` bytes without losing what `live` holds if the device refuses: a buffer that has to grow is allocated in `fresh`
static inline int grow_aside(const DevBuf &live, DevBuf &fresh, size_t need) { return need <= live.bytes ? GNNPE_OK : fresh.reserve(need); }

}  // namespace gnnpe
