// gnnpe_update.hip.h -- what the two translation units that change the resident graph share (gnnpe_update.hip: edge batches and
// relabels; gnnpe_update_vertices.hip: vertex batches): the loader's kernels they launch, the identity map, the spare-buffer
// helpers, the event timers and the whole-graph check.
#pragma once

#include "gnnpe_common.h"

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

// device_ms and, with GNNPE_DEBUG=1, its parts: [0] after the uploads, [1] after the merge, [2] after the wait and the decision
// (before the rebuild's first copy), [3] after the rebuild
struct UpdateEvents {
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
    ~UpdateEvents()
    {
        for (hipEvent_t e : ev)
            if (e) (void)hipEventDestroy(e);
    }
};

// device_ms of a call that is one launch: events right around it on the stream (nothing is created where device_ms is NULL)
struct LaunchTimer {
    UpdateEvents E;
    double *out = nullptr;
    int begin(double *device_ms, hipStream_t stream)
    {
        if (!(out = device_ms)) return GNNPE_OK;
        GNNPE_HIP_TRY(hipEventCreate(&E.ev[0]));
        GNNPE_HIP_TRY(hipEventCreate(&E.ev[1]));
        GNNPE_HIP_TRY(hipEventRecord(E.ev[0], stream));
        return GNNPE_OK;
    }
    int end(hipStream_t stream)
    {
        if (!out) return GNNPE_OK;
        float ms = 0.f;
        GNNPE_HIP_TRY(hipEventRecord(E.ev[1], stream));
        GNNPE_HIP_TRY(hipEventSynchronize(E.ev[1]));
        GNNPE_HIP_TRY(hipEventElapsedTime(&ms, E.ev[0], E.ev[1]));
        *out = ms;
        return GNNPE_OK;
    }
};

}  // namespace gnnpe

static inline int require_whole_graph(const char *who, gnnpe_ctx *c)
{
    GNNPE_REQUIRE(c->have_graph && c->rows_identity, GNNPE_ERR_UNSUPPORTED, "%s: the whole graph must be on the device (gnnpe_load_csr)", who);
    GNNPE_REQUIRE(!c->multigraph, GNNPE_ERR_UNSUPPORTED, "%s: simple graphs only (gnnpe_set_multigraph_rows was called)", who);
    return GNNPE_OK;
}
