// gnnpe_launch_timer.hip.h -- what the calls that change or read the resident graph share beyond the update kernels
// (gnnpe_update.hip.h, gnnpe_touched.hip): the event timers and the whole-graph check.
#pragma once

#include "gnnpe_common.h"

namespace gnnpe {

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
