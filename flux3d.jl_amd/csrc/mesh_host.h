// mesh_host.h -- host-side decisions shared by the units of the fit path (mesh.hip, mesh_losses.hip, mesh_update.hip, sampler.hip,
// chamfer_bwd.hip): the grid of a grid-stride mesh kernel and the check of a caller's scratch.  One definition each.
#pragma once
#include "fx3d_common.h"

namespace fx3d {

#ifndef FX3D_MESH_THREADS
#define FX3D_MESH_THREADS 256
#endif
constexpr int kMeshThreads = FX3D_MESH_THREADS;
constexpr int kMeshMaxBlocks = 4096;  // partial-sum slots of a loss's scratch; a launch takes at most mesh_grid_for()'s cap of them

// Grid of a grid-stride kernel over n elements, 256-thread blocks.  Plain gather / streaming kernels take up to 4096 blocks
// (every wave slot of the chip twice over); kernels that END IN A REDUCTION (one partial and one ticket arrival per block, the
// last block adds the partials) stop at 1024: edge_loss 20 / 22 / 26 us at 1024 / 2048 / 4096 blocks
// (profiles/r04_*_hbm_grid_sweep.txt).  Option mesh_max_blocks != 0 forces one cap for both.
// (round 5) `ew_cap`: the Laplacian adjoint's gather form wants NO cap -- one vertex per thread, 7 667 blocks at the 2 M-vertex sheet:
// 27.3 -> 25.2 us = 4.68 TB/s (caps 4 096 / 8 192 / 16 384 / none: 27.3 / 25.7 / 25.2 / 25.4); faces_areas loses half its speed
// beyond 4 096 (21.0 / 33.3 / 43.3 us), the edge forms do not care: same box, profiles/r05_v8_mesh_grid_caps.txt.  Both adjoints in one
// launch (<true, true>): 38.8 -> 36.9 us without the cap.
inline int mesh_grid_for(long long n, bool reduction = false, int ew_cap = kMeshMaxBlocks) {
    long long g = (n + kMeshThreads - 1) / kMeshThreads;
    if (g < 1) g = 1;
    int cap = opt(OPT_MESH_MAX_BLOCKS);
    if (cap < 1 || cap > kMeshMaxBlocks) cap = reduction ? 1024 : ew_cap;
    if (g > cap) g = cap;
    return (int)g;
}

// leaves the calling function with the status of a failed step
#define FX3D_TRY(call)                          \
    do {                                        \
        const fx3d_status rc__ = (call);        \
        if (rc__ != FX3D_OK) return rc__;       \
    } while (0)

// The caller's scratch `ws` of `have` bytes holds `need`: FX3D_OK, or FX3D_ERR_WORKSPACE with "<fn>: <what> too small (have < need
// bytes)".  what: "workspace", "CDF workspace", "fx3d_mesh_reg workspace".  (unit: the sampler's messages name no unit.)
inline fx3d_status ws_check(const char *fn, const char *what, const void *ws, size_t have, size_t need, const char *unit = " bytes") {
    if (ws && have >= need) return FX3D_OK;
    set_error("%s: %s too small (%zu < %zu%s)", fn, what, ws ? have : (size_t)0, need, unit);
    return FX3D_ERR_WORKSPACE;
}

}  // namespace fx3d
