// The two mesh regularisers (gfx950): edge_loss, laplacian_loss, their adjoints in every form, the fused pair and the
// fx3d_mesh_reg plan of the fit iteration's passengers.
//
// Gather + reduce over packed arrays: HBM/L2-bandwidth bound.  The reference does the gathers with
// `verts[:, faces]` temporaries (src/metrics/mesh.jl:27-28) and runs laplacian_loss's SpMM on the host even for CuArray meshes
// (`cpu(transpose(verts))`, src/metrics/mesh.jl:12); here each is a single fused pass with a deterministic two-stage reduction
// (per-block double partials -> one fixed-order block).  Arithmetic order follows the reference expression by expression,
// unfused (-ffp-contract=off).
#include <cmath>

#include "fx3d_common.h"
#include "mesh_host.h"
#include "mesh_reg.h"

using namespace fx3d;

namespace {

constexpr int kThreads = kMeshThreads;
using meshreg::xcd_logical_block;  // (mesh_reg.h)

// Fused finalisation of a mean over per-block partial sums: every block publishes its sum and takes a ticket; the
// last arriver adds the partials in index order (deterministic) and writes loss = Float32(sum / count), then
// returns the ticket to zero.  Hand-off through 8-byte agent-scope atomics as in nn1_f16_kernel (chamfer.hip).
__device__ __forceinline__ void mean_finalize_last_block(double tot, double *partials, unsigned int *ticket, double count,
                                                         float *loss, double *sm) {
    __shared__ int is_last;
    unsigned long long *pp = reinterpret_cast<unsigned long long *>(partials);
    if (threadIdx.x == 0) {
        __hip_atomic_store(&pp[blockIdx.x], __builtin_bit_cast(unsigned long long, tot), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        is_last = ticket_arrive_last(ticket, gridDim.x, blockIdx.x);
    }
    __syncthreads();
    if (!is_last) return;
    double acc = 0.0;
    for (int i = threadIdx.x; i < (int)gridDim.x; i += kThreads)
        acc += __builtin_bit_cast(double, __hip_atomic_load(&pp[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
    __syncthreads();
    const double all = block_sum<kThreads>(acc, sm);
    if (threadIdx.x == 0) {
        *loss = (float)(all / count);
        __hip_atomic_store(ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// ---- edge_loss (src/metrics/mesh.jl:24-32) ---------------------------------------------------
__global__ __launch_bounds__(kThreads) void edge_loss_kernel(
    const float *__restrict__ verts, const int32_t *__restrict__ e1,
    const int32_t *__restrict__ e2, long long E, float target, double *__restrict__ partials,
    unsigned int *ticket, float *__restrict__ loss) {
    __shared__ double sm[kThreads / 64];
    double acc = 0.0;
    const long long stride = (long long)gridDim.x * kThreads;
    for (long long e0 = xcd_logical_block(blockIdx.x, gridDim.x) * kThreads + threadIdx.x; e0 < E; e0 += 4 * stride) {  // four edges in flight
        int i1[4], i2[4];
        P3 a[4], b[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const long long e = e0 + u * stride < E ? e0 + u * stride : e0;
            i1[u] = e1[e];
            i2[u] = e2[e];
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            a[u] = *reinterpret_cast<const P3 *>(verts + 3ll * i1[u]);
            b[u] = *reinterpret_cast<const P3 *>(verts + 3ll * i2[u]);
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const float d0 = a[u].x - b[u].x, d1 = a[u].y - b[u].y, d2 = a[u].z - b[u].z;
            const float nrm = sqrtf(((d0 * d0) + (d1 * d1)) + (d2 * d2));
            const float t = nrm - target;
            if (e0 + u * stride < E) acc += (double)(t * t);
        }
    }
    const double tot = block_sum<kThreads>(acc, sm);
    mean_finalize_last_block(tot, partials, ticket, (double)E, loss, sm);
}

__global__ __launch_bounds__(kThreads) void edge_loss_bwd_kernel(
    const float *__restrict__ verts, const int32_t *__restrict__ e1,
    const int32_t *__restrict__ e2, long long E, float target, float c, float *gverts) {
    for (long long e = (long long)blockIdx.x * kThreads + threadIdx.x; e < E;
         e += (long long)gridDim.x * kThreads) {
        const int i = e1[e], j = e2[e];
        const float d0 = verts[3ll * i] - verts[3ll * j];
        const float d1 = verts[3ll * i + 1] - verts[3ll * j + 1];
        const float d2 = verts[3ll * i + 2] - verts[3ll * j + 2];
        const float nrm = sqrtf(((d0 * d0) + (d1 * d1)) + (d2 * d2));
        if (!(nrm > 0.0f)) continue;
        const float g = c * 2.0f * (nrm - target) / nrm;
        atomicAdd(&gverts[3ll * i], g * d0);
        atomicAdd(&gverts[3ll * i + 1], g * d1);
        atomicAdd(&gverts[3ll * i + 2], g * d2);
        atomicAdd(&gverts[3ll * j], -(g * d0));
        atomicAdd(&gverts[3ll * j + 1], -(g * d1));
        atomicAdd(&gverts[3ll * j + 2], -(g * d2));
    }
}

using meshreg::lap_row;
using meshreg::lap_row_lds;
using meshreg::kLapStage;  // (mesh_reg.h)

__global__ __launch_bounds__(kThreads) void laplacian_loss_kernel(
    const float *__restrict__ verts, long long V, const int32_t *__restrict__ rowptr,
    const int32_t *__restrict__ colind, const float *__restrict__ vals,
    double *__restrict__ partials, unsigned int *ticket, float *__restrict__ loss) {
    __shared__ double sm[kThreads / 64];
    __shared__ float w_stage[(kThreads / 64) * kLapStage];
    __shared__ int c_stage[(kThreads / 64) * kLapStage];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    float *w_s = w_stage + wv * kLapStage;
    int *c_s = c_stage + wv * kLapStage;
    double acc = 0.0;
    for (long long ib = xcd_logical_block(blockIdx.x, gridDim.x) * kThreads + wv * 64; ib < V; ib += (long long)gridDim.x * kThreads) {  // (wave-uniform)
        const long long i = ib + lane;
        const bool ok = i < V;
        const int k0 = rowptr[ok ? i : V], k1 = ok ? rowptr[i + 1] : k0;
        const int k_lo = __builtin_amdgcn_readfirstlane(k0), k_hi = __builtin_amdgcn_readlane(k1, 63);
        const int nent = k_hi - k_lo;
        float s0, s1, s2;
        if (nent <= kLapStage) {
            for (int e = lane; e < nent; e += 64) {
                w_s[e] = vals[k_lo + e];
                c_s[e] = colind[k_lo + e];
            }
            __builtin_amdgcn_s_waitcnt(0xc07f);
            __builtin_amdgcn_wave_barrier();
            lap_row_lds(verts, w_s, c_s, k0 - k_lo, k1 - k_lo, s0, s1, s2);
            __builtin_amdgcn_wave_barrier();
        } else if (ok) {
            lap_row(verts, rowptr, colind, vals, i, s0, s1, s2);
        } else {
            s0 = s1 = s2 = 0.0f;
        }
        if (ok) acc += (double)sqrtf(((s0 * s0) + (s1 * s1)) + (s2 * s2));
    }
    const double tot = block_sum<kThreads>(acc, sm);
    mean_finalize_last_block(tot, partials, ticket, (double)V, loss, sm);
}

__global__ __launch_bounds__(kThreads) void laplacian_loss_bwd_kernel(
    const float *__restrict__ verts, long long V, const int32_t *__restrict__ rowptr,
    const int32_t *__restrict__ colind, const float *__restrict__ vals, float c, float *gverts) {
    for (long long i = (long long)blockIdx.x * kThreads + threadIdx.x; i < V;
         i += (long long)gridDim.x * kThreads) {
        float s0, s1, s2;
        lap_row(verts, rowptr, colind, vals, i, s0, s1, s2);
        const float nrm = sqrtf(((s0 * s0) + (s1 * s1)) + (s2 * s2));
        if (!(nrm > 0.0f)) continue;
        const float u0 = s0 / nrm, u1 = s1 / nrm, u2 = s2 / nrm;
        const int k1 = rowptr[i + 1];
        for (int k0 = rowptr[i]; k0 < k1; k0 += 8) {  // (weights and columns of a sweep first: the atomics do not wait entry by entry)
            float w[8];
            int col[8];
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const int k = k0 + e < k1 ? k0 + e : k1 - 1;
                w[e] = c * vals[k];
                col[e] = colind[k];
            }
#pragma unroll
            for (int e = 0; e < 8; ++e)
                if (k0 + e < k1) {
                    float *g = gverts + 3ll * col[e];
                    atomicAdd(&g[0], w[e] * u0);
                    atomicAdd(&g[1], w[e] * u1);
                    atomicAdd(&g[2], w[e] * u2);
                }
        }
    }
}

// The same adjoint WITHOUT float atomics and without scratch (round 3), bit-identical to the oracle's row-by-row scatter.  Vertex i
// receives (c L[r,i]) u_r from every row r that holds column i -- for a structurally symmetric L (the Laplacian of an undirected
// edge list) these are the columns of ITS OWN row, and ascending columns are the order in which the scatter reaches it.  A block takes
// kLapRows consecutive vertices; one THREAD PER ENTRY (i, r) of their rows recomputes u_r (the row sum of r: two dependent round
// trips, as in the forward) and picks L[r,i] up on the way, the contributions wait in LDS, and one thread per vertex adds its
// row's contributions in column order.  (A thread per vertex walking its neighbours' rows one after the other took 38 us on eight
// teapots -- a chain of ~20 round trips --, the scatter with its memset 14.7.)
constexpr int kLapRows = 32;
__global__ __launch_bounds__(kThreads) void laplacian_loss_bwd_gather_kernel(
    const float *__restrict__ verts, long long V, const int32_t *__restrict__ rowptr, const int32_t *__restrict__ colind,
    const float *__restrict__ vals, float c, float *gverts, int accumulate, unsigned int *missing) {
    __shared__ float contrib[kThreads][3];
    __shared__ int erow[kThreads];      // row (relative to the block's first) of the entry a thread handles
    __shared__ float acc[kLapRows][3];
    const long long i0 = (long long)blockIdx.x * kLapRows;
    const int nr = V - i0 < kLapRows ? (int)(V - i0) : kLapRows;
    const int tid = threadIdx.x;
    const int e_lo = rowptr[i0], e_hi = rowptr[i0 + nr];
    if (tid < kLapRows) { acc[tid][0] = 0.0f; acc[tid][1] = 0.0f; acc[tid][2] = 0.0f; }
    for (int base = e_lo; base < e_hi; base += kThreads) {  // (one pass unless the rows are unusually long)
        __syncthreads();
        if (tid < nr) {  // the rows mark their entries of this pass
            const int k0 = rowptr[i0 + tid] > base ? rowptr[i0 + tid] : base;
            const int k1 = rowptr[i0 + tid + 1] < base + kThreads ? rowptr[i0 + tid + 1] : base + kThreads;
            for (int k = k0; k < k1; ++k) erow[k - base] = tid;
        }
        __syncthreads();
        const int k = base + tid;
        float x0 = 0.0f, x1 = 0.0f, x2 = 0.0f;
        if (k < e_hi) {
            const long long i = i0 + erow[tid], r = colind[k];
            float s0 = 0.0f, s1 = 0.0f, s2 = 0.0f, wri = 0.0f;
            bool has = false;
            const int q1 = rowptr[r + 1];
            for (int q0 = rowptr[r]; q0 < q1; q0 += 8) {  // row r as in lap_row: weights and columns, then the gathers, then the sums
                float w[8];
                int col[8];
                P3 v[8];
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    const int q = q0 + e < q1 ? q0 + e : q1 - 1;
                    w[e] = vals[q];
                    col[e] = colind[q];
                }
#pragma unroll
                for (int e = 0; e < 8; ++e) v[e] = *reinterpret_cast<const P3 *>(verts + 3ll * col[e]);
#pragma unroll
                for (int e = 0; e < 8; ++e)
                    if (q0 + e < q1) {
                        s0 = s0 + w[e] * v[e].x;
                        s1 = s1 + w[e] * v[e].y;
                        s2 = s2 + w[e] * v[e].z;
                        if (col[e] == (int)i) { wri = w[e]; has = true; }
                    }
            }
            const float nrm = sqrtf(((s0 * s0) + (s1 * s1)) + (s2 * s2));
            // L[i,r] is stored but L[r,i] is not: the precondition (structural symmetry) does not hold; the contribution this
            // form cannot see is counted (an integer atomic: the count is deterministic) so that the caller can tell
            if (!has && missing) atomicAdd(missing, 1u);
            if (has && nrm > 0.0f) {
                const float cw = c * wri;
                x0 = cw * (s0 / nrm); x1 = cw * (s1 / nrm); x2 = cw * (s2 / nrm);
            } else {
                has = false;
            }
            erow[tid] = has ? erow[tid] : -1 - erow[tid];  // (a row of zero norm / a missing transpose entry contributes nothing: skipped, not added as 0)
        }
        contrib[tid][0] = x0; contrib[tid][1] = x1; contrib[tid][2] = x2;
        __syncthreads();
        if (tid < nr) {  // in column order
            const int k0 = rowptr[i0 + tid] > base ? rowptr[i0 + tid] : base;
            const int k1 = rowptr[i0 + tid + 1] < base + kThreads ? rowptr[i0 + tid + 1] : base + kThreads;
            float a0 = acc[tid][0], a1 = acc[tid][1], a2 = acc[tid][2];
            for (int kk = k0; kk < k1; ++kk)
                if (erow[kk - base] >= 0) { a0 = a0 + contrib[kk - base][0]; a1 = a1 + contrib[kk - base][1]; a2 = a2 + contrib[kk - base][2]; }
            acc[tid][0] = a0; acc[tid][1] = a1; acc[tid][2] = a2;
        }
    }
    __syncthreads();
    if (tid < nr) {
        const long long i = i0 + tid;
        gverts[3 * i] = accumulate ? gverts[3 * i] + acc[tid][0] : acc[tid][0];
        gverts[3 * i + 1] = accumulate ? gverts[3 * i + 1] + acc[tid][1] : acc[tid][1];
        gverts[3 * i + 2] = accumulate ? gverts[3 * i + 2] + acc[tid][2] : acc[tid][2];
    }
}

// ---- both mesh losses in ONE launch, both adjoints in ONE gather launch (the fit_mesh regularisers,
//      examples/fit_mesh.jl:80-83: 0.1 laplacian_loss + edge_loss, launch bound at teapot scale) -----------------------
// Forward: blocks [0, gV) take Laplacian rows, blocks [gV, gV + gE) take edges; every block publishes one Float64
// partial, the last arriver adds each range in index order and writes both means (+ the weighted total).  As a
// by-product the row kernel stores u_r = (L v)_r / ||(L v)_r|| and 1/deg(r) per vertex (float4): all the adjoint needs.
// Adjoint, gather form, one thread per vertex i walking row i of the Laplacian's CSR (columns ascending):
//   Laplacian term  sum_{r in row i}  (c_l L[r,i]) u_r,  L[r,i] = -1 (r == i) or 1/deg(r);
//   edge term       sum_{j ~ i}  -+ g_ij d_ij           (j < i: edge (j,i), i is its second vertex; j > i: edge (i,j)).
// Both sums run in exactly the order in which the oracle's row-by-row / edge-by-edge scatter reaches vertex i (rows and
// sorted edges ascending), with its expressions, so the gradients are BIT-IDENTICAL to the oracle -- and run to run:
// no float atomics (the scatter versions above depend on the atomics' arrival order in the last bit).
// Requires the CSR to be the Laplacian of the SAME edge list (it is: both are cached per mesh, src/rep/mesh.jl:957-1002).
__global__ __launch_bounds__(kThreads) void mesh_losses_kernel(meshreg::FwdArgs A) {
    __shared__ meshreg::FwdLds<kThreads> L;
    meshreg::fwd_block<kThreads>(A, (int)blockIdx.x, L);  // (mesh_reg.h: the same body rides in the sampler's draw launch)
}

// u_r and 1/deg(r) alone (the adjoint without a preceding fused forward)
__global__ __launch_bounds__(kThreads) void lap_unit_rows_kernel(const float *__restrict__ verts, long long V,
                                                                const int32_t *__restrict__ rowptr,
                                                                const int32_t *__restrict__ colind,
                                                                const float *__restrict__ vals, float4 *__restrict__ u_out) {
    for (long long i = xcd_logical_block(blockIdx.x, gridDim.x) * kThreads + threadIdx.x; i < V; i += (long long)gridDim.x * kThreads) {
        float s0, s1, s2;
        lap_row(verts, rowptr, colind, vals, i, s0, s1, s2);
        const float nrm = sqrtf(((s0 * s0) + (s1 * s1)) + (s2 * s2));
        const int k0 = rowptr[i], k1 = rowptr[i + 1];
        float invdeg = 0.0f;
        if (k1 - k0 >= 2) invdeg = colind[k0] == (int)i ? vals[k0 + 1] : vals[k0];
        const bool ok = nrm > 0.0f;
        u_out[i] = float4{ok ? s0 / nrm : 0.0f, ok ? s1 / nrm : 0.0f, ok ? s2 / nrm : 0.0f, invdeg};
    }
}

template <bool LAP, bool EDGE>
__global__ __launch_bounds__(kThreads) void mesh_losses_bwd_gather_kernel(
    const float *__restrict__ verts, long long V, const int32_t *__restrict__ rowptr, const int32_t *__restrict__ colind,
    const float4 *__restrict__ u, float c_lap, float c_edge, float target, float *__restrict__ gverts, int accumulate) {
    // (XCD-contiguous order for the Laplacian form: + 7 %; the edge form measured 8 % SLOWER with it and keeps the plain order)
    // (blockDim.x, not kThreads: small meshes are launched with one wave per block -- the fit loop's 9.6 k vertices are 38 blocks of 256
    //  but 151 of 64, and a vertex is a chain of dependent gathers: 10.0 -> ... us at eight teapots, round 6)
    const long long nt = (long long)blockDim.x;
    for (long long i = (LAP ? xcd_logical_block(blockIdx.x, gridDim.x) : (long long)blockIdx.x) * nt + threadIdx.x; i < V; i += (long long)gridDim.x * nt)
        meshreg::adjoint_vertex<LAP, EDGE>(verts, i, rowptr, colind, u, c_lap, c_edge, target, gverts, accumulate);  // (mesh_reg.h)
}

// the tutorial's sum from finished losses (the adjoint of a planned Ride by launches of its own)
__global__ void mesh_reg_total_kernel(const float *base, float w_lap, const float *ll, float w_edge, const float *le, float *total) {
    *total = ((base ? *base : 0.0f) + (w_lap * *ll)) + (w_edge * *le);
}

fx3d_status copy_back(float *host, const float *dev, hipStream_t st) {
    if (host) {
        FX3D_HIP(hipMemcpyAsync(host, dev, sizeof(float), hipMemcpyDeviceToHost, st));
        FX3D_HIP(hipStreamSynchronize(st));
    }
    return FX3D_OK;
}

// Scratch of the losses.  One loss: one Float64 partial per block.  The fused pair: the partials of both ranges, then the (4, V)
// unit rows of the Laplacian (16-byte aligned behind them), which the forward leaves for the adjoint.
constexpr size_t kPartialsBytes = sizeof(double) * kMeshMaxBlocks;
struct MeshLossWs {
    double *partials;  // the row blocks' slots, then the edge blocks'
    float4 *u;
    static size_t bytes(int64_t V) { return 2 * kPartialsBytes + sizeof(float4) * (size_t)V; }
    explicit MeshLossWs(void *ws) : partials(static_cast<double *>(ws)), u(reinterpret_cast<float4 *>(partials + 2 * kMeshMaxBlocks)) {}
};

// the arrival counter of a launch whose last block finalises the reduction (runtime.hip: ticket_slot)
fx3d_status take_ticket(hipStream_t st, unsigned int **ticket) {
    fx3d_status rc = FX3D_OK;
    *ticket = ticket_slot(&rc, st);
    return *ticket ? FX3D_OK : rc;
}

}  // namespace

extern "C" {

fx3d_status fx3d_mesh_loss_workspace_bytes(int64_t count, size_t *bytes) {
    FX3D_REQUIRE(bytes, "fx3d_mesh_loss_workspace_bytes: null output");
    (void)count;
    *bytes = kPartialsBytes;
    return FX3D_OK;
}

fx3d_status fx3d_edge_loss(const float *verts, int64_t V, const int32_t *edges, int64_t E,
                           float target, float *loss_dev, float *loss_host, void *ws,
                           size_t ws_bytes, fx3d_stream_t s) {
    FX3D_REQUIRE(verts && edges && loss_dev, "fx3d_edge_loss: null pointer");
    FX3D_REQUIRE(V > 0 && E > 0 && V < (1ll << 31), "fx3d_edge_loss: bad sizes V=%lld E=%lld",
                 (long long)V, (long long)E);
    FX3D_TRY(ws_check("fx3d_edge_loss", "workspace", ws, ws_bytes, kPartialsBytes));
    hipStream_t st = as_stream(s);
    double *partials = reinterpret_cast<double *>(ws);
    unsigned int *ticket;
    FX3D_TRY(take_ticket(st, &ticket));
    const int g = mesh_grid_for(E, true);
    {
        ProfileScope prof("edge_loss", st);
        hipLaunchKernelGGL(edge_loss_kernel, dim3(g), dim3(kThreads), 0, st, verts, edges, edges + E,
                           (long long)E, target, partials, ticket, loss_dev);  // the last block writes the mean
    }
    FX3D_LAUNCH_CHECK();
    return copy_back(loss_host, loss_dev, st);
}

fx3d_status fx3d_edge_loss_bwd(const float *verts, int64_t V, const int32_t *edges, int64_t E,
                               float target, float gout, float *gverts, int32_t accumulate, fx3d_stream_t s) {
    // scatter form for a caller that holds nothing but an edge list (any list: duplicates, any order): float atomics, the last
    // bit depends on their arrival order.  The wrappers use fx3d_edge_loss_bwd_adj.
    FX3D_REQUIRE(verts && edges && gverts, "fx3d_edge_loss_bwd: null pointer");
    FX3D_REQUIRE(V > 0 && E > 0, "fx3d_edge_loss_bwd: bad sizes");
    hipStream_t st = as_stream(s);
    if (!accumulate) FX3D_FILL(gverts, 0, sizeof(float) * 3 * (size_t)V, st);
    hipLaunchKernelGGL(edge_loss_bwd_kernel, dim3(mesh_grid_for(E)), dim3(kThreads), 0, st, verts, edges,
                       edges + E, (long long)E, target, gout / (float)E, gverts);
    FX3D_LAUNCH_CHECK();
    return FX3D_OK;
}

fx3d_status fx3d_edge_loss_bwd_adj(const float *verts, int64_t V, const int32_t *rowptr, const int32_t *colind, int64_t E,
                                   float target, float gout, float *gverts, int32_t accumulate, fx3d_stream_t s) {
    // gather form: vertex i walks its neighbours (the Laplacian's CSR row, ascending; the diagonal is skipped) -- the order in
    // which the oracle's edge-by-edge scatter over the sorted edge list reaches it.  One launch, no atomics, no memset node.
    FX3D_REQUIRE(verts && rowptr && colind && gverts, "fx3d_edge_loss_bwd_adj: null pointer");
    FX3D_REQUIRE(V > 0 && E > 0 && V < (1ll << 31), "fx3d_edge_loss_bwd_adj: bad sizes");
    hipStream_t st = as_stream(s);
    ProfileScope prof("edge_loss_bwd", st);
    hipLaunchKernelGGL((mesh_losses_bwd_gather_kernel<false, true>), dim3(mesh_grid_for(V)), dim3(kThreads), 0, st, verts, (long long)V,
                       rowptr, colind, static_cast<const float4 *>(nullptr), 0.0f, gout / (float)E, target, gverts, accumulate);
    FX3D_LAUNCH_CHECK();
    return FX3D_OK;
}

fx3d_status fx3d_laplacian_loss(const float *verts, int64_t V, const int32_t *rowptr,
                                const int32_t *colind, const float *vals, float *loss_dev,
                                float *loss_host, void *ws, size_t ws_bytes, fx3d_stream_t s) {
    FX3D_REQUIRE(verts && rowptr && colind && vals && loss_dev, "fx3d_laplacian_loss: null pointer");
    FX3D_REQUIRE(V > 0 && V < (1ll << 31), "fx3d_laplacian_loss: bad V=%lld", (long long)V);
    FX3D_TRY(ws_check("fx3d_laplacian_loss", "workspace", ws, ws_bytes, kPartialsBytes));
    hipStream_t st = as_stream(s);
    double *partials = reinterpret_cast<double *>(ws);
    unsigned int *ticket;
    FX3D_TRY(take_ticket(st, &ticket));
    const int g = mesh_grid_for(V, true);
    {
        ProfileScope prof("laplacian_loss", st);
        hipLaunchKernelGGL(laplacian_loss_kernel, dim3(g), dim3(kThreads), 0, st, verts, (long long)V,
                           rowptr, colind, vals, partials, ticket, loss_dev);  // the last block writes the mean
    }
    FX3D_LAUNCH_CHECK();
    return copy_back(loss_host, loss_dev, st);
}

fx3d_status fx3d_mesh_losses_workspace_bytes(int64_t V, int64_t E, size_t *bytes) {
    FX3D_REQUIRE(bytes && V > 0 && E >= 0, "fx3d_mesh_losses_workspace_bytes: bad argument");
    *bytes = MeshLossWs::bytes(V);
    return FX3D_OK;
}

fx3d_status fx3d_mesh_losses(const float *verts, int64_t V, const int32_t *rowptr, const int32_t *colind,
                             const float *vals, const int32_t *edges, int64_t E, float target, float w_lap, float w_edge,
                             const float *base_dev, float *loss_lap_dev, float *loss_edge_dev, float *total_dev,
                             void *ws, size_t ws_bytes, fx3d_stream_t s) {
    FX3D_REQUIRE(verts && rowptr && colind && vals && edges, "fx3d_mesh_losses: null pointer");
    FX3D_REQUIRE(loss_lap_dev || loss_edge_dev || total_dev, "fx3d_mesh_losses: no output requested");
    FX3D_REQUIRE(V > 0 && E > 0 && V < (1ll << 31), "fx3d_mesh_losses: bad sizes V=%lld E=%lld", (long long)V, (long long)E);
    FX3D_TRY(ws_check("fx3d_mesh_losses", "workspace", ws, ws_bytes, MeshLossWs::bytes(V)));
    hipStream_t st = as_stream(s);
    const MeshLossWs W(ws);
    unsigned int *ticket;
    FX3D_TRY(take_ticket(st, &ticket));
    const int gV = mesh_grid_for(V, true), gE = mesh_grid_for(E, true);
    {
        ProfileScope prof("mesh_losses", st);
        const meshreg::FwdArgs A{verts, (long long)V, rowptr, colind, vals, edges, edges + E, (long long)E, target, gV, gE, W.partials, ticket,
                                 w_lap, w_edge, base_dev, loss_lap_dev, loss_edge_dev, total_dev, W.u};
        hipLaunchKernelGGL(mesh_losses_kernel, dim3(gV + gE), dim3(kThreads), 0, st, A);
    }
    FX3D_LAUNCH_CHECK();
    return FX3D_OK;
}

fx3d_status fx3d_mesh_losses_bwd(const float *verts, int64_t V, const int32_t *rowptr, const int32_t *colind,
                                 const float *vals, int64_t E, float target, float g_lap, float g_edge, int32_t reuse_forward,
                                 float *gverts, int32_t accumulate, void *ws, size_t ws_bytes, fx3d_stream_t s) {
    FX3D_REQUIRE(verts && rowptr && colind && vals && gverts, "fx3d_mesh_losses_bwd: null pointer");
    FX3D_REQUIRE(V > 0 && E > 0 && V < (1ll << 31), "fx3d_mesh_losses_bwd: bad sizes");
    FX3D_TRY(ws_check("fx3d_mesh_losses_bwd", "workspace", ws, ws_bytes, MeshLossWs::bytes(V)));
    hipStream_t st = as_stream(s);
    float4 *u = MeshLossWs(ws).u;
    if (g_lap == 0.0f && g_edge == 0.0f) {  // both terms dropped: the gradient is exactly zero; never read the (possibly unbuilt) unit rows
        if (!accumulate) FX3D_FILL(gverts, 0, sizeof(float) * 3 * (size_t)V, st);
        return FX3D_OK;
    }
    if (!reuse_forward && g_lap != 0.0f) {  // no fx3d_mesh_losses on the same vertices and workspace before this call: build the unit rows
        hipLaunchKernelGGL(lap_unit_rows_kernel, dim3(mesh_grid_for(V)), dim3(kThreads), 0, st, verts, (long long)V, rowptr, colind, vals, u);
        FX3D_LAUNCH_CHECK();
    }
    ProfileScope prof("mesh_losses_bwd", st);
    // (a weight of exactly zero drops its term: the Laplacian adjoint alone is how the wrappers differentiate laplacian_loss on
    // LARGE meshes -- the scratch-free fx3d_laplacian_loss_bwd_sym recomputes every neighbour's row, 7 x the traffic).
    // g_lap == 0 is tested FIRST: that instantiation never touches u, which is unbuilt in exactly that case.
    if (g_lap == 0.0f)
        hipLaunchKernelGGL((mesh_losses_bwd_gather_kernel<false, true>), dim3(mesh_grid_for(V)), dim3(kThreads), 0, st, verts, (long long)V,
                           rowptr, colind, u, 0.0f, g_edge / (float)E, target, gverts, accumulate);
    else if (g_edge == 0.0f)
        hipLaunchKernelGGL((mesh_losses_bwd_gather_kernel<true, false>), dim3(mesh_grid_for(V, false, 1 << 22)), dim3(kThreads), 0, st, verts, (long long)V,
                           rowptr, colind, u, g_lap / (float)V, 0.0f, target, gverts, accumulate);
    else if (V <= 65536)  // a small mesh: one wave per block, over four times as many CUs
        hipLaunchKernelGGL((mesh_losses_bwd_gather_kernel<true, true>), dim3((unsigned)((V + 63) / 64)), dim3(64), 0, st, verts, (long long)V,
                           rowptr, colind, u, g_lap / (float)V, g_edge / (float)E, target, gverts, accumulate);
    else
        hipLaunchKernelGGL((mesh_losses_bwd_gather_kernel<true, true>), dim3(mesh_grid_for(V, false, 1 << 22)), dim3(kThreads), 0, st, verts, (long long)V,
                           rowptr, colind, u, g_lap / (float)V, g_edge / (float)E, target, gverts, accumulate);
    FX3D_LAUNCH_CHECK();
    return FX3D_OK;
}

fx3d_status fx3d_laplacian_loss_bwd(const float *verts, int64_t V, const int32_t *rowptr,
                                    const int32_t *colind, const float *vals, float gout,
                                    float *gverts, int32_t accumulate, fx3d_stream_t s) {
    // ANY CSR (asymmetric, pruned, directed, duplicate columns): the row-by-row scatter with float atomics -- always the
    // adjoint of the forward, the last bit depends on the atomics' arrival order (the raw entry point must not
    // assume a structure it cannot check).  Callers whose L is the Laplacian of an undirected edge list -- the Python and
    // Julia wrappers -- use fx3d_laplacian_loss_bwd_sym.
    FX3D_REQUIRE(verts && rowptr && colind && vals && gverts, "fx3d_laplacian_loss_bwd: null pointer");
    FX3D_REQUIRE(V > 0, "fx3d_laplacian_loss_bwd: bad V");
    hipStream_t st = as_stream(s);
    if (!accumulate) FX3D_FILL(gverts, 0, sizeof(float) * 3 * (size_t)V, st);
    hipLaunchKernelGGL(laplacian_loss_bwd_kernel, dim3(mesh_grid_for(V)), dim3(kThreads), 0, st, verts,
                       (long long)V, rowptr, colind, vals, gout / (float)V, gverts);
    FX3D_LAUNCH_CHECK();
    return FX3D_OK;
}

fx3d_status fx3d_laplacian_loss_bwd_sym(const float *verts, int64_t V, const int32_t *rowptr, const int32_t *colind,
                                        const float *vals, float gout, float *gverts, int32_t accumulate,
                                        uint32_t *missing_dev, fx3d_stream_t s) {
    // gather form: one launch, no atomics, bit-identical to the oracle.  PRECONDITION: L structurally symmetric (column i
    // in row r iff column r in row i), no duplicate columns in a row.  missing_dev (optional, caller-zeroed device counter)
    // receives the number of stored entries L[i,r] whose transpose L[r,i] is absent: non-zero means the precondition did
    // not hold and the gradient lacks those contributions -- use fx3d_laplacian_loss_bwd.
    FX3D_REQUIRE(verts && rowptr && colind && vals && gverts, "fx3d_laplacian_loss_bwd_sym: null pointer");
    FX3D_REQUIRE(V > 0, "fx3d_laplacian_loss_bwd_sym: bad V");
    if (opt(OPT_LAP_BWD_SCATTER)) return fx3d_laplacian_loss_bwd(verts, V, rowptr, colind, vals, gout, gverts, accumulate, s);
    hipStream_t st = as_stream(s);
    ProfileScope prof("laplacian_loss_bwd", st);
    hipLaunchKernelGGL(laplacian_loss_bwd_gather_kernel, dim3((unsigned int)((V + kLapRows - 1) / kLapRows)), dim3(kThreads), 0, st, verts,
                       (long long)V, rowptr, colind, vals, gout / (float)V, gverts, accumulate, missing_dev);
    FX3D_LAUNCH_CHECK();
    return FX3D_OK;
}

}  // extern "C"

// ---- the fit iteration's passengers (mesh_reg.h) --------------------------------------------------------------------------
namespace fx3d {
fx3d_status mesh_reg_plan(const fx3d_mesh_reg *reg, float gout, float *gverts, int accumulate, hipStream_t st, const char *fn, meshreg::Ride *out) {
    FX3D_REQUIRE(reg && reg->verts && reg->rowptr && reg->colind && reg->vals && reg->edges, "%s: fx3d_mesh_reg with a null pointer", fn);
    FX3D_REQUIRE(reg->loss_lap_dev && reg->loss_edge_dev, "%s: fx3d_mesh_reg needs loss_lap_dev and loss_edge_dev", fn);
    FX3D_REQUIRE(reg->V > 0 && reg->E > 0 && reg->V < (1ll << 31), "%s: fx3d_mesh_reg: bad sizes V=%lld E=%lld", fn, (long long)reg->V, (long long)reg->E);
    FX3D_TRY(ws_check(fn, "fx3d_mesh_reg workspace", reg->ws, reg->ws_bytes, MeshLossWs::bytes(reg->V)));
    unsigned int *ticket;
    FX3D_TRY(take_ticket(st, &ticket));
    const MeshLossWs W(reg->ws);
    meshreg::Ride R{};
    R.fwd = meshreg::FwdArgs{reg->verts, (long long)reg->V, reg->rowptr, reg->colind, reg->vals, reg->edges, reg->edges + reg->E, (long long)reg->E,
                             reg->target, mesh_grid_for(reg->V, true), mesh_grid_for(reg->E, true), W.partials, ticket, reg->w_lap, reg->w_edge, reg->base_dev,
                             reg->loss_lap_dev, reg->loss_edge_dev, reg->total_dev, W.u};
    R.c_lap = (reg->w_lap * gout) / (float)reg->V;
    R.c_edge = (reg->w_edge * gout) / (float)reg->E;
    R.gverts = gverts;
    R.accumulate = accumulate;
    R.nadj = (int)((reg->V + meshreg::kAdjPerBlock - 1) / meshreg::kAdjPerBlock);
    *out = R;
    return FX3D_OK;
}
fx3d_status mesh_reg_adjoint_standalone(const fx3d_mesh_reg *reg, float gout, float *gverts, int accumulate, hipStream_t st) {
    const fx3d_status rc = fx3d_mesh_losses_bwd(reg->verts, reg->V, reg->rowptr, reg->colind, reg->vals, reg->E, reg->target, reg->w_lap * gout,
                                                reg->w_edge * gout, 1, gverts, accumulate, reg->ws, reg->ws_bytes, reinterpret_cast<fx3d_stream_t>(st));
    if (rc) return rc;
    if (reg->total_dev) {
        hipLaunchKernelGGL(mesh_reg_total_kernel, dim3(1), dim3(1), 0, st, reg->base_dev, reg->w_lap, reg->loss_lap_dev, reg->w_edge, reg->loss_edge_dev,
                           reg->total_dev);
        FX3D_LAUNCH_CHECK();
    }
    return FX3D_OK;
}
}  // namespace fx3d
