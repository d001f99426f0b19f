// The exact nearest-neighbour kernels of the chamfer forward (gfx950): the oracle's arithmetic on the VALU, no filter.  Which of
// them a problem runs is the launch plan's choice (chamfer_host.hip: make_plan / plan_kernel); nn1_exact_launch at the end of
// this file picks the instantiation.
//   * nn1_small_d_kernel<DIM, R> (D = 2, and D = 3 under option nn1_variant = 0: the A/B reference) -- the exact VALU loop of
//     round 1: candidates staged through LDS as structure-of-arrays, tiles of 32 folded by v_min3, the winning tile re-scanned
//     with the reference's strict `<`.
//   * nn1_tiny_kernel (D = 3, problems below ~24 M pair evaluations) -- the exact loop with candidates broadcast along DPP
//     rows: no statistics, no image, no barrier before the arithmetic.
//   * nn1_generic_kernel (any other D).
#include <cmath>

#include "nn1_common.h"

using namespace fx3d;

namespace {

template <int DIM, int R, bool WANT_IDX>
__global__ __launch_bounds__(kThreads) void nn1_small_d_kernel(Nn1Params p) {
    extern __shared__ __attribute__((aligned(16))) float lds[];

    // ---- XCD-aware decode of the linear block id -> (cloud c, query tile) ------------------
    const int L = blockIdx.x;
    const int xcd = L & 7, slot = L >> 3;
    const int c = (slot / p.tiles) * 8 + xcd;  // cloud id in [0, 2B): dir = c / B
    const int tile = slot % p.tiles;
    if (c >= 2 * p.B) return;
    const int dir = c >= p.B ? 1 : 0;
    const int b = dir ? c - p.B : c;
    const int NQ = dir ? p.M : p.N;  // queries
    const int NC = dir ? p.N : p.M;  // candidates
    if (tile >= (dir ? p.tiles_y : p.tiles_x)) return;
    const float *__restrict__ qb = (dir ? p.y : p.x) + (size_t)b * NQ * DIM;
    const float *__restrict__ cb = (dir ? p.x : p.y) + (size_t)b * NC * DIM;

    const int tid = threadIdx.x;
    const int CH = p.chunk;
    const int CH4 = CH >> 2;
    const float4 *lds4 = reinterpret_cast<const float4 *>(lds);

    // ---- queries into registers (out-of-range lanes clamp to the last point) ---------------
    float q[R][DIM];
    int qi[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
        qi[r] = tile * (kThreads * R) + r * kThreads + tid;
        const int qc = qi[r] < NQ ? qi[r] : NQ - 1;
#pragma unroll
        for (int d = 0; d < DIM; ++d) q[r][d] = qb[(size_t)qc * DIM + d];
    }

    float best[R];
    int btile[R], bidx[R];
#pragma unroll
    for (int r = 0; r < R; ++r) { best[r] = INFINITY; btile[r] = -1; bidx[r] = 0; }

    for (int j0 = 0; j0 < NC; j0 += CH) {
        const int cnt = (NC - j0) < CH ? (NC - j0) : CH;
        const int cnt_pad = (cnt + kTile - 1) / kTile * kTile;
        if (j0 > 0) __syncthreads();
        // ---- stage chunk: AoS global stream -> SoA LDS (coalesced dword reads) -------------
        for (int e = tid; e < cnt * DIM; e += kThreads) {
            const float v = cb[(size_t)j0 * DIM + e];
            const int pt = e / DIM, cc = e - pt * DIM;
            lds[cc * CH + pt] = v;
        }
        for (int e = cnt + tid; e < cnt_pad; e += kThreads) {
#pragma unroll
            for (int d = 0; d < DIM; ++d) lds[d * CH + e] = INFINITY;
        }
        __syncthreads();

        const int ntile = cnt_pad / kTile;
        const int tile_base = j0 / kTile;  // CH is a multiple of kTile
        for (int t = 0; t < ntile; ++t) {
            float tm[R];
#pragma unroll
            for (int r = 0; r < R; ++r) tm[r] = INFINITY;
#pragma unroll
            for (int jj = 0; jj < kTile; jj += 4) {
                float4 cv[DIM];
#pragma unroll
                for (int d = 0; d < DIM; ++d)  // float4 units: CH % 32 == 0 => always ds_read_b128
                    cv[d] = lds4[d * CH4 + t * (kTile / 4) + jj / 4];
                float c0[DIM], c1[DIM], c2[DIM], c3[DIM];
#pragma unroll
                for (int d = 0; d < DIM; ++d) { c0[d] = cv[d].x; c1[d] = cv[d].y; c2[d] = cv[d].z; c3[d] = cv[d].w; }
#pragma unroll
                for (int r = 0; r < R; ++r) {
                    const float d0 = sqd<DIM>(q[r], c0), d1 = sqd<DIM>(q[r], c1);
                    const float d2 = sqd<DIM>(q[r], c2), d3 = sqd<DIM>(q[r], c3);
                    tm[r] = min3f(tm[r], d0, d1);
                    tm[r] = min3f(tm[r], d2, d3);
                }
            }
#pragma unroll
            for (int r = 0; r < R; ++r) {
                const bool better = tm[r] < best[r];  // strict: first tile holding the minimum
                best[r] = better ? tm[r] : best[r];
                btile[r] = better ? tile_base + t : btile[r];
            }
        }

        if (WANT_IDX) {
            // ---- exact argmin: re-scan the winning tile while its chunk is still in LDS ----
#pragma unroll
            for (int r = 0; r < R; ++r) {
                if (btile[r] >= tile_base) {  // improved within this chunk
                    const int off = (btile[r] - tile_base) * kTile;
                    float cur = INFINITY;
                    int ci = 0;
                    for (int jj = 0; jj < kTile; ++jj) {
                        float cc[DIM];
#pragma unroll
                        for (int d = 0; d < DIM; ++d) cc[d] = lds[d * CH + off + jj];
                        const float dd = sqd<DIM>(q[r], cc);
                        if (dd < cur) { cur = dd; ci = jj; }
                    }
                    bidx[r] = j0 + off + ci;
                }
            }
        }
    }

    // ---- outputs ------------------------------------------------------------------------------
    int32_t *idx_out = dir ? p.idx_y : p.idx_x;
    float *dmin_out = dir ? p.dmin_y : p.dmin_x;
    double acc = 0.0;
#pragma unroll
    for (int r = 0; r < R; ++r) {
        if (qi[r] < NQ) {
            // nothing below +Inf (overflowing or non-finite coordinates): min3 / `<` skipped every candidate
            if (!(best[r] < INFINITY)) nn1_scan_isless<DIM>(q[r], cb, NC, best[r], bidx[r]);
            if (WANT_IDX && idx_out) idx_out[(size_t)b * NQ + qi[r]] = bidx[r];
            if (dmin_out) dmin_out[(size_t)b * NQ + qi[r]] = best[r];
            acc += (double)best[r];
        }
    }
    if (p.partials) {
        __shared__ double sm[kThreads / 64];
        const double tot = block_sum<kThreads>(acc, sm);
        if (tid == 0) p.partials[(size_t)c * p.tiles + tile] = tot;
    }
}

// ------------------------------------------------------------------------------------------------
// nn1_tiny_kernel (D = 3, round 4): the exact loop for SMALL problems -- 2 B N M below a few ten million pair evaluations
// (C1, the reference harness's n <= 4096: benchmarks/metrics.jl:40) -- where nn1_f16_kernel's per-cloud statistics, image
// and 1024-thread blocks are all overhead (C1 17.6 us, n = 64: 13.7 us; an empty launch is ~6 us).  No statistics, no
// image, no filter, no LDS staging, no barrier before the arithmetic: a 256-thread block owns 16 R queries and ALL
// candidates of their cloud.  Lane l of wave w holds query l & 15 (+ 16 r) and works on candidate slice s = 4 w + (l >> 4)
// of 16 contiguous slices.  The slice is consumed in groups of 16 candidates: lane l LOADS candidate (l & 15) of the group
// (one 12-byte global load per lane and 16 pairs; consecutive lanes, consecutive points) and every lane of the 16-lane
// row reads it through the DPP row broadcast of the subtraction itself (v_subrev_f32_dpp row_newbcast:i: no move, no LDS):
// 8 VALU per pair for the oracle's unfused ((dx dx) + dy dy) + dz dz, 8 v_min3 per group of 16, 3 for (best, best group)
// with a strict `<`.  The winning group is re-scanned for the FIRST candidate that attains the minimum, so a lane's
// result is its slice's (distance, lowest index); the 16 slices of a query meet in a 64-bit LDS atomicMin on
// (distance bits << 32 | index) -- the oracle's order (isless, then the lower index; no NaN passes `<`, a query without
// any distance below +Inf takes nn1_scan_isless).  Loss: per-block Float64 partial + nn1_f16_kernel's fused finalisation.

template <int I>
__device__ __forceinline__ float row_bcast(float v) {  // lane (l & ~15) + I of every 16-lane row, read by the consuming instruction's DPP operand
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x150 + I, 0xF, 0xF, false));
}
template <int I>
__device__ __forceinline__ float tiny_d(const float (&q)[3], float cx, float cy, float cz) {
    const float t0 = q[0] - row_bcast<I>(cx), t1 = q[1] - row_bcast<I>(cy), t2 = q[2] - row_bcast<I>(cz);
    return ((t0 * t0) + (t1 * t1)) + (t2 * t2);
}
__device__ __forceinline__ void tiny_group(const float (&q)[3], float cx, float cy, float cz, float (&d)[kTyG]) {
    d[0] = tiny_d<0>(q, cx, cy, cz); d[1] = tiny_d<1>(q, cx, cy, cz); d[2] = tiny_d<2>(q, cx, cy, cz); d[3] = tiny_d<3>(q, cx, cy, cz);
    d[4] = tiny_d<4>(q, cx, cy, cz); d[5] = tiny_d<5>(q, cx, cy, cz); d[6] = tiny_d<6>(q, cx, cy, cz); d[7] = tiny_d<7>(q, cx, cy, cz);
    d[8] = tiny_d<8>(q, cx, cy, cz); d[9] = tiny_d<9>(q, cx, cy, cz); d[10] = tiny_d<10>(q, cx, cy, cz); d[11] = tiny_d<11>(q, cx, cy, cz);
    d[12] = tiny_d<12>(q, cx, cy, cz); d[13] = tiny_d<13>(q, cx, cy, cz); d[14] = tiny_d<14>(q, cx, cy, cz); d[15] = tiny_d<15>(q, cx, cy, cz);
}

// kTyPF = groups in flight per lane (4; 1 for clouds of <= 256 candidates: a quarter of the code -- the smallest launches are
// eight blocks on eight cold instruction caches).
template <int R, int kTyPF, bool WANT_IDX>
__global__ __launch_bounds__(kTyThreads) void nn1_tiny_kernel(Nn1Params p) {
    __shared__ unsigned long long slot[2][kTyQ * R];
    const int tiles = p.tiles;
    const int c = blockIdx.x / tiles, btile = blockIdx.x - c * tiles;   // cloud id in [0, 2B): dir = c / B
    const int dir = c >= p.B ? 1 : 0;
    const int b = dir ? c - p.B : c;
    const int NQ = dir ? p.M : p.N, NC = dir ? p.N : p.M;
    if (btile >= (dir ? p.tiles_y : p.tiles_x)) return;
    const float *__restrict__ qb = (dir ? p.y : p.x) + (size_t)b * NQ * 3;
    const float *__restrict__ cb = (dir ? p.x : p.y) + (size_t)b * NC * 3;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int ql = lane & 15, s = wave * 4 + (lane >> 4);
    // slice s = candidates [s L, (s + 1) L), L a multiple of 16; this lane loads candidate jl + 16 g of group g
    const int L = ((NC + kTySl - 1) / kTySl + kTyG - 1) / kTyG * kTyG;
    const int ngroups = L / kTyG;
    const int jl = s * L + ql;
    auto load_group = [&](int g, float &cx, float &cy, float &cz) {
        const int j = jl + kTyG * g;
        const bool ok = g < ngroups && j < NC;
        const P3 t = *reinterpret_cast<const P3 *>(cb + 3ll * (ok ? j : 0));
        cx = ok ? t.x : INFINITY; cy = ok ? t.y : INFINITY; cz = ok ? t.z : INFINITY;   // padding at +Inf: never below anything
    };
    float cur[kTyPF][3], nxt[kTyPF][3];
#pragma unroll
    for (int u = 0; u < kTyPF; ++u) load_group(u, cur[u][0], cur[u][1], cur[u][2]);
    const bool resident = ngroups <= kTyPF;   // the lane's share of the cloud stays in registers across the block's query tiles
    if (tid < 2 * kTyQ * R) (&slot[0][0])[tid] = ~0ull;
    __syncthreads();

    // a block takes p.tpb consecutive query tiles of its cloud (one partial sum, one arrival at the ticket per BLOCK: with a
    // block per tile the 1024+ same-address atomics and the last arriver's pass over as many partials were the launch's tail)
    const int raw_tiles = (NQ + kTyQ * R - 1) / (kTyQ * R);
    int32_t *idx_out = dir ? p.idx_y : p.idx_x;
    float *dmin_out = dir ? p.dmin_y : p.dmin_x;
    double acc = 0.0;
    auto load_queries = [&](int tile, float (&qq)[R][3]) {
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const int qi = tile * (kTyQ * R) + r * kTyQ + ql;
            const P3 t = *reinterpret_cast<const P3 *>(qb + 3ll * (qi < NQ ? qi : NQ - 1));
            qq[r][0] = t.x; qq[r][1] = t.y; qq[r][2] = t.z;
        }
    };
    float qn[R][3];
    load_queries(btile * p.tpb, qn);
    for (int tt = 0; tt < p.tpb; ++tt) {
        const int tile = btile * p.tpb + tt;
        if (tile >= raw_tiles) break;   // (block-uniform)
        float q[R][3];
#pragma unroll
        for (int r = 0; r < R; ++r) { q[r][0] = qn[r][0]; q[r][1] = qn[r][1]; q[r][2] = qn[r][2]; }
        if (tt + 1 < p.tpb) load_queries(tile + 1, qn);   // the next tile's queries travel while this one is evaluated
        if (!resident && tt > 0) {
#pragma unroll
            for (int u = 0; u < kTyPF; ++u) load_group(u, cur[u][0], cur[u][1], cur[u][2]);
        }
        float best[R];
        int bg[R];
#pragma unroll
        for (int r = 0; r < R; ++r) { best[r] = INFINITY; bg[r] = 0; }
        for (int g0 = 0; g0 < ngroups; g0 += kTyPF) {
            if (g0 + kTyPF < ngroups) {
#pragma unroll
                for (int u = 0; u < kTyPF; ++u) load_group(g0 + kTyPF + u, nxt[u][0], nxt[u][1], nxt[u][2]);
            }
#pragma unroll
            for (int u = 0; u < kTyPF; ++u) {
#pragma unroll
                for (int r = 0; r < R; ++r) {
                    float d[kTyG];
                    tiny_group(q[r], cur[u][0], cur[u][1], cur[u][2], d);
                    float m = min3f(d[0], d[1], d[2]);
                    m = min3f(m, d[3], d[4]);
                    m = min3f(m, d[5], d[6]);
                    m = min3f(m, d[7], d[8]);
                    m = min3f(m, d[9], d[10]);
                    m = min3f(m, d[11], d[12]);
                    m = min3f(m, d[13], d[14]);
                    m = __builtin_fminf(m, d[15]);
                    const bool better = m < best[r];  // strict: the first group that holds the lane's minimum
                    best[r] = better ? m : best[r];
                    if (WANT_IDX) bg[r] = better ? g0 + u : bg[r];
                }
            }
            if (g0 + kTyPF < ngroups) {
#pragma unroll
                for (int u = 0; u < kTyPF; ++u) { cur[u][0] = nxt[u][0]; cur[u][1] = nxt[u][1]; cur[u][2] = nxt[u][2]; }
            }
        }
        unsigned long long *sl = slot[tt & 1];
#pragma unroll
        for (int r = 0; r < R; ++r) {
            int bi = 0;
            if (WANT_IDX) {
                // the FIRST candidate of the lane's winning group that attains the minimum.  The winning groups differ lane by
                // lane, so every lane reads the 16 candidates of its own (16 loads in flight, L1 / L2 hits)
                float d[kTyG];
#pragma unroll
                for (int i = 0; i < kTyG; ++i) {
                    const int j = s * L + kTyG * bg[r] + i;
                    const P3 t = *reinterpret_cast<const P3 *>(cb + 3ll * (j < NC ? j : 0));
                    const float t0 = q[r][0] - t.x, t1 = q[r][1] - t.y, t2 = q[r][2] - t.z;
                    d[i] = j < NC ? ((t0 * t0) + (t1 * t1)) + (t2 * t2) : INFINITY;
                }
#pragma unroll
                for (int i = kTyG - 1; i >= 0; --i)
                    if (d[i] == best[r]) bi = s * L + kTyG * bg[r] + i;
            }
            if (best[r] < INFINITY)
                atomicMin(&sl[r * kTyQ + ql], ((unsigned long long)__builtin_bit_cast(unsigned int, best[r]) << 32) | (unsigned int)bi);
        }
        __syncthreads();
        // the first wave writes the tile's results (16 R <= 32 queries) and returns the slots to "empty"; the other buffer
        // takes the next tile's minima meanwhile (this buffer is used again two tiles on, behind the next barrier)
        const int qidx = tile * (kTyQ * R) + tid;
        if (tid < kTyQ * R) {
            const unsigned long long k = sl[tid];
            sl[tid] = ~0ull;
            if (qidx < NQ) {
                float dd = __builtin_bit_cast(float, (unsigned int)(k >> 32));
                int ii = (int)(unsigned int)k;
                if (k == ~0ull) {  // nothing below +Inf (non-finite or overflowing coordinates): the exact scan in isless order
                    const P3 t = *reinterpret_cast<const P3 *>(qb + 3ll * qidx);
                    const float qq[3] = {t.x, t.y, t.z};
                    nn1_scan_isless<3>(qq, cb, NC, dd, ii);
                }
                if (WANT_IDX && idx_out) idx_out[(size_t)b * NQ + qidx] = ii;
                if (dmin_out) dmin_out[(size_t)b * NQ + qidx] = dd;
                acc += (double)dd;
            }
        }
    }
    if (tid >= 64 || !p.partials) return;
    const double tot = __shfl(wave_sum_l63_f64(acc), 63);   // fixed order: deterministic
    if (!p.ticket) {
        if (tid == 0) p.partials[(size_t)c * tiles + btile] = tot;
        return;
    }
    const FinalizeArgs fa{reinterpret_cast<unsigned long long *>(p.partials), p.ticket, p.nvalid, p.B, tiles, p.tiles_x, p.tiles_y,
                          p.sums_out, p.loss_out, p.N, p.M, p.Bg, p.w1, p.w2};
    (void)fused_finalize_wave0(fa, (size_t)c * tiles + btile, tot, tid);
}

// Generic dimension (D == 1 or D > 3): one thread per query, candidates read through L1/L2.
// Correct for any D; not the tuned path (the chamfer configs are all D = 3).
// 1-D grid of p.tiles blocks per cloud: 2B clouds on the grid's y dimension would stop at maxGridSize[1] = 65536
// (B = 32768), which check_shapes does not bound.
__global__ __launch_bounds__(kThreads) void nn1_generic_kernel(Nn1Params p, int D) {
    const int c = blockIdx.x / p.tiles;
    const int dir = c >= p.B ? 1 : 0;
    const int b = dir ? c - p.B : c;
    const int NQ = dir ? p.M : p.N, NC = dir ? p.N : p.M;
    const int tile = blockIdx.x - c * p.tiles;
    const float *__restrict__ qb = (dir ? p.y : p.x) + (size_t)b * NQ * D;
    const float *__restrict__ cb = (dir ? p.x : p.y) + (size_t)b * NC * D;
    const int i = tile * kThreads + threadIdx.x;
    double acc = 0.0;
    if (i < NQ) {
        float best = 0.0f;
        int bi = 0;
        const float *a = qb + (size_t)i * D;
        for (int j = 0; j < NC; ++j) {
            const float *cc = cb + (size_t)j * D;
            float s = 0.0f;
            for (int d = 0; d < D; ++d) { float t = a[d] - cc[d]; s = s + t * t; }
            if (j == 0 || fless(s, best)) { best = s; bi = j; }
        }
        int32_t *idx_out = dir ? p.idx_y : p.idx_x;
        float *dmin_out = dir ? p.dmin_y : p.dmin_x;
        if (idx_out) idx_out[(size_t)b * NQ + i] = bi;
        if (dmin_out) dmin_out[(size_t)b * NQ + i] = best;
        acc = (double)best;
    }
    if (p.partials) {
        __shared__ double sm[kThreads / 64];
        const double tot = block_sum<kThreads>(acc, sm);
        // blocks past this direction's tile count still write (zero) so the reduce is uniform
        if (threadIdx.x == 0) p.partials[(size_t)c * p.tiles + tile] = tot;
    }
}

}  // namespace

namespace fx3d {

template <int DIM, bool WANT_IDX>
static void launch_small_d(const Nn1Params &p, int R, int grid, size_t lds_bytes, hipStream_t st) {
    switch (R) {
        case 4:
            hipLaunchKernelGGL((nn1_small_d_kernel<DIM, 4, WANT_IDX>), dim3(grid), dim3(kThreads), lds_bytes, st, p);
            break;
        case 2:
            hipLaunchKernelGGL((nn1_small_d_kernel<DIM, 2, WANT_IDX>), dim3(grid), dim3(kThreads), lds_bytes, st, p);
            break;
        default:
            hipLaunchKernelGGL((nn1_small_d_kernel<DIM, 1, WANT_IDX>), dim3(grid), dim3(kThreads), lds_bytes, st, p);
            break;
    }
}

template <bool WANT_IDX>
static void launch_tiny(const Nn1Params &p, int R, int grid, hipStream_t st) {
    const bool small = (p.N > p.M ? p.N : p.M) <= kTySl * kTyG;   // both directions' candidates are one group per slice
    if (R == 2 && small) hipLaunchKernelGGL((nn1_tiny_kernel<2, 1, WANT_IDX>), dim3(grid), dim3(kTyThreads), 0, st, p);
    else if (R == 2) hipLaunchKernelGGL((nn1_tiny_kernel<2, 4, WANT_IDX>), dim3(grid), dim3(kTyThreads), 0, st, p);
    else if (small) hipLaunchKernelGGL((nn1_tiny_kernel<1, 1, WANT_IDX>), dim3(grid), dim3(kTyThreads), 0, st, p);
    else hipLaunchKernelGGL((nn1_tiny_kernel<1, 4, WANT_IDX>), dim3(grid), dim3(kTyThreads), 0, st, p);
}

fx3d_status nn1_exact_launch(Nn1Kernel k, const Nn1Params &p, int D, int R, int grid, size_t lds_bytes, hipStream_t st) {
    const bool want_idx = p.idx_x || p.idx_y;
    if (k == NN1_TINY) {  // (D = 3)
        want_idx ? launch_tiny<true>(p, R, grid, st) : launch_tiny<false>(p, R, grid, st);
    } else if (k == NN1_SMALL_D && D == 3) {
        want_idx ? launch_small_d<3, true>(p, R, grid, lds_bytes, st) : launch_small_d<3, false>(p, R, grid, lds_bytes, st);
    } else if (k == NN1_SMALL_D) {  // (D = 2)
        want_idx ? launch_small_d<2, true>(p, R, grid, lds_bytes, st) : launch_small_d<2, false>(p, R, grid, lds_bytes, st);
    } else {
        hipLaunchKernelGGL(nn1_generic_kernel, dim3(grid), dim3(kThreads), 0, st, p, D);
    }
    FX3D_LAUNCH_CHECK();
    return FX3D_OK;
}

}  // namespace fx3d
