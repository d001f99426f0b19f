// Adjoint of _chamfer_distance (Zygote through src/metrics/pcloud.jl:45-48 with the nearest-neighbour indices constant, :45
// `@ignore`), of chamfer_distance(m1::TriMesh, m2::TriMesh, n) (src/metrics/mesh.jl:34-44) w.r.t. the meshes' vertices, and the
// value-and-gradient entry point (benchmarks/metrics.jl:24-38 "total", examples/fit_mesh.jl:106-110).
//
// Round 5: NO float atomics on the default path.  The gradient row of point i of one side is
//     side x:  g[i] = (0 + ca (x_i - y[ix[i]]))  -  sum over { j : iy[j] == i }, j ASCENDING, of  cb (y_j - x_i)
//     side y:  g[j] = (0 - sum over { i : ix[i] == j }, i ASCENDING, of ca (x_i - y_j))  +  cb (y_j - x[iy[j]])
// -- exactly the order in which oracle/flux3d_oracle.c: fx3d_oracle_chamfer_bwd (two loops per batch element) reaches the
// row, so the result is the oracle's bit for bit and the same from run to run.  A block owns up to 4096 rows of one
// (cloud, side); per round of 4096 rows of the OTHER side it builds the inverse lists in LDS with a counting sort of their
// indices (integer LDS atomics only: counts, a block scan, cursor placement), puts every list into ascending order (up to eight
// entries: a sorting network in the owner's registers; longer ones: a wave sorts the list in place through a 4096-bit bitmap
// and walks it with lane-parallel gathers and an ordered readlane chain), and the owner of a row subtracts its entries in
// order.  D = 3: accumulators in registers, 12-byte row loads; other D: the row of g itself is the accumulator.
#include <algorithm>
#include <type_traits>

#include "fx3d_common.h"
#include "mesh_host.h"
#include "sample_gather.h"
#include "mesh_reg.h"

using namespace fx3d;

namespace {

constexpr int kThreads = 256;

// Scatter form with GLOBAL float atomics (option bwd_global_atomics; arrival order decides the last bit), two ordered passes:
//   own pass     : gx[i] = ca (x_i - y[ix[i]]),  gy[j] = cb (y_j - x[iy[j]])        plain coalesced stores
//   scatter pass : gy[ix[i]] -= ca (x_i - y[ix[i]]),  gx[iy[j]] -= cb (y_j - x[iy[j]])   float atomics
template <bool SCATTER>
__global__ __launch_bounds__(kThreads) void chamfer_bwd_kernel(
    const float *__restrict__ x, int N, const float *__restrict__ y, int M, int B, int D,
    const int32_t *__restrict__ idx_x, const int32_t *__restrict__ idx_y, float ca, float cb,
    float *gx, float *gy) {
    const long long total = (long long)B * (N + M);
    for (long long k = (long long)blockIdx.x * kThreads + threadIdx.x; k < total;
         k += (long long)gridDim.x * kThreads) {
        const int b = (int)(k / (N + M));
        const int r = (int)(k % (N + M));
        const float *xb = x + (size_t)b * N * D, *yb = y + (size_t)b * M * D;
        float *gxb = gx + (size_t)b * N * D, *gyb = gy + (size_t)b * M * D;
        if (r < N) {
            const int i = r, j = idx_x[(size_t)b * N + i];
            for (int d = 0; d < D; ++d) {
                const float t = ca * (xb[(size_t)i * D + d] - yb[(size_t)j * D + d]);
                if (SCATTER) atomicAdd(&gyb[(size_t)j * D + d], -t);
                else gxb[(size_t)i * D + d] = t;
            }
        } else {
            const int j = r - N, i = idx_y[(size_t)b * M + j];
            for (int d = 0; d < D; ++d) {
                const float t = cb * (yb[(size_t)j * D + d] - xb[(size_t)i * D + d]);
                if (SCATTER) atomicAdd(&gxb[(size_t)i * D + d], -t);
                else gyb[(size_t)j * D + d] = t;
            }
        }
    }
}

// ---- the gather form ---------------------------------------------------------------------------------------------------------
constexpr int kBgThreads = 1024;
constexpr int kBgRows = 4096;    // rows of g one block owns at most
constexpr int kBgPer = kBgRows / kBgThreads;  // rows / scan slots / other-side rows per thread and round
constexpr int kBgChunk = 4096;   // rows of the other side bucketed per round (their round-local ids fit 16 bits)
constexpr int kBgSmall = 8;      // lists up to this length are ordered in the owner's registers (one in 10^6 of uniform data's is longer)
constexpr int kBgSortWaves = kBgThreads / 64;  // every wave takes rows with longer lists (one 4096-bit bitmap each)
constexpr int kBgBigW = 256;     // long rows whose own point and index travel through LDS (the others re-read them from memory)
constexpr int kBgOcc = 4;  // waves per SIMD the kernels are compiled for.  4 = one 1024-thread block per CU with up to 128 registers; 8 (two
                           // blocks per CU, 64 registers) spills and measured 41 - 51 us against 37 at B = 256 x 4096 in every form tried
static_assert(kBgPer == 4, "the pins in bg_load_rows and bg_read_indices name four values each");
static_assert(kBgThreads == sg::kSgThreads, "row blocks and table blocks share a launch");

#ifdef FX3D_BG_PROBE   // phase stamps of every block (s_memtime, 100 MHz) for tools/chamfer_bwd_probe.py; never in the shipped build
__device__ unsigned long long g_bg_probe[1024 * 8];
#define BG_STAMP(n) do { if (threadIdx.x == 0 && blockIdx.x < 1024) g_bg_probe[blockIdx.x * 8 + (n)] = __builtin_readcyclecounter(); } while (0)
#else
#define BG_STAMP(n) do { } while (0)
#endif

// 38 KB
struct BgLds {
    unsigned int cnt2[kBgRows / 2];     // entries of own row lr in this round, two 16-bit counters per word (<= 4096 each):
                                        // counted up, then counted DOWN by the placement -- zero again for the next round
    unsigned short start[kBgRows + 4];  // first list slot of row lr; start[lr + 1] - start[lr] = its length
    unsigned short list[kBgChunk];      // round-local ids of the other side's rows, list by list
    unsigned int bitmap[kBgSortWaves][kBgChunk / 32];   // in-place ordering of a long list
    unsigned short big[kBgChunk / (kBgSmall + 1) + 1];  // rows with long lists (more cannot exist in one round)
    float4 bigw[kBgBigW];                               // D = 3: (own point, index of its neighbour as bits) of the first long rows
    __attribute__((aligned(16))) unsigned int wsum[kBgThreads / 64];
    unsigned int nbig;
};

__device__ __forceinline__ void ce(unsigned int &a, unsigned int &b) {
    const unsigned int lo = a < b ? a : b, hi = a < b ? b : a;
    a = lo; b = hi;
}
// all LDS traffic this wave issued so far is complete and visible to its other lanes
__device__ __forceinline__ void wave_lds_sync() {
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
    __builtin_amdgcn_wave_barrier();
}
// inclusive wave64 prefix sum on the VALU (DPP row shifts + row broadcasts; __shfl_up would be six ds_bpermute round trips)
template <int CTRL, int ROWMASK>
__device__ __forceinline__ unsigned int dpp_zero(unsigned int v) {  // lanes without a source / outside ROWMASK read 0
    return (unsigned int)__builtin_amdgcn_update_dpp(0, (int)v, CTRL, ROWMASK, 0xF, false);
}
__device__ __forceinline__ unsigned int wave_scan_incl(unsigned int v) {
    v += dpp_zero<0x111, 0xF>(v);  // row_shr:1
    v += dpp_zero<0x112, 0xF>(v);  // row_shr:2
    v += dpp_zero<0x114, 0xF>(v);  // row_shr:4
    v += dpp_zero<0x118, 0xF>(v);  // row_shr:8
    v += dpp_zero<0x142, 0xA>(v);  // row_bcast:15 -> rows 1, 3
    v += dpp_zero<0x143, 0xC>(v);  // row_bcast:31 -> rows 2, 3
    return v;
}
__device__ __forceinline__ float lane_val(float v, int l) {
    return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), l));
}
__device__ __forceinline__ P3 lane_val(P3 v, int l) { return P3{lane_val(v.x, l), lane_val(v.y, l), lane_val(v.z, l)}; }

// One side of a sampled adjoint: its mesh, the draws of its samples, where the gradient w.r.t. its vertices goes
struct SampledSide {
    const int32_t *faces;     // (3, Fmax, B) mesh-local
    const int32_t *face_idx;  // (n, B) the draws
    const float *r1, *r2;
    float *gverts;            // (3, Vmax, B), added to; nullptr: no gradient w.r.t. this side's mesh
    int Vmax, Fmax;
    const int32_t *vf_rowptr, *vf_ent;  // the vertex -> face table of the ordered form (the host picks the form by it; no kernel here reads it)
    bool complete() const { return faces && face_idx && r1 && r2 && Vmax > 0 && Fmax > 0; }  // (host: what a side with gverts must bring)
};

struct BgJob {
    const float *own, *oth;               // this side's rows (R x D) / the other side's (S x D) of one cloud pair
    const int32_t *idx_own, *idx_oth;     // own row -> other row / other row -> own row
    int R, S, D, r0, r1, side, b;         // the block owns rows [r0, r1) of side `side` (0: x, 1: y) of cloud pair b
    float c_own, c_oth;
    float *g;                             // MODE 0 / 1: this (cloud, side)'s gradient rows (R x D): result, and the accumulator
                                          // between the rounds of an other side beyond kBgChunk rows
    P3 *part;                             // MODE 2: the accumulator between rounds, in LDS
    SampledSide smp;                      // MODE 2: where a finished row goes
};

// MODE 2: row i of the gradient w.r.t. the sampled points -> the three vertices of sample i's face with the barycentric
// weights of its draw (sample_bwd_kernel's arithmetic, src/transforms/mesh_func.jl:64-75); a face is drawn many times: float atomics
__device__ __forceinline__ void bg_scatter_sample(const BgJob &J, int i, P3 a) {
    const SampledSide &S = J.smp;
    const size_t k = (size_t)J.b * J.R + i;
    const int32_t *fc = S.faces + ((size_t)J.b * S.Fmax + S.face_idx[k]) * 3;
    const int f3[3] = {fc[0], fc[1], fc[2]};
    const float uu = sqrtf(S.r1[k]), v = S.r2[k];
    const float wt[3] = {1.0f - uu, uu * (1.0f - v), uu * v};
    const float gr[3] = {a.x, a.y, a.z};
    float *gb = S.gverts + (size_t)J.b * S.Vmax * 3;
#pragma unroll
    for (int t = 0; t < 3; ++t)
#pragma unroll
        for (int d = 0; d < 3; ++d) atomicAdd(&gb[3ll * f3[t] + d], wt[t] * gr[d]);
}

// ---- a block's rows: bg_rows<MODE> and its phases -------------------------------------------------------------------------------------
// MODE 0: D = 3, rows stored to g;  1: any D, rows accumulated in g (no LDS image: gathers from L2);  2: D = 3, rows scattered
// onto the sampled faces' vertices.

// What a thread carries from phase to phase.  (Plain scalar arrays: an array of the packed 12-byte P3 is not promoted to registers -- it
// lived in scratch.)
struct BgThread {
    int tid, lane, wv, nrows, rpt;
    int jown[kBgPer];                              // my rows (tid + u * kBgThreads): the other side's row of their own term,
    float wx[kBgPer], wy[kBgPer], wz[kBgPer];      // D = 3: the rows themselves
    float ojx[kBgPer], ojy[kBgPer], ojz[kBgPer];   // D = 3: and the rows jown names
    int il[kBgPer];                                // this round: which of the block's rows the other side's row tid + v * kBgThreads points at (or none)
};
// One round: rows [c0, c0 + cn) of the other side.  WHEN A ROW'S OWN TERM IS ADDED is decided here and nowhere else -- side x: it
// opens the row (the oracle's first loop), side y: it closes it.
struct BgRound {
    int c0, cn;
    bool first, last, own_first;
    __device__ __forceinline__ bool own_opens() const { return first && own_first; }
    __device__ __forceinline__ bool own_closes() const { return last && !own_first; }
};
__device__ __forceinline__ BgRound bg_round(const BgJob &J, int c0) {
    return BgRound{c0, J.S - c0 < kBgChunk ? J.S - c0 : kBgChunk, c0 == 0, c0 + kBgChunk >= J.S, J.side == 0};
}

// ---- one row's sum: the one statement of it, for the long rows of phase (4) and the owners of phase (5) ---------------------------------
// V is what one sum runs over: the whole row (D = 3: three registers) or one coordinate of it (other D: the caller loops over d).
// The arithmetic reads the same in both forms (never contracted: -ffp-contract=off).
__device__ __forceinline__ P3 operator+(P3 a, P3 b) { return P3{a.x + b.x, a.y + b.y, a.z + b.z}; }
__device__ __forceinline__ P3 operator-(P3 a, P3 b) { return P3{a.x - b.x, a.y - b.y, a.z - b.z}; }
__device__ __forceinline__ P3 operator*(float c, P3 a) { return P3{c * a.x, c * a.y, c * a.z}; }

template <int MODE>
struct BgAcc {
    using V = std::conditional_t<MODE == 1, float, P3>;
    V a;
    V *home;  // WHERE THE SUM LIVES BETWEEN ROUNDS, decided here and nowhere else: the row of g itself, or (MODE 2, which has no g) J.part in LDS
    __device__ __forceinline__ BgAcc(const BgJob &J, int lr, int d) {
        const size_t i = (size_t)(J.r0 + lr);
        if constexpr (MODE == 2) home = J.part + lr;  // (one round: J.part has no bytes behind it -- and open / finish never follow it)
        else if constexpr (MODE == 0) home = reinterpret_cast<P3 *>(J.g + i * 3);
        else home = J.g + i * J.D + d;
    }
    // row r of p (D = 3), coordinate d of it (other D)
    static __device__ __forceinline__ V row(const float *p, size_t r, int D, int d) {
        if constexpr (MODE == 1) return p[r * D + d];
        else return *reinterpret_cast<const P3 *>(p + r * 3);
    }
    // ot: the own term, c_own * (w - o)
    __device__ __forceinline__ void open(const BgRound &R, V ot) {
        if (!R.first) a = *home;
        else if (R.own_opens()) a = V{} + ot;  // (0 + ot, as the oracle has it: an own term of -0 gives +0)
        else a = V{};
    }
    __device__ __forceinline__ void sub(V t) { a = a - t; }  // t: c_oth * (o - w), one call per entry, entries ascending
    __device__ __forceinline__ void close(const BgRound &R, V ot) { if (R.own_closes()) a = a + ot; }
    __device__ __forceinline__ void finish(const BgJob &J, const BgRound &R, int lr) {
        if constexpr (MODE == 2) if (R.last) return bg_scatter_sample(J, J.r0 + lr, a);
        *home = a;
    }
};

// ---- the phases ---------------------------------------------------------------------------------------------------------------------------
// requested before anything else: this thread's rows and their indices, then the own term's rows of the other side
template <int MODE>
__device__ __forceinline__ void bg_load_rows(const BgJob &J, BgThread &T) {
    constexpr bool D3 = MODE != 1;
    T.tid = threadIdx.x; T.lane = T.tid & 63;
    T.wv = __builtin_amdgcn_readfirstlane(T.tid >> 6);  // (scalar: the long-row loop and its readlane chain must not be "divergent")
    T.nrows = J.r1 - J.r0;
    T.rpt = (T.nrows + kBgThreads - 1) / kBgThreads;  // 1 .. 4 rows per thread, kBgThreads apart: a wave's rows are contiguous
                                                      // (12-byte loads / stores of consecutive lanes coalesce; 48 bytes apart they are 64 transactions)
#pragma unroll
    for (int u = 0; u < kBgPer; ++u) {
        const bool mine = u < T.rpt && T.tid + u * kBgThreads < T.nrows;
        T.jown[u] = mine ? J.idx_own[J.r0 + T.tid + u * kBgThreads] : 0;
        T.wx[u] = 0.0f; T.wy[u] = 0.0f; T.wz[u] = 0.0f;
        if (D3 && mine) {
            const P3 t = *reinterpret_cast<const P3 *>(J.own + (size_t)(J.r0 + T.tid + u * kBgThreads) * 3);
            T.wx[u] = t.x; T.wy[u] = t.y; T.wz[u] = t.z;
        }
    }
    // (round 6) the own term's rows of the other side, requested as soon as the indices are here and consumed in phase (5): the request
    // used to sit inside phase (5)'s per-row branch with a full wait behind it -- one more dependent trip to the L2 per row.
    // UNCONDITIONAL loads throughout these phases (a thread without a row reads row 0): `cond ? load : 0` compiles to a branch
    // around the load and `s_waitcnt vmcnt(0)` behind it, i.e. the loads of a group leave one after the other.
    // (The pin, as in bg_read_indices: without it the optimiser moves each index's `* 12` into the branch of its `mine` select, with a
    //  wait for that index behind it -- four dependent trips instead of one; seen in the ISA, +0.3 us at B = 32 x 4096.)
    asm volatile("" : "+v"(T.jown[0]), "+v"(T.jown[1]), "+v"(T.jown[2]), "+v"(T.jown[3]));
#pragma unroll
    for (int u = 0; u < kBgPer; ++u) {
        T.ojx[u] = 0.0f; T.ojy[u] = 0.0f; T.ojz[u] = 0.0f;
        if (D3) {
            const P3 t = *reinterpret_cast<const P3 *>(J.oth + (size_t)T.jown[u] * 3);
            T.ojx[u] = t.x; T.ojy[u] = t.y; T.ojz[u] = t.z;
        }
    }
}

// (1) this round's indices of the other side: which of my block's rows does other row c0 + jl point at
__device__ __forceinline__ void bg_read_indices(BgLds &L, const BgJob &J, const BgRound &R, BgThread &T) {
    if (T.tid == 0) L.nbig = 0u;
#pragma unroll
    for (int v = 0; v < kBgPer; ++v) {
        const int jl = T.tid + v * kBgThreads;
        T.il[v] = J.idx_oth[R.c0 + (jl < R.cn ? jl : 0)];
    }
    // (an empty asm that names all four: the optimiser otherwise sinks every load back into the branch of its `jl < cn` select,
    //  with a full wait behind it -- four dependent trips to memory instead of one)
    asm volatile("" : "+v"(T.il[0]), "+v"(T.il[1]), "+v"(T.il[2]), "+v"(T.il[3]));
#pragma unroll
    for (int v = 0; v < kBgPer; ++v) T.il[v] = T.tid + v * kBgThreads < R.cn ? T.il[v] - J.r0 : -1;
}

__device__ __forceinline__ void bg_count(BgLds &L, const BgThread &T) {
#pragma unroll
    for (int v = 0; v < kBgPer; ++v)
        if ((unsigned int)T.il[v] < (unsigned int)T.nrows) atomicAdd(&L.cnt2[T.il[v] >> 1], (T.il[v] & 1) ? 0x10000u : 1u);
}

// (2) exclusive scan of the counts over the rows (thread t: slots 4t .. 4t+3) -> start[]; one barrier inside, behind the waves' sums
__device__ __forceinline__ void bg_scan(BgLds &L, const BgThread &T) {
    unsigned int cc[kBgPer], s4 = 0u;
#pragma unroll
    for (int q = 0; q < kBgPer / 2; ++q) {
        const unsigned int cw = L.cnt2[kBgPer / 2 * T.tid + q];
        cc[2 * q] = cw & 0xFFFFu; cc[2 * q + 1] = cw >> 16;
        s4 += cc[2 * q] + cc[2 * q + 1];
    }
    const unsigned int inc = wave_scan_incl(s4);
    if (T.lane == 63) L.wsum[T.wv] = inc;
    __syncthreads();
    unsigned int base = 0u;
#pragma unroll
    for (int q = 0; q < kBgThreads / 64; q += 4) {
        const uint4 t = *reinterpret_cast<const uint4 *>(&L.wsum[q]);
        base += (q < T.wv ? t.x : 0u) + (q + 1 < T.wv ? t.y : 0u) + (q + 2 < T.wv ? t.z : 0u) + (q + 3 < T.wv ? t.w : 0u);
    }
    unsigned int ex = base + inc - s4;
#pragma unroll
    for (int q = 0; q < kBgPer / 2; ++q) {
        const unsigned int lo = ex, hi = ex + cc[2 * q];
        *reinterpret_cast<unsigned int *>(&L.start[kBgPer * T.tid + 2 * q]) = lo | (hi << 16);
        ex = hi + cc[2 * q + 1];
    }
    if (T.tid == kBgThreads - 1) L.start[kBgRows] = (unsigned short)ex;
}

// (3) placement, from the back of every list (arrival order inside a list: whatever the atomics give; put right in (4) and (5));
//     the owners register their rows with long lists and hand the waves what they hold of them
template <int MODE>
__device__ __forceinline__ void bg_place(BgLds &L, const BgThread &T) {
    constexpr bool D3 = MODE != 1;
#pragma unroll
    for (int v = 0; v < kBgPer; ++v)
        if ((unsigned int)T.il[v] < (unsigned int)T.nrows) {
            const int sh = (T.il[v] & 1) * 16;
            const unsigned int old = atomicSub(&L.cnt2[T.il[v] >> 1], 1u << sh);
            L.list[L.start[T.il[v]] + ((old >> sh) & 0xFFFFu) - 1u] = (unsigned short)(T.tid + v * kBgThreads);
        }
#pragma unroll
    for (int u = 0; u < kBgPer; ++u) {
        const int lr = T.tid + u * kBgThreads;
        if (u < T.rpt && lr < T.nrows && (int)L.start[lr + 1] - (int)L.start[lr] > kBgSmall) {
            const unsigned int k = atomicAdd(&L.nbig, 1u);
            L.big[k] = (unsigned short)lr;
            if (D3 && k < (unsigned int)kBgBigW) L.bigw[k] = float4{T.wx[u], T.wy[u], T.wz[u], __builtin_bit_cast(float, T.jown[u])};
        }
    }
}

// (4) rows with long lists: one wave each -- bitmap sort in place, lane-parallel gathers, an ordered readlane chain
template <int MODE>
__device__ __forceinline__ void bg_long_rows(BgLds &L, const BgJob &J, const BgRound &R, const BgThread &T) {
    constexpr bool D3 = MODE != 1;
    using V = typename BgAcc<MODE>::V;
    const unsigned int nb = (unsigned int)__builtin_amdgcn_readfirstlane((int)L.nbig);
    for (unsigned int k = (unsigned int)T.wv; k < nb; k += kBgSortWaves) {
        const int lr = __builtin_amdgcn_readfirstlane((int)L.big[k]);
        const int start = __builtin_amdgcn_readfirstlane((int)L.start[lr]);
        const int c = __builtin_amdgcn_readfirstlane((int)L.start[lr + 1]) - start;
        unsigned int *bm = L.bitmap[T.wv];
        bm[T.lane] = 0u;
        bm[T.lane + 64] = 0u;
        wave_lds_sync();
        for (int e = T.lane; e < c; e += 64) {
            const unsigned int j = L.list[start + e];
            atomicOr(&bm[j >> 5], 1u << (j & 31u));
        }
        wave_lds_sync();
        unsigned int w0 = bm[2 * T.lane], w1 = bm[2 * T.lane + 1];
        const unsigned int p = __popc(w0) + __popc(w1);
        const unsigned int pin = wave_scan_incl(p);
        int pos = start + (int)(pin - p);
        while (w0) { L.list[pos++] = (unsigned short)(64 * T.lane + __ffs(w0) - 1); w0 &= w0 - 1u; }
        while (w1) { L.list[pos++] = (unsigned short)(64 * T.lane + 32 + __ffs(w1) - 1); w1 &= w1 - 1u; }
        wave_lds_sync();
        const size_t i = (size_t)(J.r0 + lr);
        V w;
        int jo;
        if (D3 && k < (unsigned int)kBgBigW) {  // the row's point and index came through LDS
            const float4 t = L.bigw[k];
            if constexpr (D3) w = P3{t.x, t.y, t.z};
            jo = __builtin_bit_cast(int, t.w);
        } else {
            if constexpr (D3) w = BgAcc<MODE>::row(J.own, i, 3, 0);
            jo = J.idx_own[i];
        }
        for (int d = 0; d < (D3 ? 1 : J.D); ++d) {  // (D = 3: the whole row at once)
            if constexpr (!D3) w = J.own[i * J.D + d];
            V ot{};  // the own term
            if (!D3 || R.own_opens() || R.own_closes()) ot = J.c_own * (w - BgAcc<MODE>::row(J.oth, (size_t)jo, J.D, d));
            BgAcc<MODE> acc(J, lr, d);
            acc.open(R, ot);
            for (int e0 = 0; e0 < c; e0 += 64) {
                V t{};
                if (e0 + T.lane < c) t = J.c_oth * (BgAcc<MODE>::row(J.oth, (size_t)(R.c0 + L.list[start + e0 + T.lane]), J.D, d) - w);
                const int n = c - e0 < 64 ? c - e0 : 64;
                for (int l = 0; l < n; ++l) acc.sub(lane_val(t, l));
            }
            acc.close(R, ot);
            if (T.lane == 0) acc.finish(J, R, lr);
        }
    }
}

// (5) the owners: short lists ordered in registers, subtracted in order (no barrier between (4) and (5): the waves
//     touch only the lists / rows of the long rows, which the owners skip).  Row by row: two rows at a time with every
//     stage's LDS reads issued together was measured slower at every list cap (4 / 6 / 8: the arrays of both rows spill)
template <int MODE>
__device__ __forceinline__ void bg_owners(const BgLds &L, const BgJob &J, const BgRound &R, const BgThread &T) {
    constexpr bool D3 = MODE != 1;
    using V = typename BgAcc<MODE>::V;
#pragma unroll
    for (int u = 0; u < kBgPer; ++u) {
        const int lr = T.tid + u * kBgThreads;
        if (!(u < T.rpt && lr < T.nrows)) continue;
        const int start = L.start[lr], c = (int)L.start[lr + 1] - start;
        if (c > kBgSmall || (c == 0 && !R.first && !R.last)) continue;
        unsigned int e[kBgSmall];
#pragma unroll
        for (int k = 0; k < kBgSmall; ++k) e[k] = k < c ? (unsigned int)L.list[start + k] : 0xFFFFu;
        if (c > 4) {
            ce(e[0], e[1]); ce(e[2], e[3]); ce(e[4], e[5]); ce(e[6], e[7]);
            ce(e[0], e[2]); ce(e[1], e[3]); ce(e[4], e[6]); ce(e[5], e[7]);
            ce(e[1], e[2]); ce(e[5], e[6]); ce(e[0], e[4]); ce(e[3], e[7]);
            ce(e[1], e[5]); ce(e[2], e[6]);
            ce(e[1], e[4]); ce(e[3], e[6]);
            ce(e[2], e[4]); ce(e[3], e[5]);
            ce(e[3], e[4]);
        } else if (c > 2) {
            ce(e[0], e[1]); ce(e[2], e[3]); ce(e[0], e[2]); ce(e[1], e[3]); ce(e[1], e[2]);
        } else if (c == 2) {
            ce(e[0], e[1]);
        }
        for (int d = 0; d < (D3 ? 1 : J.D); ++d) {  // (D = 3: the whole row at once)
            V w, o;
            if constexpr (D3) { w = P3{T.wx[u], T.wy[u], T.wz[u]}; o = P3{T.ojx[u], T.ojy[u], T.ojz[u]}; }
            else { w = J.own[(size_t)(J.r0 + lr) * J.D + d]; o = J.oth[(size_t)T.jown[u] * J.D + d]; }
            V ot{};  // the own term
            if (!D3 || R.own_opens() || R.own_closes()) ot = J.c_own * (w - o);
            BgAcc<MODE> acc(J, lr, d);
            acc.open(R, ot);
            if constexpr (D3) {
#pragma unroll
                for (int h = 0; h < kBgSmall; h += 4) {  // four gathers in flight
                    if (h >= c) break;
                    float ox[4], oy[4], oz[4];
#pragma unroll
                    for (int k = 0; k < 4; ++k) {  // (unconditional: a slot beyond the list re-reads the round's first row)
                        const P3 t = *reinterpret_cast<const P3 *>(J.oth + (size_t)(R.c0 + (h + k < c ? e[h + k] : 0u)) * 3);
                        ox[k] = t.x; oy[k] = t.y; oz[k] = t.z;
                    }
                    asm volatile("" : "+v"(ox[0]), "+v"(oy[0]), "+v"(oz[0]), "+v"(ox[1]), "+v"(oy[1]), "+v"(oz[1]), "+v"(ox[2]), "+v"(oy[2]),
                                      "+v"(oz[2]), "+v"(ox[3]), "+v"(oy[3]), "+v"(oz[3]));  // (all four requested before the first is used)
#pragma unroll
                    for (int k = 0; k < 4; ++k)
                        if (h + k < c) acc.sub(J.c_oth * (P3{ox[k], oy[k], oz[k]} - w));
                }
            } else {
#pragma unroll
                for (int k = 0; k < kBgSmall; ++k)
                    if (k < c) acc.sub(J.c_oth * (J.oth[(size_t)(R.c0 + e[k]) * J.D + d] - w));
            }
            acc.close(R, ot);
            acc.finish(J, R, lr);
        }
    }
}

// The rows [J.r0, J.r1) of the block's (cloud, side).  Every barrier of a round but the scan's own is here.
template <int MODE>
__device__ __forceinline__ void bg_rows(BgLds &L, const BgJob &J) {
    BgThread T;
    bg_load_rows<MODE>(J, T);
    BG_STAMP(0);
#pragma unroll
    for (int q = 0; q < kBgPer / 2; ++q) L.cnt2[kBgPer / 2 * T.tid + q] = 0u;  // (the placement of every round leaves the counters at zero)
    for (int c0 = 0; c0 < J.S; c0 += kBgChunk) {
        const BgRound R = bg_round(J, c0);
        bg_read_indices(L, J, R, T);     // (1)
        __syncthreads();
        BG_STAMP(1);
        bg_count(L, T);
        __syncthreads();
        BG_STAMP(2);
        bg_scan(L, T);                   // (2)
        __syncthreads();
        BG_STAMP(3);
        bg_place<MODE>(L, T);            // (3)
        __syncthreads();
        BG_STAMP(4);
        bg_long_rows<MODE>(L, J, R, T);  // (4)
        BG_STAMP(5);
        bg_owners<MODE>(L, J, R, T);     // (5)
        BG_STAMP(6);
        if (!R.last) __syncthreads();  // the next round reuses the image / start / list (and reads the accumulators back)
    }
}

// blk: the block's number among the launch's row blocks; one_side >= 0: only that side's rows are formed (B * nsplit blocks)
__device__ __forceinline__ BgJob bg_job(const float *x, int N, const float *y, int M, int D, const int32_t *idx_x,
                                        const int32_t *idx_y, float ca, float cb, int nsplit, int blk, int one_side = -1) {
    const int part = blk % nsplit, bs = blk / nsplit;
    const int b = one_side >= 0 ? bs : bs >> 1, side = one_side >= 0 ? one_side : bs & 1;  // side 0: gx, 1: gy
    BgJob J{};
    J.side = side; J.D = D; J.b = b;
    J.R = side ? M : N; J.S = side ? N : M;
    J.own = (side ? y : x) + (size_t)b * J.R * D;
    J.oth = (side ? x : y) + (size_t)b * J.S * D;
    J.idx_own = (side ? idx_y : idx_x) + (size_t)b * J.R;
    J.idx_oth = (side ? idx_x : idx_y) + (size_t)b * J.S;
    J.c_own = side ? cb : ca; J.c_oth = side ? ca : cb;
    const int per = (J.R + nsplit - 1) / nsplit;
    J.r0 = part * per < J.R ? part * per : J.R;
    J.r1 = J.r0 + per < J.R ? J.r0 + per : J.R;
    return J;
}

// (round 6) spare blocks behind the row blocks of fx3d_chamfer_sampled_bwd's first launch: block e builds the ordered gather's tables of
// mesh e of a side -- the draws bucketed by face, sample_gather.h: they depend on the draws alone -- and leaves them in the scratch for the
// gather's blocks (7 us of a gather block's work done while the rows are formed)
struct SgTabJobs {
    const int32_t *face_idx[2];  // (n, B) draws of side x / y; nullptr: no tables for that side
    unsigned char *blob[2];
    int F[2], n[2], B;
};
__device__ __forceinline__ void bg_passenger_block(int e, const SgTabJobs &tj, int ntab, const meshreg::Ride &ride, unsigned char *tab_lds) {
    if (e >= ntab) {  // the regularisers' adjoint (mesh_reg.h): reads the vertices and the forward's unit rows, writes gverts
        meshreg::adj_block(ride, e - ntab);
        return;
    }
    int side = 0;
    if (tj.face_idx[0]) { if (e >= tj.B) { e -= tj.B; side = 1; } } else side = 1;
    sg::SgMesh m{};
    m.face_idx = tj.face_idx[side] + (size_t)e * tj.n[side];
    m.F = tj.F[side]; m.n = tj.n[side];
    sg::sg_tables(tab_lds, m);
    sg::sg_tables_store(tab_lds, m.F, m.n, tj.blob[side] + (size_t)e * sg::sg_blob_bytes(m.F, m.n));
}
// RIDE: the launch carries passengers behind its nrow row blocks (fx3d_chamfer_sampled_bwd's first launch); fx3d_chamfer_bwd's own
// launches are compiled without them
template <bool D3, bool RIDE>
__global__ __launch_bounds__(kBgThreads, kBgOcc) void chamfer_bwd_gather_kernel(
    const float *__restrict__ x, int N, const float *__restrict__ y, int M, int D, const int32_t *__restrict__ idx_x,
    const int32_t *__restrict__ idx_y, float ca, float cb, float *__restrict__ gx, float *__restrict__ gy, int nsplit, int npass,
    SgTabJobs tj, int ntab, meshreg::Ride ride) {
    int blk = (int)blockIdx.x, one_side = -1;
    if constexpr (RIDE) {
        // the passengers take the FIRST npass block numbers: blocks are handed to the CUs in order, and behind a full round of row blocks
        // (eight meshes: 256) the tables started a row block's time late -- the launch took 21 us instead of 10
        if (blk < npass) {
            extern __shared__ __attribute__((aligned(16))) unsigned char tab_lds[];
            bg_passenger_block(blk, tj, ntab, ride, tab_lds);
            return;
        }
        blk -= npass;
        one_side = !gy ? 0 : (!gx ? 1 : -1);  // (a fitting loop differentiates w.r.t. one mesh: no blocks for the other side's rows)
    }
    __shared__ BgLds L;
    BgJob J = bg_job(x, N, y, M, D, idx_x, idx_y, ca, cb, nsplit, blk, one_side);
    if (!(J.side ? gy : gx)) return;  // (a side nobody asked for: fx3d_chamfer_sampled_bwd differentiates w.r.t. one mesh)
    J.g = (J.side ? gy : gx) + (size_t)J.b * J.R * D;
    bg_rows<D3 ? 0 : 1>(L, J);
}

// Adjoint of chamfer_distance(sample_points(m_x), sample_points(m_y)) w.r.t. the meshes' vertices, SCATTER form, in one launch: the
// gradient w.r.t. the sampled points is formed exactly as in chamfer_bwd_gather_kernel (D = 3), then every finished row goes onto
// the three vertices of its sampled face with global float atomics (sums in arrival order) instead of being written out.  A side
// without a mesh gradient (gverts == nullptr) is skipped.  (The ORDERED form -- fx3d_chamfer_sampled_bwd with the vertex -> face
// tables -- is two launches: chamfer_bwd_gather_kernel writes the rows, sample_bwd_gather_kernel gathers them, sample_gather.h.)
__global__ __launch_bounds__(kBgThreads, kBgOcc) void chamfer_sampled_bwd_kernel(
    const float *__restrict__ x, int N, const float *__restrict__ y, int M, const int32_t *__restrict__ idx_x,
    const int32_t *__restrict__ idx_y, float ca, float cb, SampledSide sx, SampledSide sy, int nsplit) {
    __shared__ BgLds L;
    extern __shared__ __attribute__((aligned(16))) unsigned char bg_dyn[];  // the accumulators between rounds (n > 4096 samples)
    BgJob J = bg_job(x, N, y, M, 3, idx_x, idx_y, ca, cb, nsplit, (int)blockIdx.x);
    J.smp = J.side ? sy : sx;
    if (!J.smp.gverts) return;
    J.part = reinterpret_cast<P3 *>(bg_dyn);
    bg_rows<2>(L, J);
}

// blocks per (cloud, side): ONE round of blocks on the chip (a block is a chain of dependent phases: a second round doubles the
// time), a block never owns fewer than 256 rows nor more than kBgRows.  Measured (kernel us, B x N): 32 x 4096: 15 / 11.7 / 18 / 28
// at 1 / 4 / 8 / 16 blocks per side; 8 x 5000: 17 / 13.5 / 11.6 at 1 / 4 / 16; 1 x 16384: 31 / 23 / 20 at 1 / 8 / 16.
int bg_nsplit(int B, int maxr, int sides = 2) {
    int nsplit = device_cus() / (sides * B);
    if (nsplit > maxr / 256) nsplit = maxr / 256;
    if (nsplit < 1) nsplit = 1;
    while ((maxr + nsplit - 1) / nsplit > kBgRows) ++nsplit;
    return nsplit;
}

// The weights of the two sums' gradient rows.  ONE expression, its order fixed: these are the bits every adjoint multiplies by.
struct ChamferCoef { float ca, cb; };
ChamferCoef chamfer_coef(float gout, float w1, float w2, int D, int N, int M, int64_t B_global) {
    return ChamferCoef{gout * w1 * (float)(6.0 / ((double)D * N * (double)B_global)),
                       gout * w2 * (float)(6.0 / ((double)D * M * (double)B_global))};
}

// The one launch site of chamfer_bwd_gather_kernel: `nsplit` row blocks per cloud and side with a gradient array.
// pass == nullptr (fx3d_chamfer_bwd, any D): the row blocks alone.  Otherwise (fx3d_chamfer_sampled_bwd's first launch, D = 3): in
// front of them the passengers -- ntab table jobs with `lds` bytes of dynamic LDS, then the regularisers' adjoint blocks.
constexpr size_t kTabLds = 112 * 1024;  // what the table jobs may take beside the row blocks' 38 KB of static LDS
struct BgPassengers {
    SgTabJobs tj;
    int ntab;
    size_t lds;
    const meshreg::Ride *ride;
};
fx3d_status launch_bwd_gather(const float *x, int N, const float *y, int M, int B, int D, const int32_t *idx_x, const int32_t *idx_y,
                              ChamferCoef c, float *gx, float *gy, int nsplit, const BgPassengers *pass, hipStream_t st) {
    const BgPassengers P = pass ? *pass : BgPassengers{};
    const auto kernel = pass ? chamfer_bwd_gather_kernel<true, true>
                             : (D == 3 ? chamfer_bwd_gather_kernel<true, false> : chamfer_bwd_gather_kernel<false, false>);
    if (P.ntab) FX3D_TRY(ensure_dynamic_lds(reinterpret_cast<const void *>(kernel), (int)kTabLds, "chamfer_bwd_gather_kernel"));
    const int sides = (gx ? 1 : 0) + (gy ? 1 : 0), npass = P.ntab + (P.ride ? P.ride->nadj : 0);
    ProfileScope prof(pass ? "chamfer_sampled_bwd" : "chamfer_bwd", st);
    hipLaunchKernelGGL(kernel, dim3(npass + sides * B * nsplit), dim3(kBgThreads), P.lds, st, x, N, y, M, D, idx_x, idx_y, c.ca, c.cb, gx, gy,
                       nsplit, npass, P.tj, P.ntab, P.ride ? *P.ride : meshreg::Ride{});
    FX3D_LAUNCH_CHECK();
    return FX3D_OK;
}

}  // namespace

extern "C" {

fx3d_status fx3d_chamfer_bwd(const float *x, int32_t N, const float *y, int32_t M, int32_t B,
                             int32_t D, const int32_t *idx_x, const int32_t *idx_y, float w1,
                             float w2, float gout, int64_t B_global, float *gx, float *gy,
                             fx3d_stream_t s) {
    fx3d_status rc = chamfer_check_shapes("fx3d_chamfer_bwd", x, N, y, M, B, D);
    if (rc) return rc;
    FX3D_REQUIRE(idx_x && idx_y && gx && gy, "fx3d_chamfer_bwd: null pointer");
    FX3D_REQUIRE(B_global >= B, "fx3d_chamfer_bwd: B_global < B");
    hipStream_t st = as_stream(s);
    const ChamferCoef c = chamfer_coef(gout, w1, w2, D, N, M, B_global);
    const int nsplit = bg_nsplit(B, N > M ? N : M);
    if ((long long)2 * B * nsplit < (1ll << 30) && !opt(OPT_BWD_GLOBAL_ATOMICS))
        return launch_bwd_gather(x, N, y, M, B, D, idx_x, idx_y, c, gx, gy, nsplit, nullptr, st);
    const long long total = (long long)B * (N + M);
    long long blocks = (total + kThreads - 1) / kThreads;
    if (blocks > 4096) blocks = 4096;
    {
        ProfileScope prof("chamfer_bwd", st);
        hipLaunchKernelGGL(chamfer_bwd_kernel<false>, dim3((unsigned)blocks), dim3(kThreads), 0, st, x, N, y, M,
                           B, D, idx_x, idx_y, c.ca, c.cb, gx, gy);
        hipLaunchKernelGGL(chamfer_bwd_kernel<true>, dim3((unsigned)blocks), dim3(kThreads), 0, st, x, N, y, M,
                           B, D, idx_x, idx_y, c.ca, c.cb, gx, gy);
    }
    FX3D_LAUNCH_CHECK();
    return FX3D_OK;
}

#ifdef FX3D_BG_PROBE
__attribute__((visibility("default"))) int fx3d_debug_bg_probe(unsigned long long *host) {
    return (int)hipMemcpyFromSymbol(host, HIP_SYMBOL(g_bg_probe), sizeof(unsigned long long) * 1024 * 8);
}
#endif

}  // extern "C"

namespace {
size_t al256(size_t v) { return (v + 255) & ~(size_t)255; }
// The ordered form's scratch: the chamfer adjoint's rows of both sides, then the gather's tables of both sides (one blob per mesh), every
// part 256-byte aligned.  ASYMMETRY, on purpose: `total` is sized for the largest face count the ordered form takes at these draw counts
// (kSgMaxF -- the size query need not name Fmax), while the blobs are laid out with the stride of the ACTUAL Fmax, y's behind the blobs
// x actually has (nothing lies behind y's, so y's mesh does not enter).
struct SampledWs {
    size_t gsx, gsy, tbx, tby, total;  // byte offsets
    static SampledWs plan(int N, int M, int B, int Fmax_x, bool want_x) {
        SampledWs w{};
        w.gsy = w.gsx + al256(sizeof(float) * 3 * (size_t)N * B);
        w.tbx = w.gsy + al256(sizeof(float) * 3 * (size_t)M * B);
        w.tby = w.tbx + al256(want_x ? sg::sg_blob_bytes(Fmax_x, N) * (size_t)B : 0);
        w.total = w.tbx + al256(sg::sg_blob_bytes(sg::kSgMaxF, N) * (size_t)B) + al256(sg::sg_blob_bytes(sg::kSgMaxF, M) * (size_t)B);
        return w;
    }
};
// fx3d_chamfer_fwd_bwd's scratch: the forward's own (fx3d_chamfer_workspace_bytes, rounded up to 256), then the (N + M, B) neighbour indices
struct FwdBwdWs {
    size_t fwd, total;  // bytes of the forward's part = offset of the indices; bytes in all
    static fx3d_status plan(int N, int M, int B, int D, FwdBwdWs *w) {
        FX3D_TRY(fx3d_chamfer_workspace_bytes(N, M, B, D, &w->fwd));
        w->fwd = al256(w->fwd);
        w->total = w->fwd + al256(sizeof(int32_t) * (size_t)B * ((size_t)N + M));
        return FX3D_OK;
    }
};
// ax / ay: the two sides, x's first; a side without gverts gets no gradient
fx3d_status chamfer_sampled_bwd_impl(const char *fn, const float *x, int32_t N, const float *y, int32_t M, int32_t B, const int32_t *idx_x,
                                     const int32_t *idx_y, float w1, float w2, float gout, int64_t B_global, const SampledSide &ax,
                                     const SampledSide &ay, int32_t accumulate, const sg::SgStep &step_x, void *ws, size_t ws_bytes,
                                     fx3d_stream_t s, const fx3d_mesh_reg *reg = nullptr) {
    const SampledSide *const side[2] = {&ax, &ay};
    const int cnt[2] = {N, M};  // a side's samples
    fx3d_status rc = chamfer_check_shapes(fn, x, N, y, M, B, 3);
    if (rc) return rc;
    FX3D_REQUIRE(idx_x && idx_y, "%s: null index array", fn);
    FX3D_REQUIRE(ax.gverts || ay.gverts, "%s: no gradient requested", fn);
    for (int k = 0; k < 2; ++k)
        FX3D_REQUIRE(!side[k]->gverts || side[k]->complete(), "%s: incomplete mesh of %s", fn, k ? "y" : "x");
    FX3D_REQUIRE((ax.vf_rowptr == nullptr) == (ax.vf_ent == nullptr) && (ay.vf_rowptr == nullptr) == (ay.vf_ent == nullptr),
                 "%s: vf_rowptr and vf_ent go together", fn);
    FX3D_REQUIRE(B_global >= B, "%s: B_global < B", fn);
    hipStream_t st = as_stream(s);
    const ChamferCoef c = chamfer_coef(gout, w1, w2, 3, N, M, B_global);
    const int nsplit = bg_nsplit(B, N > M ? N : M);
    FX3D_REQUIRE((long long)2 * B * nsplit < (1ll << 30), "%s: batch too large", fn);
    // Ordered form (no float atomics, bit-identical to the oracle): every requested side comes with its vertex -> face table and
    // fits the gather's LDS tables.  Otherwise: the float-atomic scatter.
    bool ordered = true;
    for (int k = 0; k < 2; ++k) ordered = ordered && (!side[k]->gverts || (side[k]->vf_rowptr && sg::sg_fits(side[k]->Fmax, cnt[k])));
    FX3D_REQUIRE(!step_x.vel || (ordered && ax.gverts), "%s: the optimiser step needs the ordered form (vertex -> face table, draws that fit "
                 "fx3d_sample_points_bwd_ordered)", fn);
    // (refused before any device work: the regularisers' stand-alone adjoint below writes gverts_x and total_dev)
    const SampledWs W = SampledWs::plan(N, M, B, ax.Fmax, ax.gverts != nullptr);
    if (ordered) FX3D_TRY(ws_check(fn, "workspace", ws, ws_bytes, W.total));
    // the fit iteration's regularisers (fx3d_mesh_reg): their adjoint writes gverts_x, the sampling adjoint then accumulates on top
    meshreg::Ride ride_v{};
    const meshreg::Ride *ride = nullptr;
    if (reg) {
        FX3D_REQUIRE(ax.gverts && reg->V == (int64_t)ax.Vmax * B, "%s: fx3d_mesh_reg covers the source batch (V = %lld, B * Vmax = %lld)", fn,
                     (long long)reg->V, (long long)ax.Vmax * B);
        rc = mesh_reg_plan(reg, gout, ax.gverts, accumulate, st, fn, &ride_v);
        if (rc) return rc;
        if (ordered && ride_v.c_lap != 0.0f && ride_v.c_edge != 0.0f) ride = &ride_v;  // rides in the rows launch
        else {  // (a weight of zero drops its term, fx3d_mesh_losses_bwd knows how; the scatter form is one launch with no room)
            rc = mesh_reg_adjoint_standalone(reg, gout, ax.gverts, accumulate, st);
            if (rc) return rc;
        }
        accumulate = 1;
    }
    if (ordered) {
        // two launches: the chamfer adjoint's rows of the requested sides into the scratch (bit-identical to fx3d_chamfer_bwd), then the
        // ordered gather of every side (+ the optimiser step).  (One launch -- gather blocks behind the row blocks, waiting on a counter --
        // was built and measured equal inside the fit loop's graph, 104 against 105 us per iteration: the gather's tables, 7 us, do
        // overlap the rows there, but its tail -- acquire, staging, walk: ~9 us -- does not shrink; not kept: a bounded spin and a
        // dispatch-order argument for nothing.)
        unsigned char *w = static_cast<unsigned char *>(ws);
        float *const gs[2] = {reinterpret_cast<float *>(w + W.gsx), reinterpret_cast<float *>(w + W.gsy)};
        unsigned char *tb[2] = {w + W.tbx, w + W.tby};
        // the rows of the requested sides + (in front of them, one block per mesh and side) the gather's tables
        BgPassengers P{};
        P.tj.B = B;
        P.ride = ride;
        for (int k = 0; k < 2; ++k) {
            const SampledSide &a = *side[k];
            if (!a.gverts) continue;
            P.tj.face_idx[k] = a.face_idx; P.tj.blob[k] = tb[k]; P.tj.F[k] = a.Fmax; P.tj.n[k] = cnt[k];
            P.lds = std::max(P.lds, sg::sg_tables_lds_bytes(a.Fmax, cnt[k]));
            P.ntab += B;
        }
        if (P.lds > kTabLds) {  // (meshes of > ~20 000 faces: every gather block builds its own tables, as fx3d_sample_points_bwd's do)
            P.tj = SgTabJobs{};
            P.lds = 0; P.ntab = 0;
            tb[0] = tb[1] = nullptr;
        }
        const int sides = (ax.gverts ? 1 : 0) + (ay.gverts ? 1 : 0);
        const int ns = bg_nsplit(B, sides == 2 ? (N > M ? N : M) : (ax.gverts ? N : M), sides);  // (row blocks of the requested sides only)
        FX3D_TRY(launch_bwd_gather(x, N, y, M, B, 3, idx_x, idx_y, c, ax.gverts ? gs[0] : nullptr, ay.gverts ? gs[1] : nullptr, ns, &P, st));
        for (int k = 0; k < 2; ++k) {
            const SampledSide &a = *side[k];
            if (a.gverts)
                FX3D_TRY(sg::launch_sample_bwd_gather(a.faces, a.Vmax, a.Fmax, B, cnt[k], a.face_idx, a.r1, a.r2, gs[k], a.vf_rowptr, a.vf_ent,
                                                      a.gverts, accumulate, k == 0 ? step_x : sg::SgStep{}, st, tb[k]));
        }
        return FX3D_OK;
    }
    if (!accumulate)
        for (int k = 0; k < 2; ++k)
            if (side[k]->gverts) FX3D_FILL(side[k]->gverts, 0, sizeof(float) * 3 * (size_t)side[k]->Vmax * B, st);
    // sides beyond kBgChunk samples (the reference's default is 5000): the accumulators between the rounds live in LDS
    const int maxr = N > M ? N : M;
    const size_t dyn = maxr > kBgChunk ? sizeof(P3) * (size_t)((maxr + nsplit - 1) / nsplit) : 0;
    if (dyn > 0) {  // static BgLds (~38 KB) + up to 48 KB of accumulators: beyond the 64 KB a kernel gets without an opt-in
        const fx3d_status arc = ensure_dynamic_lds(reinterpret_cast<const void *>(&chamfer_sampled_bwd_kernel), (int)(sizeof(P3) * kBgRows),
                                                   "chamfer_sampled_bwd_kernel");
        if (arc != FX3D_OK) return arc;
    }
    ProfileScope prof("chamfer_sampled_bwd", st);
    hipLaunchKernelGGL(chamfer_sampled_bwd_kernel, dim3(2 * B * nsplit), dim3(kBgThreads), dyn, st, x, N, y, M, idx_x, idx_y, c.ca,
                       c.cb, ax, ay, nsplit);
    FX3D_LAUNCH_CHECK();
    return FX3D_OK;
}

// fx3d_chamfer_sampled_bwd_step and _step_reg (reg: the regularisers that ride): the gradient w.r.t. mesh x alone + the optimiser step
fx3d_status sampled_bwd_step(const char *fn, const float *x, int32_t N, const float *y, int32_t M, int32_t B, const int32_t *idx_x,
                             const int32_t *idx_y, float w1, float w2, float gout, const int32_t *faces_x, int32_t V, int32_t F,
                             const int32_t *face_idx_x, const float *r1_x, const float *r2_x, float *gverts_x, int32_t accumulate,
                             const int32_t *vf_rowptr_x, const int32_t *vf_ent_x, float rho, float eta, float *vel, float *params,
                             const float *base, float *out, uint64_t *ctr, uint64_t inc, void *ws, size_t ws_bytes,
                             const fx3d_mesh_reg *reg, fx3d_stream_t s) {
    FX3D_REQUIRE(vel && params && base && out && gverts_x, "%s: null pointer", fn);
    const SampledSide ax{faces_x, face_idx_x, r1_x, r2_x, gverts_x, V, F, vf_rowptr_x, vf_ent_x};
    const SampledSide ay{};
    const sg::SgStep st{rho, eta, vel, params, base, out, reinterpret_cast<unsigned long long *>(ctr), (unsigned long long)inc};
    return chamfer_sampled_bwd_impl(fn, x, N, y, M, B, idx_x, idx_y, w1, w2, gout, B, ax, ay, accumulate, st, ws, ws_bytes, s, reg);
}
}  // namespace

extern "C" {

fx3d_status fx3d_chamfer_sampled_bwd_workspace_bytes(int32_t N, int32_t M, int32_t B, size_t *bytes) {
    FX3D_REQUIRE(bytes, "fx3d_chamfer_sampled_bwd_workspace_bytes: null output");
    FX3D_REQUIRE(N > 0 && M > 0 && B > 0, "fx3d_chamfer_sampled_bwd_workspace_bytes: bad sizes");
    *bytes = SampledWs::plan(N, M, B, sg::kSgMaxF, true).total;
    return FX3D_OK;
}

fx3d_status fx3d_chamfer_sampled_bwd(const float *x, int32_t N, const float *y, int32_t M, int32_t B, const int32_t *idx_x,
                                     const int32_t *idx_y, float w1, float w2, float gout, int64_t B_global,
                                     const int32_t *faces_x, int32_t Vmax_x, int32_t Fmax_x, const int32_t *face_idx_x,
                                     const float *r1_x, const float *r2_x, float *gverts_x, const int32_t *faces_y,
                                     int32_t Vmax_y, int32_t Fmax_y, const int32_t *face_idx_y, const float *r1_y,
                                     const float *r2_y, float *gverts_y, int32_t accumulate, const int32_t *vf_rowptr_x,
                                     const int32_t *vf_ent_x, const int32_t *vf_rowptr_y, const int32_t *vf_ent_y, void *ws,
                                     size_t ws_bytes, fx3d_stream_t s) {
    const SampledSide ax{faces_x, face_idx_x, r1_x, r2_x, gverts_x, Vmax_x, Fmax_x, vf_rowptr_x, vf_ent_x};
    const SampledSide ay{faces_y, face_idx_y, r1_y, r2_y, gverts_y, Vmax_y, Fmax_y, vf_rowptr_y, vf_ent_y};
    return chamfer_sampled_bwd_impl("fx3d_chamfer_sampled_bwd", x, N, y, M, B, idx_x, idx_y, w1, w2, gout, B_global, ax, ay, accumulate,
                                    sg::SgStep{}, ws, ws_bytes, s);
}

fx3d_status fx3d_chamfer_sampled_bwd_step(const float *x, int32_t N, const float *y, int32_t M, int32_t B, const int32_t *idx_x,
                                          const int32_t *idx_y, float w1, float w2, float gout, const int32_t *faces_x,
                                          int32_t V, int32_t F, const int32_t *face_idx_x, const float *r1_x, const float *r2_x,
                                          float *gverts_x, int32_t accumulate, const int32_t *vf_rowptr_x, const int32_t *vf_ent_x,
                                          float rho, float eta, float *vel, float *params, const float *base, float *out,
                                          uint64_t *ctr, uint64_t inc, void *ws, size_t ws_bytes, fx3d_stream_t s) {
    return sampled_bwd_step("fx3d_chamfer_sampled_bwd_step", x, N, y, M, B, idx_x, idx_y, w1, w2, gout, faces_x, V, F, face_idx_x, r1_x, r2_x,
                            gverts_x, accumulate, vf_rowptr_x, vf_ent_x, rho, eta, vel, params, base, out, ctr, inc, ws, ws_bytes, nullptr, s);
}

fx3d_status fx3d_chamfer_sampled_bwd_step_reg(const float *x, int32_t N, const float *y, int32_t M, int32_t B, const int32_t *idx_x,
                                              const int32_t *idx_y, float w1, float w2, float gout, const int32_t *faces_x,
                                              int32_t V, int32_t F, const int32_t *face_idx_x, const float *r1_x, const float *r2_x,
                                              float *gverts_x, int32_t accumulate, const int32_t *vf_rowptr_x, const int32_t *vf_ent_x,
                                              float rho, float eta, float *vel, float *params, const float *base, float *out,
                                              uint64_t *ctr, uint64_t inc, void *ws, size_t ws_bytes, const fx3d_mesh_reg *reg,
                                              fx3d_stream_t s) {
    FX3D_REQUIRE(reg, "fx3d_chamfer_sampled_bwd_step_reg: null pointer");
    return sampled_bwd_step("fx3d_chamfer_sampled_bwd_step_reg", x, N, y, M, B, idx_x, idx_y, w1, w2, gout, faces_x, V, F, face_idx_x, r1_x, r2_x,
                            gverts_x, accumulate, vf_rowptr_x, vf_ent_x, rho, eta, vel, params, base, out, ctr, inc, ws, ws_bytes, reg, s);
}

// Value AND gradient in one ABI call (the shape of `gradient(() -> chamfer_distance(A, B), ...)`, benchmarks/metrics.jl:24-38,
// examples/fit_mesh.jl:106-110): the forward with indices and the adjoint are queued back to back on the stream, the
// nearest-neighbour indices stay in the caller's scratch (or go to idx_x / idx_y when the caller wants them).  Two ABI calls
// leave the device idle between the launches for as long as the host needs for the second call.
fx3d_status fx3d_chamfer_fwd_bwd_workspace_bytes(int32_t N, int32_t M, int32_t B, int32_t D, size_t *bytes) {
    FX3D_REQUIRE(bytes, "fx3d_chamfer_fwd_bwd_workspace_bytes: null output");
    FwdBwdWs W;
    FX3D_TRY(FwdBwdWs::plan(N, M, B, D, &W));
    *bytes = W.total;
    return FX3D_OK;
}

fx3d_status fx3d_chamfer_fwd_bwd(const float *x, int32_t N, const float *y, int32_t M, int32_t B, int32_t D, float w1,
                                 float w2, float gout, int64_t B_global, float *loss_dev, float *loss_host, float *gx,
                                 float *gy, int32_t *idx_x, int32_t *idx_y, void *ws, size_t ws_bytes, fx3d_stream_t s) {
    fx3d_status rc = chamfer_check_shapes("fx3d_chamfer_fwd_bwd", x, N, y, M, B, D);
    if (rc) return rc;
    FX3D_REQUIRE(loss_dev && gx && gy, "fx3d_chamfer_fwd_bwd: null output pointer");
    FX3D_REQUIRE(B_global >= B, "fx3d_chamfer_fwd_bwd: B_global < B");
    FwdBwdWs W;
    FX3D_TRY(FwdBwdWs::plan(N, M, B, D, &W));
    FX3D_TRY(ws_check("fx3d_chamfer_fwd_bwd", "workspace", ws, ws_bytes, W.total));
    int32_t *ix = reinterpret_cast<int32_t *>(static_cast<char *>(ws) + W.fwd);
    int32_t *iy = ix + (size_t)B * N;
    if (idx_x) ix = idx_x;
    if (idx_y) iy = idx_y;
    rc = chamfer_forward(x, N, y, M, B, D, nullptr, loss_dev, (long long)B_global, w1, w2, ix, iy, ws, W.fwd, as_stream(s),
                         "fx3d_chamfer_fwd_bwd");
    if (rc) return rc;
    rc = fx3d_chamfer_bwd(x, N, y, M, B, D, ix, iy, w1, w2, gout, B_global, gx, gy, s);
    if (rc) return rc;
    if (loss_host) {
        FX3D_HIP(hipMemcpyAsync(loss_host, loss_dev, sizeof(float), hipMemcpyDeviceToHost, as_stream(s)));
        FX3D_HIP(hipStreamSynchronize(as_stream(s)));
    }
    return FX3D_OK;
}

}  // extern "C"
