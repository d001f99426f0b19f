// What the units of the chamfer forward / nearest-neighbour family share.  One unit per kernel family, as for k-NN:
//   chamfer.hip       nn1_f16_kernel (D = 3, the default) + nn1_split_finalize_kernel, and the functions that launch them
//   nn1_exact.hip     the exact kernels: nn1_tiny_kernel, nn1_small_d_kernel, nn1_generic_kernel, and their launcher
//   chamfer_host.hip  the launch plan (make_plan), the workspace layout, the drivers, the loss kernels, the C entry points
// Here: the kernels' parameter block, the constants a kernel and the planner both use, the order of distances, the loss
// formula and the fused "last block finalises" tail.
#pragma once
#include "fx3d_common.h"

namespace fx3d {

constexpr int kThreads = 256;   // the exact kernels, nn1_split_finalize_kernel, the partials' reduction
constexpr int kTile = 32;       // candidates per min3 tile
constexpr int kChunkMax = 4096; // candidates staged in LDS at once (DIM*16 KiB)

struct Nn1Params {
    const float *x;  // (D,N,B)
    const float *y;  // (D,M,B)
    int N, M, B;
    int32_t *idx_x, *idx_y;  // optional
    float *dmin_x, *dmin_y;  // optional
    double *partials;        // [2*Bpad8... ] one per (cloud, tile); optional
    int tiles;               // max(tiles_x, tiles_y)
    int tiles_x, tiles_y;
    int chunk;               // LDS chunk capacity (multiple of kTile)
    int tpb;                 // fp16 variant: query-tile passes per block (>1 only for one-chunk clouds), x -> y direction
    int tpb_y;               // ... y -> x direction (clouds of different sizes: the plan balances the two directions' blocks)
    // fused finalisation (fp16 variant): the last block to arrive reduces the partials in fixed order
    unsigned int *ticket;    // library-owned arrival counter, zero between launches; nullptr = no fusion
    unsigned int nvalid;     // number of blocks that deliver a partial
    double *sums_out;        // [2] optional
    float *loss_out;         // optional
    float w1, w2;
    long long Bg;
    // candidate split (few, large clouds): blocks of one query tile take different chunk subsets and
    // merge per query through 64-bit atomics in global scratch; nn1_split_finalize_kernel unpacks
    int nsplit;                  // 1 = off
    unsigned long long *gres;    // [nsplit][2B][qstride] packed (d_bits << 32 | index): every split block stores its own row (no init, no atomics)
    int qstride;
    int fuse_split;              // 1: the last block of a query tile's chunk subsets merges their rows itself (arrival counters in the ticket slot's spare words)
    int tail;                    // > 0: a cloud of chunk + (1 .. tail) points is ONE chunk + a tail every query evaluates exactly
    // spatial pruning (round 6, nn1_f16_kernel<.., PRUNE = true>): per-block scratch in the caller's workspace -- the block's candidate
    // cloud in image order and its window of the query cloud in processing order, as 16-bit ORIGINAL INDICES (a pruned launch holds
    // either cloud in one chunk of at most kHChunkMax points); the readers fetch the points themselves from x / y by index
    unsigned short *pscr;        // nullptr: the launch runs the PRUNE = false instantiation
    int pscr_stride;             // slots per block: kHScrCand candidates + the query window (passes x 512 + kHTail)
};

// The kernel a launch plan runs (chamfer_host.hip: plan_kernel) and the units' launchers.  Grid and dynamic LDS are the plan's;
// the instantiation (want indices; fp16: pruned / fused split merge) follows from `p`.
enum Nn1Kernel { NN1_GENERIC, NN1_SMALL_D, NN1_TINY, NN1_F16 };
fx3d_status nn1_exact_launch(Nn1Kernel k, const Nn1Params &p, int D, int R, int grid, size_t lds_bytes, hipStream_t st);  // nn1_exact.hip
size_t nn1_f16_lds_bytes(int chunk);  // chamfer.hip: image of `chunk` candidates + the kernel's scratch (the -D FX3D_H* build knobs size it)
fx3d_status nn1_f16_launch(const Nn1Params &p, int grid, size_t lds_bytes, hipStream_t st);
fx3d_status nn1_split_finalize_launch(const Nn1Params &p, int tiles_f, hipStream_t st);

__device__ __forceinline__ float min3f(float a, float b, float c) {
    return __builtin_fminf(__builtin_fminf(a, b), c);
}

template <int DIM>
__device__ __forceinline__ float sqd(const float (&q)[DIM], const float (&c)[DIM]) {
    float t0 = q[0] - c[0];
    float s = t0 * t0;
#pragma unroll
    for (int d = 1; d < DIM; ++d) {
        float t = q[d] - c[d];
        s = s + t * t;
    }
    return s;
}

// Order of distances = the oracle's (oracle/flux3d_oracle.c: fless): Julia's isless on Float32 -- ascending, every NaN
// after +Inf, all NaNs equal -- then the lower index.  Squared distances are >= +0 or NaN, so the order is the unsigned
// order of the bit patterns once NaNs are canonical; finite data never produces a NaN distance (at worst +Inf), and
// the hot paths below only pay for this on data that is not finite.
__device__ __forceinline__ bool fless(float a, float b) { return (a < b) || (b != b && a == a); }
__device__ __forceinline__ unsigned int dist_key(float d) { return d != d ? 0x7fc00000u : __builtin_bit_cast(unsigned int, d); }

// exact scan of a whole cloud in that order (the rare exit of the exact-loop kernels: no distance below +Inf)
template <int DIM>
__device__ __forceinline__ void nn1_scan_isless(const float (&q)[DIM], const float *__restrict__ cb, int NC, float &best, int &bi) {
    float c0[DIM];
#pragma unroll
    for (int d = 0; d < DIM; ++d) c0[d] = cb[d];
    best = sqd<DIM>(q, c0);
    bi = 0;
    for (int j = 1; j < NC; ++j) {
        float cc[DIM];
#pragma unroll
        for (int d = 0; d < DIM; ++d) cc[d] = cb[(size_t)j * DIM + d];
        const float dd = sqd<DIM>(q, cc);
        if (fless(dd, best)) { best = dd; bi = j; }
    }
}

// nn1_f16_kernel's geometry, as far as the planner needs it (the rest, with its build knobs, is in chamfer.hip)
constexpr int kHThreads = 1024;   // 16 waves share one LDS image: 1 block per CU, 4 waves per SIMD
#ifndef FX3D_HLT
#define FX3D_HLT 2
#endif
constexpr int kHLT = FX3D_HLT;    // 32-candidate blocks per lane tile (lane sees 16 rows of each)
constexpr int kHChunkMax = 4096;  // 32 B per candidate => 128 KiB
constexpr int kHTail = 64;        // a cloud of up to kHChunkMax + kHTail points stays one LDS image: the last <= 64 candidates are
                                  // compared exactly by every query (N = M = 4097 was 2.1 x N = M = 4096: two half-empty chunks,
                                  // three rounds of blocks), and <= 64 queries beyond a block's passes are one more pass of one wave
constexpr int kHScrCand = kHChunkMax + 64;  // (PRUNE) candidate slots of a block's scratch: the image's positions, its two padding blocks included

// nn1_tiny_kernel's geometry (nn1_exact.hip)
constexpr int kTyThreads = 256;
constexpr int kTyQ = 16;                      // queries per 16-lane row
constexpr int kTySl = 16;                     // candidate slices per block (4 per wave, one per DPP row)
constexpr int kTyG = 16;                      // candidates per group (one per lane of a row)

__device__ __forceinline__ float chamfer_loss_from_sums(double sa, double sb, int N, int M, int D,
                                                        long long Bg, float w1, float w2) {
    // mean(...) * 3.0f0, src/metrics/pcloud.jl:47-48 ; w1*dA + w2*dB, :50
    const float dA = (float)(sa / ((double)D * (double)N * (double)Bg)) * 3.0f;
    const float dB = (float)(sb / ((double)D * (double)M * (double)Bg)) * 3.0f;
    return (w1 * dA) + (w2 * dB);
}

// The tail of a launch with fused finalisation, run by the FIRST WAVE of every block after the block's sum `tot` has
// arrived in its lane 0: publish the partial (8-byte agent-scope store -> drain -> relaxed ticket), and the last arriver
// reduces all partials in a fixed order and writes the sums / the loss.  That reduction is the launch's tail -- every
// other CU is idle by then --, so it is one wave, all its loads in flight together (four per lane and direction), DPP
// double adds, no barrier, 32-bit index math (the block-wide version with two barrier rounds and 64-bit divisions took
// 6.0 k cycles from ticket to end at C2; this one 2.3 k).  `slot`: this block's entry; rows of `stride` entries per
// (direction, cloud), the first tiles_x / tiles_y of a row are valid.
// MEMORY-ORDER NOTE (applies to this hand-off and to the fused split merge further down).  The protocol is
//   producer:  agent-scope RELAXED atomic stores of the data (sc1: they go THROUGH the XCD's L2 to memory) -> s_waitcnt vmcnt(0) (the
//              stores have left the CU and are acknowledged) -> relaxed agent-scope fetch_add on the counter
//   consumer:  the last arriver's relaxed agent-scope atomic LOADS of the data (sc1: served from memory / the coherent fabric,
//              never from a stale line of its own XCD's L2)
// i.e. ordering by completion (waitcnt) + coherence by the access kind, not by release / acquire fences.  It is outside the HIP /
// LLVM memory model on purpose: an agent-scope RELEASE on gfx942 / gfx950 is `buffer_wbl2 sc1` -- a write-back of the WHOLE L2 of
// the XCD -- and was measured at 32 -> 94 us on the split runs (round 5); with the pruning scratch of round 6 dirty in L2 (21 MB per
// launch) it would cost more.  The `asm volatile("s_waitcnt vmcnt(0)" ::: "memory")` is both the hardware wait and the compiler
// barrier (no store may sink below it, no load of the counter may rise above it).  The assumption -- sc1 stores are visible to sc1
// loads of every XCD once vmcnt has drained -- is MI355X_MICROARCH.md's "valid forms" table; the library is built for gfx950 only:
#if defined(__HIP_DEVICE_COMPILE__) && !defined(__gfx950__)
#error "nn1_common.h: the relaxed-atomic + s_waitcnt hand-off between blocks is validated on gfx950 only (see the note above)"
#endif
struct FinalizeArgs {
    unsigned long long *pp;
    unsigned int *ticket;
    unsigned int nvalid;
    int B, stride, tiles_x, tiles_y;
    double *sums_out;
    float *loss_out;
    int N, M;
    long long Bg;
    float w1, w2;
};
__device__ __forceinline__ int fused_finalize_wave0(const FinalizeArgs &f, size_t slot, double tot, int lane) {
    int last = 0;
    if (lane == 0) {
        __hip_atomic_store(&f.pp[slot], __builtin_bit_cast(unsigned long long, tot), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        const unsigned int old = __hip_atomic_fetch_add(f.ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        last = old == f.nvalid - 1;
    }
    last = __builtin_amdgcn_readfirstlane(last);
    if (!last) return 0;
    // lane l sums entries l, l + 64, ... of a direction in order (four of each direction in flight), then the DPP tree
    double a[2] = {0.0, 0.0};
    const unsigned int n0 = (unsigned int)f.B * (unsigned int)f.tiles_x, n1 = (unsigned int)f.B * (unsigned int)f.tiles_y;  // (< 2^30: check_shapes)
    for (unsigned int k0 = lane; k0 < n0 || k0 < n1; k0 += 64 * 4) {
        unsigned long long v[2][4];
#pragma unroll
        for (int dd = 0; dd < 2; ++dd)
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const unsigned int nt = dd ? f.tiles_y : f.tiles_x;
                const unsigned int k = k0 + 64 * u, kc = k < (dd ? n1 : n0) ? k : 0;
                // (directions of equal tile counts -- the usual case -- : rows are dense, no division)
                const size_t e = nt == (unsigned int)f.stride ? (size_t)dd * f.B * f.stride + kc : ((size_t)(dd * f.B) + kc / nt) * f.stride + kc % nt;
                v[dd][u] = __hip_atomic_load(&f.pp[e], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
#pragma unroll
        for (int dd = 0; dd < 2; ++dd)
#pragma unroll
            for (int u = 0; u < 4; ++u)
                if (k0 + 64 * u < (dd ? n1 : n0)) a[dd] += __builtin_bit_cast(double, v[dd][u]);
    }
    const double t0 = wave_sum_l63_f64(a[0]), t1 = wave_sum_l63_f64(a[1]);
    if (lane == 63) {
        if (f.sums_out) { f.sums_out[0] = t0; f.sums_out[1] = t1; }
        if (f.loss_out) *f.loss_out = chamfer_loss_from_sums(t0, t1, f.N, f.M, 3, f.Bg, f.w1, f.w2);
        __hip_atomic_store(f.ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // ready for reuse
    }
    return 1;
}

}  // namespace fx3d
