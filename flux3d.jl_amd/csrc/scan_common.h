// Device-side primitives shared by the conversion kernels (voxel.hip, trimesh_voxel.hip, voxel_mesh.hip) and the topology
// builders (topology_dev.hip): the integer block scan, the single-block scan of a whole sequence and the scalar range of a
// cloud.  Integer sums and min / max are order-free, so none of them depends on the block size or on scheduling.  All threads
// of the block call them together (they synchronise).  The workspace layouts of the same files use WsBump (fx3d_common.h).
#pragma once
#include "fx3d_common.h"

namespace fx3d {

template <typename T>
__device__ __forceinline__ T block_exclusive_scan(T v, T *sw, T *total) {  // sw: blockDim.x / kWave values
    const int lane = threadIdx.x & (kWave - 1), w = threadIdx.x / kWave, nw = blockDim.x / kWave;
    T inc = v;
#pragma unroll
    for (int o = 1; o < kWave; o <<= 1) {
        const T u = __shfl_up(inc, o, kWave);
        if (lane >= o) inc += u;
    }
    if (lane == kWave - 1) sw[w] = inc;
    __syncthreads();
    T base = 0, tot = 0;
    for (int i = 0; i < nw; ++i) {
        const T x = sw[i];
        if (i < w) base += x;
        tot += x;
    }
    __syncthreads();  // sw is reused by the next call
    *total = tot;
    return base + inc - v;
}

// The same values with the wave totals folded by thread 0 alone (three barriers; *total in LDS, written by thread 0).  The
// 1024-thread kernels of trimesh_voxel.hip and voxel_mesh.hip stay on it: with sixteen waves reading the sixteen totals at once,
// block_exclusive_scan measured 0.3 - 1.0 us slower per launch there (profiles/conversions_refactor_time.txt).
__device__ __forceinline__ long long block_exclusive_scan_serial(long long v, long long *sw, long long *total) {
    const int lane = threadIdx.x & (kWave - 1), w = threadIdx.x / kWave;
    long long inc = v;
#pragma unroll
    for (int o = 1; o < kWave; o <<= 1) {
        const long long u = __shfl_up(inc, o, kWave);
        if (lane >= o) inc += u;
    }
    if (lane == kWave - 1) sw[w] = inc;
    __syncthreads();
    if (threadIdx.x == 0) {
        long long run = 0;
        for (int i = 0; i < (int)blockDim.x / kWave; ++i) {
            const long long x = sw[i];
            sw[i] = run;
            run += x;
        }
        *total = run;
    }
    __syncthreads();
    const long long r = sw[w] + inc - v;
    __syncthreads();  // sw / total are reused by the next call
    return r;
}

// One block of NT threads scans a whole sequence, NT entries a round: out[e] = the sum of load(0) .. load(e - 1), e = 0..n-1.
// Returns the sum of all n to every thread.  out may be the array load reads (each thread loads its entry before it writes it).
template <typename T, int NT, typename Load>
__device__ __forceinline__ T scan_entries(long long n, Load load, T *out, T *sw) {  // sw: NT / kWave values
    T carry = 0;
    for (long long base = 0; base < n; base += NT) {
        const long long e = base + threadIdx.x;
        T tot;
        const T ex = block_exclusive_scan<T>(e < n ? load(e) : T(0), sw, &tot);
        if (e < n) out[e] = carry + ex;
        carry += tot;
    }
    return carry;
}

// The scalar minimum and maximum of p[0, n) and whether any of them is a NaN (fminf / fmaxf skip NaNs: of n NaNs lo = +inf,
// hi = -inf, as of n = 0).  lo and hi are valid in thread 0, nan in every thread.  The sign of a zero minimum or maximum is
// that of whichever zero the order of the reduction meets last: callers must not let it reach an output.
struct Range {
    float lo, hi;
    bool nan;
};
template <int NT>  // the block's threads: a constant stride lets the compiler keep several loads of the one block in flight
__device__ __forceinline__ Range block_range(const float *__restrict__ p, int n, float *sw) {  // sw: 2 NT / kWave floats
    constexpr int nw = NT / kWave;
    float lo = __builtin_inff(), hi = -__builtin_inff();
    int nan = 0;
    for (int e = threadIdx.x; e < n; e += NT) {
        const float v = p[e];
        nan |= (v != v);
        lo = fminf(lo, v);
        hi = fmaxf(hi, v);
    }
    for (int o = kWave / 2; o > 0; o >>= 1) {
        lo = fminf(lo, __shfl_xor(lo, o, kWave));
        hi = fmaxf(hi, __shfl_xor(hi, o, kWave));
    }
    const int anynan = __syncthreads_or(nan);
    if ((threadIdx.x & (kWave - 1)) == 0) {
        sw[threadIdx.x / kWave] = lo;
        sw[nw + threadIdx.x / kWave] = hi;
    }
    __syncthreads();
    if (threadIdx.x == 0)
        for (int i = 1; i < nw; ++i) {
            lo = fminf(lo, sw[i]);
            hi = fmaxf(hi, sw[nw + i]);
        }
    return Range{lo, hi, anynan != 0};
}

}  // namespace fx3d
