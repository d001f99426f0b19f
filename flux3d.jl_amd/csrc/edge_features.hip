// EdgeConv's graph features (src/models/dgcnn.jl:3-9, 32-51): the gather X[:, idx], cat(X, KNN - X) + permute for any F, and the
// @nograd adjoint -- what follows the neighbour search of knn.hip (whose fx3d_edgeconv_graph calls fx3d_edge_features; F = 3 is
// written by the search kernel itself, knn_d3.hip).
#include "fx3d_common.h"

using namespace fx3d;

namespace {

constexpr int kThreads = 256;
typedef float f32x4v __attribute__((ext_vector_type(4)));

// out[(((b*N+i)*k + r)*F + f] = x[(b*N + idx[(b*N+i)*k + r])*F + f]
__global__ __launch_bounds__(kThreads) void knn_gather_kernel(const float *__restrict__ x, int N, int B,
                                                              int F, int k,
                                                              const int32_t *__restrict__ idx,
                                                              float *__restrict__ out) {
    const long long total = (long long)B * N * k * F;
    for (long long e = (long long)blockIdx.x * kThreads + threadIdx.x; e < total;
         e += (long long)gridDim.x * kThreads) {
        const long long row = e / F;  // (b*N+i)*k + r
        const int f = (int)(e - row * F);
        const long long bn = row / k;
        const int b = (int)(bn / N);
        const int j = idx[row];
        out[e] = x[((size_t)b * N + j) * F + f];
    }
}

// knn_gather_kernel with 16-byte elements (F4 = F/4 float4 per row)
// NT: streaming (non-temporal) stores for tensors beyond the caches (round 4: the F = 64 feature build gained 28 % from them).
// Only for outputs larger than 3/4 of the 256 MB Infinity Cache: a consumer kernel may still find a smaller tensor there (the
// 168 MB gather of C4' gains 3 % from streaming stores -- not worth taking that away from its reader).
constexpr size_t kStreamingStoreBytes = (size_t)192 << 20;
template <bool NT>
__global__ __launch_bounds__(kThreads) void knn_gather4_kernel(const float *__restrict__ x, int N, int B, int F4, int k,
                                                               const int32_t *__restrict__ idx, float *__restrict__ out) {
    const long long total = (long long)B * N * k * F4;
    const f32x4v *x4 = reinterpret_cast<const f32x4v *>(x);
    f32x4v *o4 = reinterpret_cast<f32x4v *>(out);
    for (long long e = (long long)blockIdx.x * kThreads + threadIdx.x; e < total;
         e += (long long)gridDim.x * kThreads) {
        const long long row = e / F4;  // (b*N+i)*k + r
        const int f = (int)(e - row * F4);
        const int b = (int)(row / k / N);
        const f32x4v v = x4[((size_t)b * N + idx[row]) * F4 + f];
        if (NT) __builtin_nontemporal_store(v, o4 + e);
        else o4[e] = v;
    }
}

// ---- EdgeConv graph features (src/models/dgcnn.jl:36-51): cat(X, KNNGraph - X, dims=1) in one pass --------
// layout 0: out (2F,K,N,B) as the reference holds it after `cat(..., dims = 1)` (:45)
__global__ __launch_bounds__(kThreads) void edge_features_cat_kernel(const float *__restrict__ x, int N, int B,
                                                                     int F, int k,
                                                                     const int32_t *__restrict__ idx,
                                                                     float *__restrict__ out) {
    const long long total = (long long)B * N * k * 2 * F;
    const int F2 = 2 * F;
    for (long long e = (long long)blockIdx.x * kThreads + threadIdx.x; e < total;
         e += (long long)gridDim.x * kThreads) {
        const long long row = e / F2;  // (b*N+i)*k + r
        const int f = (int)(e - row * F2);
        const long long bn = row / k;  // b*N + i
        if (f < F) {
            out[e] = x[(size_t)bn * F + f];
        } else {
            const int b = (int)(bn / N);
            const int j = idx[row];
            out[e] = x[((size_t)b * N + j) * F + (f - F)] - x[(size_t)bn * F + (f - F)];
        }
    }
}

// layout 1: out (K*N, 2F, B), what reaches the 1x1 conv after PermutedDimsArray + reshape (:48-51).
// One thread per (r,i) position (the contiguous dimension of the output), looping over features, so every
// feature row is written with unit stride; the two source rows are read as float4 when F % 4 == 0.
template <bool VEC4>
__global__ __launch_bounds__(kThreads) void edge_features_mlp_kernel(const float *__restrict__ x, int N, int B,
                                                                     int F, int k,
                                                                     const int32_t *__restrict__ idx,
                                                                     float *__restrict__ out) {
    const int b = blockIdx.y;
    const long long KN = (long long)k * N;
    const long long e = (long long)blockIdx.x * kThreads + threadIdx.x;  // i*k + r
    if (e >= KN) return;
    const int i = (int)(e / k);
    const int j = idx[(size_t)b * KN + e];
    const float *xi = x + ((size_t)b * N + i) * F;
    const float *xj = x + ((size_t)b * N + j) * F;
    float *o = out + (size_t)b * 2 * F * KN + e;
    if (VEC4) {
        for (int f = 0; f < F; f += 4) {
            const float4 a = *reinterpret_cast<const float4 *>(xi + f);
            const float4 c = *reinterpret_cast<const float4 *>(xj + f);
            o[(size_t)(f + 0) * KN] = a.x;
            o[(size_t)(f + 1) * KN] = a.y;
            o[(size_t)(f + 2) * KN] = a.z;
            o[(size_t)(f + 3) * KN] = a.w;
            o[(size_t)(F + f + 0) * KN] = c.x - a.x;
            o[(size_t)(F + f + 1) * KN] = c.y - a.y;
            o[(size_t)(F + f + 2) * KN] = c.z - a.z;
            o[(size_t)(F + f + 3) * KN] = c.w - a.w;
        }
    } else {
        for (int f = 0; f < F; ++f) {
            const float a = xi[f];
            o[(size_t)f * KN] = a;
            o[(size_t)(F + f) * KN] = xj[f] - a;
        }
    }
}

// Same, four consecutive (r,i) positions per thread: the 4 x 4 block (4 positions x 4 features) is read as
// float4 along the features and written as float4 along the positions -- every store is 16 bytes, a wave writes
// 1 KiB runs.  Needs F % 4 == 0, (k*N) % 4 == 0 and 16-byte aligned x / out.
// Round 4: blockIdx.z splits the feature loop (fper features per block) -- F = 64 at C4' is 335 MB written by what used to be 640
// blocks (2.5 per CU, ten waves per CU, each a serial loop of load -> 8 stores); the write stream wants many more waves in
// flight (tools/ubench_hbm.hip: 4.7 TB/s from 2048 blocks, 6.1 from 32768) -- and NT selects streaming (non-temporal) stores:
// the tensor is larger than the Infinity Cache and nobody reads it back inside the launch.
template <bool NT>
__global__ __launch_bounds__(kThreads) void edge_features_mlp4_kernel(const float *__restrict__ x, int N, int B,
                                                                      int F, int k,
                                                                      const int32_t *__restrict__ idx,
                                                                      float *__restrict__ out, int fper) {
    const int b = blockIdx.y;
    const long long KN = (long long)k * N;
    const long long e0 = ((long long)blockIdx.x * kThreads + threadIdx.x) * 4;  // i*k + r of the first position
    if (e0 >= KN) return;
    const int f_lo = blockIdx.z * fper, f_hi = f_lo + fper < F ? f_lo + fper : F;
    const int4 jj = *reinterpret_cast<const int4 *>(idx + (size_t)b * KN + e0);
    const float *xb = x + (size_t)b * N * F;
    const float *xi0 = xb + (size_t)(e0 / k) * F, *xi1 = xb + (size_t)((e0 + 1) / k) * F;
    const float *xi2 = xb + (size_t)((e0 + 2) / k) * F, *xi3 = xb + (size_t)((e0 + 3) / k) * F;
    const float *xj0 = xb + (size_t)jj.x * F, *xj1 = xb + (size_t)jj.y * F, *xj2 = xb + (size_t)jj.z * F,
                *xj3 = xb + (size_t)jj.w * F;
    float *o = out + (size_t)b * 2 * F * KN + e0;
    auto put = [](float *p, const f32x4v &v) {
        if (NT) __builtin_nontemporal_store(v, reinterpret_cast<f32x4v *>(p));
        else *reinterpret_cast<f32x4v *>(p) = v;
    };
    for (int f = f_lo; f < f_hi; f += 4) {
        const float4 a0 = *reinterpret_cast<const float4 *>(xi0 + f), a1 = *reinterpret_cast<const float4 *>(xi1 + f);
        const float4 a2 = *reinterpret_cast<const float4 *>(xi2 + f), a3 = *reinterpret_cast<const float4 *>(xi3 + f);
        const float4 c0 = *reinterpret_cast<const float4 *>(xj0 + f), c1 = *reinterpret_cast<const float4 *>(xj1 + f);
        const float4 c2 = *reinterpret_cast<const float4 *>(xj2 + f), c3 = *reinterpret_cast<const float4 *>(xj3 + f);
        put(o + (size_t)(f + 0) * KN, f32x4v{a0.x, a1.x, a2.x, a3.x});
        put(o + (size_t)(f + 1) * KN, f32x4v{a0.y, a1.y, a2.y, a3.y});
        put(o + (size_t)(f + 2) * KN, f32x4v{a0.z, a1.z, a2.z, a3.z});
        put(o + (size_t)(f + 3) * KN, f32x4v{a0.w, a1.w, a2.w, a3.w});
        put(o + (size_t)(F + f + 0) * KN, f32x4v{c0.x - a0.x, c1.x - a1.x, c2.x - a2.x, c3.x - a3.x});
        put(o + (size_t)(F + f + 1) * KN, f32x4v{c0.y - a0.y, c1.y - a1.y, c2.y - a2.y, c3.y - a3.y});
        put(o + (size_t)(F + f + 2) * KN, f32x4v{c0.z - a0.z, c1.z - a1.z, c2.z - a2.z, c3.z - a3.z});
        put(o + (size_t)(F + f + 3) * KN, f32x4v{c0.w - a0.w, c1.w - a1.w, c2.w - a2.w, c3.w - a3.w});
    }
}

// Adjoint w.r.t. X.  CreateSingleKNNGraph is @nograd (src/models/dgcnn.jl:9), so the gathered neighbours are
// constants and dX[f,i,b] = sum_r (g[f,r,i,b] - g[F+f,r,i,b]), accumulated in rank order.
__global__ __launch_bounds__(kThreads) void edge_features_bwd_kernel(const float *__restrict__ g, int N, int B, int F,
                                                                     int k, int layout, float *__restrict__ gx) {
    const long long total = (long long)B * N * F;
    const long long KN = (long long)k * N;
    for (long long e = (long long)blockIdx.x * kThreads + threadIdx.x; e < total;
         e += (long long)gridDim.x * kThreads) {
        long long bn;
        int f;
        if (layout == 0) {  // consecutive threads -> consecutive f (reads stride 1 in f)
            bn = e / F;
            f = (int)(e - bn * F);
        } else {            // consecutive threads -> consecutive i (reads k-float runs)
            const long long bf = e / N;
            const int i = (int)(e - bf * N);
            const int b = (int)(bf / F);
            f = (int)(bf - (long long)b * F);
            bn = (long long)b * N + i;
        }
        const int b = (int)(bn / N);
        const int i = (int)(bn - (long long)b * N);
        float acc = 0.0f;
        for (int r = 0; r < k; ++r) {
            float a, c;
            if (layout == 0) {
                const size_t base = ((size_t)bn * k + r) * 2 * F;
                a = g[base + f];
                c = g[base + F + f];
            } else {
                const size_t base = (size_t)b * 2 * F * KN + (size_t)i * k + r;
                a = g[base + (size_t)f * KN];
                c = g[base + (size_t)(F + f) * KN];
            }
            acc = acc + (a - c);
        }
        gx[(size_t)bn * F + f] = acc;
    }
}

}  // namespace

extern "C" {

fx3d_status fx3d_knn_gather(const float *x, int32_t N, int32_t B, int32_t F, int32_t k,
                            const int32_t *idx, float *out, fx3d_stream_t s) {
    FX3D_REQUIRE(x && idx && out, "fx3d_knn_gather: null pointer");
    FX3D_REQUIRE(N > 0 && B > 0 && F > 0 && k > 0, "fx3d_knn_gather: bad sizes");
    if (F % 4 == 0 && (((uintptr_t)x | (uintptr_t)out) & 15) == 0) {  // 16-byte copies
        const long long total4 = (long long)B * N * k * (F / 4);
        long long g4 = (total4 + kThreads - 1) / kThreads;
        if (g4 > 16384) g4 = 16384;
        ProfileScope prof4("knn_gather", as_stream(s));
        if ((size_t)F * k * N * B * 4 > kStreamingStoreBytes)
            hipLaunchKernelGGL(knn_gather4_kernel<true>, dim3((unsigned)g4), dim3(kThreads), 0, as_stream(s), x, N, B, F / 4, k, idx, out);
        else
            hipLaunchKernelGGL(knn_gather4_kernel<false>, dim3((unsigned)g4), dim3(kThreads), 0, as_stream(s), x, N, B, F / 4, k, idx, out);
        FX3D_LAUNCH_CHECK();
        return FX3D_OK;
    }
    const long long total = (long long)B * N * k * F;
    long long g = (total + kThreads - 1) / kThreads;
    if (g > 8192) g = 8192;
    ProfileScope prof("knn_gather", as_stream(s));
    hipLaunchKernelGGL(knn_gather_kernel, dim3((unsigned)g), dim3(kThreads), 0, as_stream(s), x, N, B, F, k, idx, out);
    FX3D_LAUNCH_CHECK();
    return FX3D_OK;
}


fx3d_status fx3d_edge_features(const float *x, int32_t N, int32_t B, int32_t F, int32_t k, const int32_t *idx,
                               int32_t layout, float *out, fx3d_stream_t s) {
    FX3D_REQUIRE(x && idx && out, "fx3d_edge_features: null pointer");
    FX3D_REQUIRE(N > 0 && B > 0 && F > 0 && k > 0, "fx3d_edge_features: bad sizes");
    FX3D_REQUIRE(layout == 0 || layout == 1, "fx3d_edge_features: layout must be 0 (2F,K,N,B) or 1 (K*N,2F,B)");
    if (layout == 1) FX3D_REQUIRE_GRID_Y("fx3d_edge_features", B, 1);  // (the layout-1 kernels take the cloud from blockIdx.y)
    ProfileScope prof("edge_features", as_stream(s));
    if (layout == 0) {
        const long long total = (long long)B * N * k * 2 * F;
        long long g = (total + kThreads - 1) / kThreads;
        if (g > 16384) g = 16384;
        hipLaunchKernelGGL(edge_features_cat_kernel, dim3((unsigned)g), dim3(kThreads), 0, as_stream(s), x, N, B, F, k,
                           idx, out);
    } else {
        const long long KN = (long long)k * N;
        dim3 grid((unsigned)((KN + kThreads - 1) / kThreads), B);
        const bool al16 = (((uintptr_t)x | (uintptr_t)out | (uintptr_t)idx) & 15) == 0;
        if (F % 4 == 0 && KN % 4 == 0 && al16) {
            // the feature loop split over blockIdx.z until the grid holds ~16 blocks per CU
            const long long gx = (KN / 4 + kThreads - 1) / kThreads;
            int fper = F;
            while (fper > 4 && gx * B * ((F + fper - 1) / fper) < 16ll * device_cus()) fper = (fper / 2 + 3) / 4 * 4;
            const unsigned gz = (unsigned)((F + fper - 1) / fper);
            const bool nt = (size_t)2 * F * KN * B * 4 > kStreamingStoreBytes;  // (smaller tensors may be read back from the caches)
            if (nt)
                hipLaunchKernelGGL(edge_features_mlp4_kernel<true>, dim3((unsigned)gx, B, gz), dim3(kThreads), 0, as_stream(s), x, N, B, F, k, idx, out, fper);
            else
                hipLaunchKernelGGL(edge_features_mlp4_kernel<false>, dim3((unsigned)gx, B, gz), dim3(kThreads), 0, as_stream(s), x, N, B, F, k, idx, out, fper);
        }
        else if (F % 4 == 0 && ((uintptr_t)x & 15) == 0)
            hipLaunchKernelGGL(edge_features_mlp_kernel<true>, grid, dim3(kThreads), 0, as_stream(s), x, N, B, F, k, idx, out);
        else
            hipLaunchKernelGGL(edge_features_mlp_kernel<false>, grid, dim3(kThreads), 0, as_stream(s), x, N, B, F, k, idx, out);
    }
    FX3D_LAUNCH_CHECK();
    return FX3D_OK;
}

fx3d_status fx3d_edge_features_bwd(const float *gout, int32_t N, int32_t B, int32_t F, int32_t k, int32_t layout,
                                   float *gx, fx3d_stream_t s) {
    FX3D_REQUIRE(gout && gx, "fx3d_edge_features_bwd: null pointer");
    FX3D_REQUIRE(N > 0 && B > 0 && F > 0 && k > 0, "fx3d_edge_features_bwd: bad sizes");
    FX3D_REQUIRE(layout == 0 || layout == 1, "fx3d_edge_features_bwd: bad layout");
    const long long total = (long long)B * N * F;
    long long g = (total + kThreads - 1) / kThreads;
    if (g > 16384) g = 16384;
    hipLaunchKernelGGL(edge_features_bwd_kernel, dim3((unsigned)g), dim3(kThreads), 0, as_stream(s), gout, N, B, F, k,
                       layout, gx);
    FX3D_LAUNCH_CHECK();
    return FX3D_OK;
}

}  // extern "C"
