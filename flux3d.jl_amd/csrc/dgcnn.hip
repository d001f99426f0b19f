// DGCNN inference (gfx950): (m::DGCNN)(X) of src/models/dgcnn.jl:113-147 in test mode, Float32, forward only.
// include/flux3d_hip.h ("DGCNN inference") states the network, the arithmetic and the parameter layout; this file is how they are
// computed.  The arithmetic is PointNet's (mlp_common.h): one accumulator per output element, walking the input channels
// upwards on v_mfma_f32_32x32x2_f32 (or v_fma_f32 for the 6-channel layer and the dense head); no contraction split over
// waves or blocks, no float atomics.
//
// Per forward: search, edgeconv<3>, search, edgeconv<64>, conv3, head.
//   neighbour search   fx3d_knn_ws on the cloud itself with the rank-0 hit dropped: coordinates, then the 64 features of x1.
//   dgcnn_edgeconv_kernel<F>: one block = 64 points of one cloud, 4 waves, looping over the neighbour rank k.  The
//     (K N, 2F, B) array the reference hands to its convolutions is never built: for each k the block gathers the 64 edge
//     rows [x_n, x_idx(k,n) - x_n] of its points straight into the LDS activation image (the x_n half once, before the loop),
//     runs the layer chain on it (conv_mfma from image to image), and folds the LAST layer -- never stored -- into a running
//     Julia max per (point, channel) held in registers: a lane owns one channel and 16 points per 32-point half, a wave the
//     slabs wave, wave + 4, ... of 32 channels (two slabs = 64 VGPRs at 256 channels).  After the last k the (C, N, B) slab
//     is written with plain stores.  The reference's reshape / MaxPool((K,)) / reshape / permute (:57-68) is exactly that
//     maximum over k (tests/test_dgcnn_host.py transcribes the array operations); the maximum is order-free.
//     F = 3:  rows of 6 in a small LDS array, conv 6 -> 32 as one v_fma_f32 chain per (point, channel), 32 -> 64, 64 -> 64 folded.
//     F = 64: rows of 128 in image A (stride kLd = 130), 128 -> 128 into image B, 128 -> 256 folded.
//     Rows beyond the cloud's last point are zeros: computed, never written.
//   dgcnn_conv3_kernel: one block = 64 points; the (64 x 256) tile of x2 in one LDS image (row stride 258 = 2 mod 64, the bank
//     pattern of kLd), conv 256 -> 1024 + BN + relu reduced to the tile's maximum per channel (conv_mfma<.., FINAL>).
//   dgcnn_head_kernel: one block per cloud folds the tile maxima (= MaxPool((npoints,))), then fc_4, fc_5 (dense, BN, relu),
//     fc_6 (dense, no activation) with one thread per output element, and the softmax.
#include "mlp_common.h"

using namespace fx3d;
using namespace fx3d::mlp;

namespace {

constexpr int kHeadThreads = 1024;
constexpr int kFeat = 1024;       // channels of conv_3 and of the pooled feature
constexpr int kLd3 = 258;         // LDS row stride of conv_3's 256-channel input image
constexpr int kMaxN = 36864;      // the neighbour search's general kernel holds a query's N distance keys in LDS
constexpr size_t kEdgeLds = (size_t)(2 * kTile * kLd + kTile * 6) * sizeof(float);
constexpr size_t kConv3Lds = (size_t)kTile * kLd3 * sizeof(float);

struct EdgeArgs {
    const float *x;      // (F, N, B)
    const int32_t *idx;  // (K, N, B), 0-based
    float *out;          // (C, N, B), C = 64 (F = 3) or 256 (F = 64)
    Conv c1, c2, c3;     // F = 3: 6 -> 32 -> 64 -> 64;  F = 64: 128 -> 128 -> 256 (c3 unused)
    int N, K;
};

// the last layer of an EdgeConv for the current k: rm[p][o] = jmax(rm[p][o], relu(BN(conv))) for the wave's slabs
template <int CIN, int NS>
__device__ __forceinline__ void conv_mfma_fold(const float *in, int cout, const Conv &c, f32x16 (&rm0)[NS], f32x16 (&rm1)[NS]) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, h = lane >> 5, j = lane & 31;
    const float *a0 = in + j * kLd + h, *a1 = a0 + 32 * kLd;
#pragma unroll
    for (int s = 0; s < NS; ++s) {
        const int sl = wave + s * (kPtThreads / 64);
        if (sl >= cout / 32) break;  // wave-uniform
        const int o = sl * 32 + j;
        f32x16 acc0 = {0}, acc1 = {0};
        mfma_slab<CIN>(a0, a1, c.W + (size_t)CIN * o, h, acc0, acc1);
        fold_slab(acc0, acc1, c, o, rm0[s], rm1[s]);
    }
}

template <int F>
__global__ __launch_bounds__(kPtThreads) void dgcnn_edgeconv_kernel(const EdgeArgs a) {
    constexpr int COUT = F == 3 ? 64 : 256;
    constexpr int NS = COUT >= 128 ? COUT / 128 : 1;  // slabs of 32 channels per wave
    extern __shared__ float lds[];
    float *bufA = lds, *bufB = lds + kTile * kLd, *es = bufB + kTile * kLd;  // es[p][6]: F = 3
    const int tile = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
    const int p0 = tile * kTile;
    const int nvalid = min(kTile, a.N - p0);
    const float *xb = a.x + (size_t)b * a.N * F;
    const int32_t *ib = a.idx + ((size_t)b * a.N + p0) * a.K;
    f32x16 rm0[NS], rm1[NS];
    fold_init<NS>(rm0, rm1);
    float *rows = F == 3 ? es : bufA;  // the edge rows: es[p][6] or image A's first 128 channels
    constexpr int ldr = F == 3 ? 6 : kLd;
    gather_centre<F>(rows, ldr, xb, F, p0, nvalid);  // x_n, the first half of every edge row of point n, whatever k
    __syncthreads();
    for (int k = 0; k < a.K; ++k) {
        gather_diff<F>(rows, ldr, xb, ib, F, a.N, a.K, k, p0, nvalid);  // x_idx(k, n) - x_n, the second half
        __syncthreads();
        if constexpr (F == 3) {
            for (int i = tid; i < kTile * 32; i += kPtThreads) {
                const int p = i >> 5, o = i & 31;
                const float *e = es + p * 6, *w = a.c1.W + 6 * o;
                float acc = 0.0f;
#pragma unroll
                for (int c = 0; c < 6; ++c) acc = fmaf(e[c], w[c], acc);
                bufA[p * kLd + o] = epilogue<kBnRelu>(acc, a.c1.b[o], a.c1.bn.g[o], a.c1.bn.b[o], a.c1.bn.m[o], sqrtf(a.c1.bn.v[o] + kBnEps));
            }
            __syncthreads();
            conv_mfma<32, kBnRelu, false>(bufA, bufB, 64, a.c2.W, a.c2.b, a.c2.bn, nvalid, nullptr);
            __syncthreads();
            conv_mfma_fold<64, NS>(bufB, COUT, a.c3, rm0, rm1);
        } else {
            conv_mfma<2 * F, kBnRelu, false>(bufA, bufB, 128, a.c1.W, a.c1.b, a.c1.bn, nvalid, nullptr);
            __syncthreads();
            conv_mfma_fold<128, NS>(bufB, COUT, a.c2, rm0, rm1);
        }
        // the next k's writes: es / image A's second half were last read before the barrier above; image B is written again only
        // after the barrier that follows the next gather, which a wave reaches after its fold
    }
    fold_store<NS>(a.out + ((size_t)b * a.N + p0) * COUT, COUT, nvalid, rm0, rm1);
}

__global__ __launch_bounds__(kPtThreads) void dgcnn_conv3_kernel(const float *__restrict__ x2, const Conv c, float *__restrict__ tmax_all,
                                                                 int N, int ntiles) {
    extern __shared__ float lds[];
    const int tile = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
    const int p0 = tile * kTile;
    const int nvalid = min(kTile, N - p0);
    const float *xb = x2 + ((size_t)b * N + p0) * 256;
    for (int i = tid; i < kTile * 256; i += kPtThreads) lds[(i >> 8) * kLd3 + (i & 255)] = i < nvalid * 256 ? xb[i] : 0.0f;
    __syncthreads();
    conv_mfma<256, kBnRelu, true, kLd3>(lds, nullptr, kFeat, c.W, c.b, c.bn, nvalid, tmax_all + ((size_t)b * ntiles + tile) * kFeat);
}

struct HeadArgs {
    const float *tmax;  // (1024, ntiles, B)
    int ntiles;
    Dense d4, d5, d6;   // 1024 -> 512, 512 -> 256, 256 -> nc
    Bn bn4, bn5;
    int nc;
    float *pooled;          // optional: (1024, B)
    float *logits, *probs;  // (nc, B) each; logits is the caller's array or the workspace
};

__global__ __launch_bounds__(kHeadThreads) void dgcnn_head_kernel(const HeadArgs a) {
    __shared__ float v0[kFeat], v1[512], v2[256];
    const int b = blockIdx.x, tid = threadIdx.x;
    {
        const float *t = a.tmax + (size_t)b * a.ntiles * kFeat + tid;
        float m = t[0];
        for (int k = 1; k < a.ntiles; ++k) m = jmax(m, t[(size_t)k * kFeat]);
        v0[tid] = m;
        if (a.pooled) a.pooled[(size_t)b * kFeat + tid] = m;
    }
    __syncthreads();
    if (tid < 512) {
        const float v = dense_chain(v0, kFeat, a.d4.W, 512, tid) + a.d4.b[tid];
        v1[tid] = relu(batchnorm(v, a.bn4.g[tid], a.bn4.b[tid], a.bn4.m[tid], sqrtf(a.bn4.v[tid] + kBnEps)));
    }
    __syncthreads();
    if (tid < 256) {
        const float v = dense_chain(v1, 512, a.d5.W, 256, tid) + a.d5.b[tid];
        v2[tid] = relu(batchnorm(v, a.bn5.g[tid], a.bn5.b[tid], a.bn5.m[tid], sqrtf(a.bn5.v[tid] + kBnEps)));
    }
    __syncthreads();
    float *z = a.logits + (size_t)b * a.nc, *pr = a.probs + (size_t)b * a.nc;
    for (int o = tid; o < a.nc; o += kHeadThreads) z[o] = dense_chain(v2, 256, a.d6.W, a.nc, o) + a.d6.b[o];
    __syncthreads();  // the block's logits are in memory
    __shared__ float zmax, esum;
    if (tid == 0) {
        float m = z[0];
        for (int i = 1; i < a.nc; ++i) m = jmax(m, z[i]);
        zmax = m;
    }
    __syncthreads();
    for (int o = tid; o < a.nc; o += kHeadThreads) pr[o] = expf(z[o] - zmax);
    __syncthreads();
    if (tid == 0) {
        float s = 0.0f;
        for (int i = 0; i < a.nc; ++i) s = s + pr[i];  // in class order
        esum = s;
    }
    __syncthreads();
    for (int o = tid; o < a.nc; o += kHeadThreads) pr[o] = pr[o] / esum;
}

// ---- the flat parameter buffer in forward order (flux3d_hip.h) ----------------------------------------------------------
struct Net {
    Conv e1c1, e1c2, e1c3, e2c1, e2c2, c3;
    Dense d4, d5, d6;
    Bn bn4, bn5;
    long long count;
};

Net layout(const float *params, int num_classes) {
    Cursor c{params, 0};
    Net n;
    n.e1c1 = c.conv(6, 32);     n.e1c1.bn = c.bn(32);
    n.e1c2 = c.conv(32, 64);    n.e1c2.bn = c.bn(64);
    n.e1c3 = c.conv(64, 64);    n.e1c3.bn = c.bn(64);
    n.e2c1 = c.conv(128, 128);  n.e2c1.bn = c.bn(128);
    n.e2c2 = c.conv(128, 256);  n.e2c2.bn = c.bn(256);
    n.c3 = c.conv(256, kFeat);  n.c3.bn = c.bn(kFeat);
    n.d4 = c.dense(kFeat, 512); n.bn4 = c.bn(512);
    n.d5 = c.dense(512, 256);   n.bn5 = c.bn(256);
    n.d6 = c.dense(256, num_classes);
    n.count = c.at;
    return n;
}

fx3d_status check_sizes(const char *fn, int32_t N, int32_t B, int32_t K, int32_t nc) {
    FX3D_REQUIRE(nc >= 1 && nc <= (1 << 20), "%s: num_classes must be in [1, 2^20], got %d", fn, nc);
    FX3D_REQUIRE(N >= 1 && B >= 1, "%s: N and B must be positive, got N=%d B=%d", fn, N, B);
    FX3D_REQUIRE(K >= 1, "%s: K must be positive, got %d", fn, K);
    FX3D_REQUIRE((long long)K + 1 <= N, "%s: K + 1 = %lld neighbours (the point itself is dropped) of N = %d points", fn, (long long)K + 1, N);
    FX3D_REQUIRE(N <= kMaxN, "%s: N must be at most %d (the neighbour search), got %d", fn, kMaxN, N);
    FX3D_REQUIRE(B <= 65535, "%s: B must be at most 65535, got %d", fn, B);
    FX3D_REQUIRE((long long)N * B * K <= (1ll << 31), "%s: N * B * K must be at most 2^31, got %lld", fn, (long long)N * B * K);
    return FX3D_OK;
}

// the workspace: idx1 (K, N, B) | x1 (64, N, B) | idx2 (K, N, B) | x2 (256, N, B) | per-tile maxima (1024, ntiles, B) |
// logits (num_classes, B) | the neighbour search's scratch (the larger of the two searches')
struct WsPlan { size_t idx1, x1, idx2, x2, tmax, logits, knn, knn_bytes, total; int ntiles; };
fx3d_status ws_plan(int N, int B, int K, int nc, WsPlan *w) {
    w->ntiles = (N + kTile - 1) / kTile;
    size_t at = 0;
    auto put = [&](size_t bytes) { const size_t o = at; at += (bytes + 255) & ~(size_t)255; return o; };
    w->idx1 = put((size_t)K * N * B * sizeof(int32_t));
    w->x1 = put((size_t)64 * N * B * sizeof(float));
    w->idx2 = put((size_t)K * N * B * sizeof(int32_t));
    w->x2 = put((size_t)256 * N * B * sizeof(float));
    w->tmax = put((size_t)kFeat * w->ntiles * B * sizeof(float));
    w->logits = put((size_t)nc * B * sizeof(float));
    size_t k3 = 0, k64 = 0;
    fx3d_status rc;
    if ((rc = fx3d_knn_workspace_bytes(N, N, B, 3, K, 1, &k3)) != FX3D_OK) return rc;
    if ((rc = fx3d_knn_workspace_bytes(N, N, B, 64, K, 1, &k64)) != FX3D_OK) return rc;
    w->knn_bytes = k3 > k64 ? k3 : k64;
    w->knn = put(w->knn_bytes);
    w->total = at;
    return FX3D_OK;
}

template <int F>
fx3d_status launch_edgeconv(const EdgeArgs &a, int ntiles, int B, hipStream_t st) {
    const fx3d_status rc = ensure_dynamic_lds(reinterpret_cast<const void *>(&dgcnn_edgeconv_kernel<F>), (int)kEdgeLds, "dgcnn_edgeconv_kernel");
    if (rc != FX3D_OK) return rc;
    ProfileScope prof(F == 3 ? "dgcnn_edgeconv1" : "dgcnn_edgeconv2", st);
    hipLaunchKernelGGL(dgcnn_edgeconv_kernel<F>, dim3(ntiles, B), dim3(kPtThreads), kEdgeLds, st, a);
    FX3D_LAUNCH_CHECK();
    return FX3D_OK;
}

}  // namespace

extern "C" {

fx3d_status fx3d_dgcnn_param_count(int32_t num_classes, int64_t *count) {
    FX3D_REQUIRE(count != nullptr, "fx3d_dgcnn_param_count: count is NULL");
    FX3D_REQUIRE(num_classes >= 1 && num_classes <= (1 << 20), "fx3d_dgcnn_param_count: num_classes must be in [1, 2^20], got %d", num_classes);
    *count = layout(nullptr, num_classes).count;
    return FX3D_OK;
}

fx3d_status fx3d_dgcnn_workspace_bytes(int32_t N, int32_t B, int32_t K, int32_t num_classes, size_t *bytes) {
    FX3D_REQUIRE(bytes != nullptr, "fx3d_dgcnn_workspace_bytes: bytes is NULL");
    fx3d_status rc = check_sizes("fx3d_dgcnn_workspace_bytes", N, B, K, num_classes);
    if (rc != FX3D_OK) return rc;
    WsPlan w;
    if ((rc = ws_plan(N, B, K, num_classes, &w)) != FX3D_OK) return rc;
    *bytes = w.total;
    return FX3D_OK;
}

fx3d_status fx3d_dgcnn_forward(const float *params_dev, int32_t num_classes, int32_t K, const float *x, int32_t N, int32_t B,
                               float *probs, float *logits, int32_t *idx1, float *x1, int32_t *idx2, float *x2, float *pooled,
                               void *ws, size_t ws_bytes, fx3d_stream_t s) {
    const char *fn = "fx3d_dgcnn_forward";
    FX3D_REQUIRE(params_dev && x && probs && ws, "%s: params_dev, x, probs and ws must not be NULL", fn);
    fx3d_status r = check_sizes(fn, N, B, K, num_classes);
    if (r != FX3D_OK) return r;
    WsPlan w;
    if ((r = ws_plan(N, B, K, num_classes, &w)) != FX3D_OK) return r;
    FX3D_REQUIRE(ws_bytes >= w.total, "%s: workspace of %zu bytes, fx3d_dgcnn_workspace_bytes says %zu", fn, ws_bytes, w.total);
    FX3D_REQUIRE((reinterpret_cast<uintptr_t>(ws) & 255) == 0, "%s: ws must be 256-byte aligned", fn);
    FX3D_REQUIRE(!x1 || (reinterpret_cast<uintptr_t>(x1) & 15) == 0, "%s: x1 must be 16-byte aligned", fn);
    const Net n = layout(params_dev, num_classes);
    hipStream_t st = as_stream(s);
    char *wsb = static_cast<char *>(ws);
    int32_t *i1 = idx1 ? idx1 : reinterpret_cast<int32_t *>(wsb + w.idx1), *i2 = idx2 ? idx2 : reinterpret_cast<int32_t *>(wsb + w.idx2);
    float *f1 = x1 ? x1 : reinterpret_cast<float *>(wsb + w.x1), *f2 = x2 ? x2 : reinterpret_cast<float *>(wsb + w.x2);
    float *tmax = reinterpret_cast<float *>(wsb + w.tmax);
    float *lg = logits ? logits : reinterpret_cast<float *>(wsb + w.logits);
    void *kws = w.knn_bytes ? wsb + w.knn : nullptr;

    // EdgeConv1: neighbours in coordinate space
    if ((r = fx3d_knn_ws(x, N, x, N, B, 3, K, 1, i1, nullptr, kws, w.knn_bytes, s)) != FX3D_OK) return r;
    EdgeArgs e{};
    e.x = x; e.idx = i1; e.out = f1; e.c1 = n.e1c1; e.c2 = n.e1c2; e.c3 = n.e1c3; e.N = N; e.K = K;
    if ((r = launch_edgeconv<3>(e, w.ntiles, B, st)) != FX3D_OK) return r;
    // EdgeConv2: neighbours in the space of x1's 64 features
    if ((r = fx3d_knn_ws(f1, N, f1, N, B, 64, K, 1, i2, nullptr, kws, w.knn_bytes, s)) != FX3D_OK) return r;
    e.x = f1; e.idx = i2; e.out = f2; e.c1 = n.e2c1; e.c2 = n.e2c2; e.c3 = Conv{};
    if ((r = launch_edgeconv<64>(e, w.ntiles, B, st)) != FX3D_OK) return r;
    // conv_3 + the maximum over the points, per tile
    if ((r = ensure_dynamic_lds(reinterpret_cast<const void *>(&dgcnn_conv3_kernel), (int)kConv3Lds, "dgcnn_conv3_kernel")) != FX3D_OK) return r;
    {
        ProfileScope prof("dgcnn_conv3", st);
        hipLaunchKernelGGL(dgcnn_conv3_kernel, dim3(w.ntiles, B), dim3(kPtThreads), kConv3Lds, st, f2, n.c3, tmax, N, w.ntiles);
        FX3D_LAUNCH_CHECK();
    }
    HeadArgs hd{};
    hd.tmax = tmax; hd.ntiles = w.ntiles;
    hd.d4 = n.d4; hd.bn4 = n.bn4; hd.d5 = n.d5; hd.bn5 = n.bn5; hd.d6 = n.d6;
    hd.nc = num_classes; hd.pooled = pooled; hd.logits = lg; hd.probs = probs;
    ProfileScope prof("dgcnn_head", st);
    hipLaunchKernelGGL(dgcnn_head_kernel, dim3(B), dim3(kHeadThreads), 0, st, hd);
    FX3D_LAUNCH_CHECK();
    return FX3D_OK;
}

}  // extern "C"
