// PointNet inference (gfx950): (m::PointNet)(X) of src/models/pointnet.jl:62-85 in test mode, Float32: the forward (pointnet_grad.hip: its adjoint).
// include/flux3d_hip.h states the network, the arithmetic and the parameter layout; this file is how they are computed.
//
// Every contraction is one accumulator per output element that walks the input channels upwards with one rounding per
// step: acc = fmaf(x[c], W[c,o], acc) from +0.0f.  v_mfma_f32_32x32x2_f32 is that chain (two steps per instruction, the
// lower k first), so the 1x1 convolutions with 64 or 128 input channels run on it; the 3-channel ones (no multiple of the
// instruction's k: padding with zeros would turn an Inf weight into NaN) and the dense heads run the same chain as v_fma_f32.
// No split of a contraction over waves or blocks, no float atomics: the bits do not depend on the launch shape.
//
// Two kernels, three rounds (stn, fstn, feat):
//   pointnet_points_kernel<MODE>: one block = 64 points of one cloud, 4 waves.  The tile's activations live in two
//     (64 x 128) LDS images (row stride 130 floats: the A-operand reads of a 32-point tile fall on 64 distinct banks; the
//     epilogue's stores, 32 consecutive channels per lane half with the halves 4 rows = 8 banks apart, overlap on 24 banks).  A wave owns slabs of 32 output channels and computes them for both 32-point halves of the tile from
//     one stream of weights: lane (h, j) reads row j of the slab, W[4q .. 4q+3, o] per step (the (Cin, Cout) column-major
//     layout makes that 16 contiguous bytes), and feeds elements h and 2 + h to two consecutive k-steps.  The epilogue
//     (bias, relu, BatchNorm in the order of the layer) runs on the accumulators: a lane holds ONE channel and 16 points
//     per half.  The last layer (128 -> 1024) is never stored: each slab is reduced to the tile's maximum per channel
//     (Julia's max) and written to the workspace with plain stores.
//     MODE 0 = stn (X -> 64 -> 128 -> 1024), 1 = fstn (X * T -> conv_block1 -> stored as h (64, N, B) -> 64 -> 128 -> 1024),
//     2 = feat (h * F -> 128 -> 1024, no relu on the last).
//   pointnet_head_kernel<FEAT>: one block per cloud folds the per-tile maxima, then the dense layers with one thread per
//     output element (W (out, in) column-major: consecutive threads read consecutive weights), BatchNorm, and for the
//     classifier relu + softmax.  stn / fstn write their (K, K) matrix already transposed (T[i,j] = d[j + K i] at i + K j),
//     which is the (Cin, Cout) layout of a convolution: the per-cloud transform is one more bias-free layer of the point kernel.
#include "pointnet_net.h"

using namespace fx3d;
using namespace fx3d::mlp;
using namespace fx3d::mlp::pointnet;

namespace {

// the round's last layer (128 -> 1024), reduced to the tile's maxima
template <int EPI, bool WIN>
__device__ __forceinline__ void last_layer(const PointArgs &a, const float *in, int nvalid, int p0, float *tmax) {
    if (WIN) {
        const size_t at = tmax - a.tmax;
        conv_final_win<EPI>(in, a.c3.W, a.c3.b, a.c3.bn, nvalid, p0, tmax, a.tfirst + at, a.tpre + at);
    } else {
        conv_mfma<128, EPI, true>(in, nullptr, kFeat, a.c3.W, a.c3.b, a.c3.bn, nvalid, tmax);
    }
}

// WIN: the adjoint's instantiation (pointnet_grad.hip), whose last layer also writes the tile's winners (conv_final_win)
template <int MODE, bool WIN>
__global__ __launch_bounds__(kPtThreads) void pointnet_points_kernel(const PointArgs a) {
    extern __shared__ float lds[];
    float *bufA = lds, *bufB = lds + kTile * kLd, *xs = bufB + kTile * kLd, *xt = xs + kTile * 3;
    const int tile = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
    const int p0 = tile * kTile;
    const int nvalid = min(kTile, a.N - p0);
    float *tmax = a.tmax + ((size_t)b * a.ntiles + tile) * kFeat;
    // rows beyond the cloud's last point are zeros: they are computed and take part in nothing
    if (MODE != 2) {
        const float *xb = a.x + ((size_t)b * a.N + p0) * 3;
        for (int i = tid; i < kTile * 3; i += kPtThreads) xs[i] = i < nvalid * 3 ? xb[i] : 0.0f;
    } else {
        const float *hb = a.h + ((size_t)b * a.N + p0) * 64;
        for (int i = tid; i < kTile * 64; i += kPtThreads) bufA[(i >> 6) * kLd + (i & 63)] = i < nvalid * 64 ? hb[i] : 0.0f;
    }
    __syncthreads();
    if (MODE == 0) {
        conv3<kReluBn>(xs, bufA, kLd, 64, a.c1.W, a.c1.b, a.c1.bn);
        __syncthreads();
        conv_mfma<64, kReluBn, false>(bufA, bufB, 128, a.c2.W, a.c2.b, a.c2.bn, nvalid, nullptr);
        __syncthreads();
        last_layer<kReluBn, WIN>(a, bufB, nvalid, p0, tmax);
    } else if (MODE == 1) {
        conv3<kNone>(xs, xt, 3, 3, a.tf + (size_t)b * 9, nullptr, Bn{});
        __syncthreads();
        conv3<kBnRelu>(xt, bufA, kLd, 64, a.c0.W, a.c0.b, a.c0.bn);
        __syncthreads();
        float *hb = a.h + ((size_t)b * a.N + p0) * 64;
        for (int i = tid; i < nvalid * 64; i += kPtThreads) hb[i] = bufA[(i >> 6) * kLd + (i & 63)];
        conv_mfma<64, kReluBn, false>(bufA, bufB, 64, a.c1.W, a.c1.b, a.c1.bn, nvalid, nullptr);
        __syncthreads();
        conv_mfma<64, kReluBn, false>(bufB, bufA, 128, a.c2.W, a.c2.b, a.c2.bn, nvalid, nullptr);
        __syncthreads();
        last_layer<kReluBn, WIN>(a, bufA, nvalid, p0, tmax);
    } else {
        conv_mfma<64, kNone, false>(bufA, bufB, 64, a.tf + (size_t)b * 4096, nullptr, Bn{}, nvalid, nullptr);
        __syncthreads();
        conv_mfma<64, kReluBn, false>(bufB, bufA, 128, a.c2.W, a.c2.b, a.c2.bn, nvalid, nullptr);
        __syncthreads();
        last_layer<kBnOnly, WIN>(a, bufA, nvalid, p0, tmax);
    }
}

template <bool FEAT>
__global__ __launch_bounds__(kHeadThreads) void pointnet_head_kernel(const HeadArgs a) {
    __shared__ float v0[kFeat], v1[512], v2[256];
    const int b = blockIdx.x, tid = threadIdx.x;
    const float m = fold_tile_maxima(a.tmax, a.ntiles, b);
    v0[tid] = m;
    if (FEAT && a.pooled) a.pooled[(size_t)b * kFeat + tid] = m;
    __syncthreads();
    if (tid < 512) {
        float v = relu(dense_chain(v0, kFeat, a.d1.W, 512, tid) + a.d1.b[tid]);
        if (FEAT) v = batchnorm(v, a.bn1.g[tid], a.bn1.b[tid], a.bn1.m[tid], sqrtf(a.bn1.v[tid] + kBnEps));
        v1[tid] = v;
    }
    __syncthreads();
    if (tid < 256) {
        const float v = relu(dense_chain(v1, 512, a.d2.W, 256, tid) + a.d2.b[tid]);
        v2[tid] = batchnorm(v, a.bn2.g[tid], a.bn2.b[tid], a.bn2.m[tid], sqrtf(a.bn2.v[tid] + kBnEps));
    }
    __syncthreads();
    for (int o = tid; o < a.n3; o += kHeadThreads) {
        const float v = dense_chain(v2, 256, a.d3.W, a.n3, o) + a.d3.b[o];
        if (FEAT) {
            a.logits[(size_t)b * a.n3 + o] = relu(v);
        } else {
            const size_t at = (size_t)b * a.n3 + (o / a.K) + (size_t)a.K * (o % a.K);
            a.mat[at] = v;
            if (a.mat_user) a.mat_user[at] = v;
        }
    }
    if (FEAT) softmax_of_logits(a.logits + (size_t)b * a.n3, a.probs + (size_t)b * a.n3, a.n3);
}

template <int MODE, bool WIN>
fx3d_status launch_points_of(const PointArgs &a, int B, hipStream_t st) {
    const fx3d_status rc = ensure_dynamic_lds(reinterpret_cast<const void *>(&pointnet_points_kernel<MODE, WIN>), (int)kPtLds,
                                              "pointnet_points_kernel");
    if (rc != FX3D_OK) return rc;
    ProfileScope prof(WIN ? "pointnet_points_win" : "pointnet_points", st);
    hipLaunchKernelGGL((pointnet_points_kernel<MODE, WIN>), dim3(a.ntiles, B), dim3(kPtThreads), kPtLds, st, a);
    FX3D_LAUNCH_CHECK();
    return FX3D_OK;
}

template <bool FEAT>
fx3d_status launch_head_of(const HeadArgs &a, int B, hipStream_t st) {
    ProfileScope prof("pointnet_head", st);
    hipLaunchKernelGGL(pointnet_head_kernel<FEAT>, dim3(B), dim3(kHeadThreads), 0, st, a);
    FX3D_LAUNCH_CHECK();
    return FX3D_OK;
}

}  // namespace

namespace fx3d {
namespace mlp {
namespace pointnet {

fx3d_status launch_points(int mode, bool win, const PointArgs &a, int B, hipStream_t st) {
    if (win) return mode == 0 ? launch_points_of<0, true>(a, B, st) : mode == 1 ? launch_points_of<1, true>(a, B, st) : launch_points_of<2, true>(a, B, st);
    return mode == 0 ? launch_points_of<0, false>(a, B, st) : mode == 1 ? launch_points_of<1, false>(a, B, st) : launch_points_of<2, false>(a, B, st);
}

fx3d_status launch_head(bool feat, const HeadArgs &a, int B, hipStream_t st) {
    return feat ? launch_head_of<true>(a, B, st) : launch_head_of<false>(a, B, st);
}

}  // namespace pointnet
}  // namespace mlp
}  // namespace fx3d

extern "C" {

fx3d_status fx3d_pointnet_param_count(int32_t num_classes, int64_t *count) {
    FX3D_REQUIRE(count != nullptr, "fx3d_pointnet_param_count: count is NULL");
    FX3D_REQUIRE(num_classes >= 1 && num_classes <= (1 << 20), "fx3d_pointnet_param_count: num_classes must be in [1, 2^20], got %d",
                 num_classes);
    *count = layout(nullptr, num_classes).count;
    return FX3D_OK;
}

fx3d_status fx3d_pointnet_workspace_bytes(int32_t N, int32_t B, int32_t num_classes, size_t *bytes) {
    FX3D_REQUIRE(bytes != nullptr, "fx3d_pointnet_workspace_bytes: bytes is NULL");
    const fx3d_status rc = check_sizes("fx3d_pointnet_workspace_bytes", N, B, num_classes);
    if (rc != FX3D_OK) return rc;
    *bytes = ws_plan(N, B, num_classes).total;
    return FX3D_OK;
}

fx3d_status fx3d_pointnet_forward(const float *params_dev, int32_t num_classes, const float *x, int32_t N, int32_t B,
                                  float *probs, float *logits, float *stn, float *fstn, float *pooled, void *ws,
                                  size_t ws_bytes, fx3d_stream_t s) {
    const char *fn = "fx3d_pointnet_forward";
    FX3D_REQUIRE(params_dev && x && probs && ws, "%s: params_dev, x, probs and ws must not be NULL", fn);
    const fx3d_status rc = check_sizes(fn, N, B, num_classes);
    if (rc != FX3D_OK) return rc;
    const WsPlan w = ws_plan(N, B, num_classes);
    FX3D_REQUIRE(ws_bytes >= w.total, "%s: workspace of %zu bytes, fx3d_pointnet_workspace_bytes says %zu", fn, ws_bytes, w.total);
    FX3D_REQUIRE((reinterpret_cast<uintptr_t>(ws) & 15) == 0, "%s: ws must be 16-byte aligned", fn);
    const Net n = layout(params_dev, num_classes);
    hipStream_t st = as_stream(s);
    char *wsb = static_cast<char *>(ws);
    float *h = reinterpret_cast<float *>(wsb + w.h), *tmax = reinterpret_cast<float *>(wsb + w.tmax);
    float *T = reinterpret_cast<float *>(wsb + w.T), *F = reinterpret_cast<float *>(wsb + w.F);
    float *lg = logits ? logits : reinterpret_cast<float *>(wsb + w.logits);

    PointArgs p{};
    p.x = x; p.h = h; p.tmax = tmax; p.N = N; p.ntiles = w.ntiles;
    fx3d_status r;
    // stn: the (3, 3) input transform of every cloud
    p.c1 = n.stn.c1; p.c2 = n.stn.c2; p.c3 = n.stn.c3;
    if ((r = launch_points(0, false, p, B, st)) != FX3D_OK) return r;
    if ((r = launch_head(false, stn_head(n.stn, 3, tmax, w.ntiles, T, stn), B, st)) != FX3D_OK) return r;
    // input transform, conv_block1 (kept as h), fstn: the (64, 64) feature transform
    p.tf = T; p.c0 = n.block1; p.c1 = n.fstn.c1; p.c2 = n.fstn.c2; p.c3 = n.fstn.c3;
    if ((r = launch_points(1, false, p, B, st)) != FX3D_OK) return r;
    if ((r = launch_head(false, stn_head(n.fstn, 64, tmax, w.ntiles, F, fstn), B, st)) != FX3D_OK) return r;
    // feature transform, feat, cls, softmax
    p.tf = F; p.c2 = n.f1; p.c3 = n.f2;
    if ((r = launch_points(2, false, p, B, st)) != FX3D_OK) return r;
    HeadArgs hd{};
    hd.tmax = tmax; hd.ntiles = w.ntiles;
    hd.d1 = n.fd1; hd.bn1 = n.fbn1; hd.d2 = n.fd2; hd.bn2 = n.fbn2; hd.d3 = n.cls;
    hd.n3 = num_classes; hd.K = 1; hd.pooled = pooled; hd.logits = lg; hd.probs = probs;
    return launch_head(true, hd, B, st);
}

}  // extern "C"
