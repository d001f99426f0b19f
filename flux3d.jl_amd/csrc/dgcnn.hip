// DGCNN inference (gfx950): (m::DGCNN)(X) of src/models/dgcnn.jl:113-147 in test mode, Float32: the forward (its adjoint:
// dgcnn_grad.hip; dgcnn_net.h holds what the two share).
// include/flux3d_hip.h ("DGCNN inference") states the network, the arithmetic and the parameter layout; this file is how they are
// computed.  The arithmetic is PointNet's (mlp_common.h): one accumulator per output element, walking the input channels
// upwards on v_mfma_f32_32x32x2_f32 (or v_fma_f32 for the dense head); no contraction split over waves or blocks, no float
// atomics.
//
// Per forward: EdgeConv([3, 32, 64, 64], K) on x, EdgeConv([64, 128, 256], K) on x1, conv3, head.
//   The two EdgeConv stages are the EdgeConv layer itself (edgeconv.hip's header comment: the neighbour search, then
//     edgeconv_kernel<NS, LD> with the widths as arguments), run through edgeconv_run on the ec1 / ec2 slices of the parameter
//     buffer, whose layout is the layer's own.  They share one EdgeConv workspace; a caller's idx1 / idx2 are the layer's idx_out.
//   dgcnn_conv3_kernel: one block = 64 points; the (64 x 256) tile of x2 in one LDS image (row stride 258 = 2 mod 64, the bank
//     pattern of kLd), conv 256 -> 1024 + BN + relu reduced to the tile's maximum per channel (conv_mfma<.., FINAL>).
//   dgcnn_head_kernel: one block per cloud folds the tile maxima (= MaxPool((npoints,))), then fc_4, fc_5 (dense, BN, relu),
//     fc_6 (dense, no activation) with one thread per output element, and the softmax.
#include "dgcnn_net.h"

using namespace fx3d;
using namespace fx3d::mlp;

namespace {

__global__ __launch_bounds__(kPtThreads) void dgcnn_conv3_kernel(const float *__restrict__ x2, const Conv c, float *__restrict__ tmax_all,
                                                                 int N, int ntiles) {
    extern __shared__ float lds[];
    const int tile = blockIdx.x, b = blockIdx.y;
    const int p0 = tile * kTile;
    const int nvalid = min(kTile, N - p0);
    load_x2_tile(lds, x2, b, N, p0, nvalid);
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
    const float m = fold_tile_maxima(a.tmax, a.ntiles, b);
    v0[tid] = m;
    if (a.pooled) a.pooled[(size_t)b * kFeat + tid] = m;
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
    softmax_of_logits(z, pr, a.nc);
}

}  // namespace

namespace fx3d {
namespace mlp {

fx3d_status launch_conv3(const float *x2, const Conv &c3, float *tmax, int N, int ntiles, int B, hipStream_t st, const char *label) {
    const fx3d_status r = ensure_dynamic_lds(reinterpret_cast<const void *>(&dgcnn_conv3_kernel), (int)kConv3Lds, "dgcnn_conv3_kernel");
    if (r != FX3D_OK) return r;
    ProfileScope prof(label, st);
    hipLaunchKernelGGL(dgcnn_conv3_kernel, dim3(ntiles, B), dim3(kPtThreads), kConv3Lds, st, x2, c3, tmax, N, ntiles);
    FX3D_LAUNCH_CHECK();
    return FX3D_OK;
}

}  // namespace mlp
}  // namespace fx3d

extern "C" {

fx3d_status fx3d_dgcnn_param_count(int32_t num_classes, int64_t *count) {
    FX3D_REQUIRE(count != nullptr, "fx3d_dgcnn_param_count: count is NULL");
    FX3D_REQUIRE(num_classes >= 1 && num_classes <= (1 << 20), "fx3d_dgcnn_param_count: num_classes must be in [1, 2^20], got %d", num_classes);
    *count = dgcnn_layout(nullptr, num_classes).count;
    return FX3D_OK;
}

fx3d_status fx3d_dgcnn_workspace_bytes(int32_t N, int32_t B, int32_t K, int32_t num_classes, size_t *bytes) {
    FX3D_REQUIRE(bytes != nullptr, "fx3d_dgcnn_workspace_bytes: bytes is NULL");
    fx3d_status rc = dgcnn_check_sizes("fx3d_dgcnn_workspace_bytes", N, B, K, num_classes);
    if (rc != FX3D_OK) return rc;
    DgcnnWsPlan w;
    if ((rc = dgcnn_ws_plan(N, B, K, num_classes, &w)) != FX3D_OK) return rc;
    *bytes = w.total;
    return FX3D_OK;
}

fx3d_status fx3d_dgcnn_forward(const float *params_dev, int32_t num_classes, int32_t K, const float *x, int32_t N, int32_t B,
                               float *probs, float *logits, int32_t *idx1, float *x1, int32_t *idx2, float *x2, float *pooled,
                               void *ws, size_t ws_bytes, fx3d_stream_t s) {
    const char *fn = "fx3d_dgcnn_forward";
    FX3D_REQUIRE(params_dev && x && probs && ws, "%s: params_dev, x, probs and ws must not be NULL", fn);
    fx3d_status r = dgcnn_check_sizes(fn, N, B, K, num_classes);
    if (r != FX3D_OK) return r;
    DgcnnWsPlan w;
    if ((r = dgcnn_ws_plan(N, B, K, num_classes, &w)) != FX3D_OK) return r;
    FX3D_REQUIRE(ws_bytes >= w.total, "%s: workspace of %zu bytes, fx3d_dgcnn_workspace_bytes says %zu", fn, ws_bytes, w.total);
    FX3D_REQUIRE((reinterpret_cast<uintptr_t>(ws) & 255) == 0, "%s: ws must be 256-byte aligned", fn);
    FX3D_REQUIRE(!x1 || (reinterpret_cast<uintptr_t>(x1) & 15) == 0, "%s: x1 must be 16-byte aligned", fn);
    const Net n = dgcnn_layout(params_dev, num_classes);
    hipStream_t st = as_stream(s);
    char *wsb = static_cast<char *>(ws);
    float *f1 = x1 ? x1 : reinterpret_cast<float *>(wsb + w.x1), *f2 = x2 ? x2 : reinterpret_cast<float *>(wsb + w.x2);
    float *tmax = reinterpret_cast<float *>(wsb + w.tmax);
    float *lg = logits ? logits : reinterpret_cast<float *>(wsb + w.logits);

    // EdgeConv1: neighbours in coordinate space; EdgeConv2: in the space of x1's 64 features
    if ((r = edgeconv_run(n.ec1, kEc1, 4, K, x, N, B, nullptr, f1, idx1, wsb + w.ec, s, "dgcnn_edgeconv1")) != FX3D_OK) return r;
    if ((r = edgeconv_run(n.ec2, kEc2, 3, K, f1, N, B, nullptr, f2, idx2, wsb + w.ec, s, "dgcnn_edgeconv2")) != FX3D_OK) return r;
    // conv_3 + the maximum over the points, per tile
    if ((r = launch_conv3(f2, n.c3, tmax, N, w.ntiles, B, st, "dgcnn_conv3")) != FX3D_OK) return r;
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
