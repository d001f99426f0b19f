// PointNet inference (gfx950): (m::PointNet)(X) of src/models/pointnet.jl:62-85 in test mode, Float32: the forward (pointnet_grad.hip: its adjoint).
// include/flux3d_hip.h states the network, the arithmetic and the parameter layout; this file is how they are computed.
//
// Every contraction is one accumulator per output element that walks the input channels upwards with one rounding per
// step: acc = fmaf(x[c], W[c,o], acc) from +0.0f.  v_mfma_f32_32x32x2_f32 is that chain (two steps per instruction, the
// lower k first), so the 1x1 convolutions with 64 or 128 input channels run on it; the 3-channel ones (no multiple of the
// instruction's k: padding with zeros would turn an Inf weight into NaN) and the dense heads run the same chain as v_fma_f32.
// No split of a contraction over waves or blocks, no float atomics: the bits do not depend on the launch shape.
//
// Two kernels, three rounds (stn, fstn, feat).  pointnet_net.h states a round's layer chain (round_trunk) and the head's phases
// (head_pool .. head_finish) for them, for the training-mode forward and for the adjoint; the kernels here are:
//   pointnet_points_kernel<MODE>: one block = 64 points of one cloud, 4 waves.  The tile's activations live in two
//     (64 x 128) LDS images (row stride 130 floats: the A-operand reads of a 32-point tile fall on 64 distinct banks; the
//     epilogue's stores, 32 consecutive channels per lane half with the halves 4 rows = 8 banks apart, overlap on 24 banks).  A wave owns slabs of 32 output channels and computes them for both 32-point halves of the tile from
//     one stream of weights: lane (h, j) reads row j of the slab, W[4q .. 4q+3, o] per step (the (Cin, Cout) column-major
//     layout makes that 16 contiguous bytes), and feeds elements h and 2 + h to two consecutive k-steps.  The epilogue
//     (bias, relu, BatchNorm in the order of the layer) runs on the accumulators: a lane holds ONE channel and 16 points
//     per half.  The last layer (128 -> 1024) is never stored: each slab is reduced to the tile's maximum per channel
//     (Julia's max) and written to the workspace with plain stores.
//     MODE 0 = stn (X -> 64 -> 128 -> 1024), 1 = fstn (X * T -> conv_block1 -> stored as h (64, N, B) -> 64 -> 128 -> 1024),
//     2 = feat (h * F -> 128 -> 1024, no relu on the last), 3 = stnKD(K) for a K known at run time only (stnkd.hip: MODE 0's
//     layers, the first on mfma_slab_rt over the tile of x (K, N, B) in columns 0 .. K - 1 of an image).
//   pointnet_head_kernel<FEAT>: one block per cloud folds the per-tile maxima, then the dense layers with one thread per
//     output element (W (out, in) column-major: consecutive threads read consecutive weights), BatchNorm, and for the
//     classifier relu + softmax.  stn / fstn write their (K, K) matrix already transposed (T[i,j] = d[j + K i] at i + K j),
//     which is the (Cin, Cout) layout of a convolution: the per-cloud transform is one more bias-free layer of the point kernel.
#include "pointnet_net.h"

using namespace fx3d;
using namespace fx3d::mlp;
using namespace fx3d::mlp::pointnet;

namespace {

// The round's layers (round_trunk) with the last one (128 -> 1024) reduced to the tile's maxima.  WIN: the adjoint's
// instantiation (pointnet_grad.hip), whose last layer also writes the tile's winners (conv_final_win).
template <int MODE, bool WIN>
__global__ __launch_bounds__(kPtThreads) void pointnet_points_kernel(const PointArgs a) {
    extern __shared__ float lds[];
    const int tile = blockIdx.x, b = blockIdx.y;
    const int p0 = tile * kTile;
    const int nvalid = min(kTile, a.N - p0);
    const size_t at = ((size_t)b * a.ntiles + tile) * kFeat;
    round_trunk<MODE, kLastLayer[MODE], true>(a, lds, b, p0, nvalid, [&](const float *in, const Conv &c, auto layer) {
        constexpr int EPI = decltype(layer)::EPI;
        if (WIN) conv_final_win<EPI>(in, c, nvalid, p0, a.tmax + at, a.tfirst + at, a.tpre + at);
        else conv_mfma<128, EPI, true>(in, nullptr, kFeat, c.W, c.b, c.bn, nvalid, a.tmax + at);
    });
}

template <bool FEAT>
__global__ __launch_bounds__(kHeadThreads) void pointnet_head_kernel(const HeadArgs a) {
    __shared__ float v0[kFeat], v1[512], v2[256];
    const int b = blockIdx.x, tid = threadIdx.x;
    head_pool<FEAT>(a, b, v0);
    __syncthreads();
    if (tid < 512) {
        const float v = head_relu_dense<512>(a.d1, v0);
        v1[tid] = FEAT ? head_bn(a.bn1, v) : v;
    }
    __syncthreads();
    if (tid < 256) v2[tid] = head_bn(a.bn2, head_relu_dense<256>(a.d2, v1));
    __syncthreads();
    head_finish<FEAT>(a, b, v2);
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
    if (mode == 3) {  // stnKD(K), stnkd.hip: it has no adjoint, so no instantiation with the winners
        if (win) {
            set_error("launch_points: stnKD(K) has no winners' instantiation");
            return FX3D_ERR_UNSUPPORTED;
        }
        return launch_points_of<3, false>(a, B, st);
    }
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
    const WsView v{static_cast<char *>(ws)};
    float *tmax = v.f32(w.tmax), *T = v.f32(w.T), *F = v.f32(w.F);
    PointArgs p{};
    p.x = x; p.h = v.f32(w.h); p.tmax = tmax; p.N = N; p.ntiles = w.ntiles;
    fx3d_status r;
    // stn: T (3, 3) of every cloud; x T, conv_block1 (kept as h), fstn: F (64, 64); h F, feat, cls, softmax
    for (int mode = 0; mode < 3; ++mode) {
        set_round(p, n, mode, T, F);
        if ((r = launch_points(mode, false, p, B, st)) != FX3D_OK) return r;
        const HeadArgs hd = mode < 2 ? stn_head(n, mode, tmax, w.ntiles, T, F, mode == 0 ? stn : fstn)
                                     : feat_head(n, num_classes, tmax, w.ntiles, pooled, logits ? logits : v.f32(w.logits), probs);
        if ((r = launch_head(mode == 2, hd, B, st)) != FX3D_OK) return r;
    }
    return FX3D_OK;
}

}  // extern "C"
