// What dgcnn.hip (the forward), dgcnn_train.hip (the training-mode forward), dgcnn_grad.hip (the adjoint) and dgcnn_grad_train.hip
// (the training-mode adjoint) share: the layers of
// the two EdgeConv stages, conv_3's LDS image of a 64-point tile of x2, the winners of the maximum over the points (the two
// adjoints), the walk over the flat parameter buffer, the size check of the entries, and the forward's workspace and conv_3 launch.
#pragma once
#include "mlp_common.h"
#include "pointnet_net.h"

namespace fx3d {
namespace mlp {

constexpr int kLd3 = 258;         // LDS row stride of conv_3's 256-channel input image
constexpr size_t kConv3Lds = (size_t)kTile * kLd3 * sizeof(float);
constexpr int32_t kEc1[] = {3, 32, 64, 64}, kEc2[] = {64, 128, 256};  // the layers of the two EdgeConv stages

// the (64 x 256) tile of x2 (256, N, B) that begins at point p0 of cloud b, rows beyond the cloud's last point zeros; all
// kPtThreads threads call it, and synchronise afterwards
__device__ __forceinline__ void load_x2_tile(float *lds, const float *__restrict__ x2, int b, int N, int p0, int nvalid) {
    const float *xb = x2 + ((size_t)b * N + p0) * 256;
    for (int i = threadIdx.x; i < kTile * 256; i += kPtThreads) lds[(i >> 8) * kLd3 + (i & 255)] = i < nvalid * 256 ? xb[i] : 0.0f;
}

// The winners of the maximum over the points, one block = 64 points of one cloud, lds of kConv3Lds bytes: the forward's conv_3
// again, block for block (the x2 tile, mfma_slab<256> and epilogue<kBnRelu>: the forward's bits), compared with pooled where that
// is positive; per (tile, channel) the smallest matching point into tfirst (1024, ntiles, B), kNoPoint where the tile has none -- a
// lane minimum over its 32 rows and one shuffle across the half-waves --, and with PRE what conv3.bn was given there (conv + bias;
// 0 where there is none) into tpre, picked from the accumulators once the lane's minimum is known.  dgcnn_argmax_kernel
// (dgcnn_grad.hip) is PRE = false, dgcnn_gt_argmax_kernel (dgcnn_grad_train.hip, at the batch statistics) PRE = true.  The slab
// walk is pointnet::for_each_slab<256, kLd3>'s, written out: with the body as a lambda PRE = false takes 90 VGPRs for 80, which is
// 5 waves per SIMD for 6.
template <bool PRE>
__device__ __forceinline__ void conv3_winners(float *lds, const float *__restrict__ x2, const Conv &c, const float *__restrict__ pooled,
                                              int32_t *__restrict__ tfirst, float *__restrict__ tpre, int N, int ntiles) {
    const int tile = blockIdx.x, b = blockIdx.y;
    const int p0 = tile * kTile;
    const int nvalid = min(kTile, N - p0);
    load_x2_tile(lds, x2, b, N, p0, nvalid);
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, h = lane >> 5, j = lane & 31;
    const float *a0 = lds + j * kLd3 + h, *a1 = a0 + 32 * kLd3;
    const size_t out = ((size_t)b * ntiles + tile) * kFeat;
    for (int sl = wave; sl < kFeat / 32; sl += kPtThreads / 64) {
        const int o = sl * 32 + j;
        f32x16 acc0 = {0}, acc1 = {0};
        mfma_slab<256>(a0, a1, c.W + (size_t)256 * o, h, acc0, acc1);
        const float bi = c.b[o], g = c.bn.g[o], be = c.bn.b[o], mu = c.bn.m[o], sd = pointnet::bn_sd(c.bn, o);
        const float pv = pooled[(size_t)b * kFeat + o];
        const float tgt = pv > 0.0f ? pv : __int_as_float(0x7fc00000);  // NaN equals nothing: no winner
        int first = pointnet::kNoPoint;  // the lane's smallest matching point: a minimum, no branch
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int p = mfma_row(r, h);
            const float v0 = epilogue<kBnRelu>(acc0[r], bi, g, be, mu, sd), v1 = epilogue<kBnRelu>(acc1[r], bi, g, be, mu, sd);
            if (p < nvalid && v0 == tgt) first = min(first, p0 + p);
            if (p + 32 < nvalid && v1 == tgt) first = min(first, p0 + p + 32);
        }
        float pre = 0.0f;
        if (PRE) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int p = p0 + mfma_row(r, h);
                pre = p == first ? acc0[r] + bi : p + 32 == first ? acc1[r] + bi : pre;
            }
        }
        const int ofirst = __shfl_xor(first, 32, 64);
        const float opre = __shfl_xor(pre, 32, 64);
        if (h == 0) {
            tfirst[out + o] = min(first, ofirst);
            if (PRE) tpre[out + o] = ofirst < first ? opre : pre;
        }
    }
}

// a training-mode head block's BatchNorm and relu of this thread's element v = dense + bias (dgcnn_train.hip's head kernels, and
// dgcnn_grad_train.hip, which computes them again)
__device__ __forceinline__ float head_bn_relu(const Bn &bn, float v) {
    const int tid = threadIdx.x;
    return relu(batchnorm(v, bn.g[tid], bn.b[tid], bn.m[tid], sqrtf(bn.v[tid] + kBnEps)));
}

// ---- the flat parameter buffer in forward order (flux3d_hip.h) ----------------------------------------------------------
struct Net {
    const float *ec1, *ec2;  // the parameters of the two EdgeConv stages, in the EdgeConv layout
    Conv c3;
    Dense d4, d5, d6;
    Bn bn4, bn5;
    long long count;
};

inline Net dgcnn_layout(const float *params, int num_classes) {
    Cursor c{params, 0};
    Net n;
    n.ec1 = c.take(edgeconv_layout(nullptr, kEc1, 4, nullptr));
    n.ec2 = c.take(edgeconv_layout(nullptr, kEc2, 3, nullptr));
    n.c3 = c.conv(256, kFeat);  n.c3.bn = c.bn(kFeat);
    n.d4 = c.dense(kFeat, 512); n.bn4 = c.bn(512);
    n.d5 = c.dense(512, 256);   n.bn5 = c.bn(256);
    n.d6 = c.dense(256, num_classes);
    n.count = c.at;
    return n;
}

inline fx3d_status dgcnn_check_sizes(const char *fn, int32_t N, int32_t B, int32_t K, int32_t nc) {
    FX3D_REQUIRE(nc >= 1 && nc <= (1 << 20), "%s: num_classes must be in [1, 2^20], got %d", fn, nc);
    return check_edgeconv_sizes(fn, N, B, K);
}

// the training-mode entries' (dgcnn_train.hip, dgcnn_grad_train.hip) sizes
inline fx3d_status dgcnn_check_train_sizes(const char *fn, int32_t N, int32_t B, int32_t K, int32_t nc) {
    const fx3d_status rc = dgcnn_check_sizes(fn, N, B, K, nc);
    if (rc != FX3D_OK) return rc;
    FX3D_REQUIRE(B >= 2, "%s: training-mode BatchNorm needs B >= 2 clouds (a Dense BatchNorm's running variance divides by B - 1), got %d",
                 fn, B);
    return FX3D_OK;
}

// the forward's workspace: x1 (64, N, B) | x2 (256, N, B) | per-tile maxima (1024, ntiles, B) | logits (num_classes, B) | one
// EdgeConv workspace, the larger of the two stages'
struct DgcnnWsPlan { size_t x1, x2, tmax, logits, ec, total; int ntiles; };
inline fx3d_status dgcnn_ws_plan(int N, int B, int K, int nc, DgcnnWsPlan *w) {
    w->ntiles = (N + kTile - 1) / kTile;
    WsBump ws;
    w->x1 = ws.put((size_t)64 * N * B * sizeof(float));
    w->x2 = ws.put((size_t)256 * N * B * sizeof(float));
    w->tmax = ws.put((size_t)kFeat * w->ntiles * B * sizeof(float));
    w->logits = ws.put((size_t)nc * B * sizeof(float));
    size_t e1 = 0, e2 = 0;
    fx3d_status rc;
    if ((rc = edgeconv_workspace_bytes(kEc1[0], N, B, K, &e1)) != FX3D_OK) return rc;
    if ((rc = edgeconv_workspace_bytes(kEc2[0], N, B, K, &e2)) != FX3D_OK) return rc;
    w->ec = ws.put(e1 > e2 ? e1 : e2);
    w->total = ws.at;
    return FX3D_OK;
}

// dgcnn.hip: dgcnn_conv3_kernel on st -- conv_3 + BatchNorm + relu of x2 (256, N, B) reduced to the per-tile maxima tmax
// (1024, ntiles, B); label: the launch's name in the library's profile
fx3d_status launch_conv3(const float *x2, const Conv &c3, float *tmax, int N, int ntiles, int B, hipStream_t st, const char *label);

}  // namespace mlp
}  // namespace fx3d
