// What dgcnn.hip (the forward) and dgcnn_grad.hip (its adjoint) share: the layers of the two EdgeConv stages, conv_3's LDS image
// of a 64-point tile of x2, the walk over the flat parameter buffer and the size check of both entries.
#pragma once
#include "mlp_common.h"

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

}  // namespace mlp
}  // namespace fx3d
