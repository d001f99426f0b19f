// What pointnet.hip (the forward) and pointnet_grad.hip (its adjoint) share: the walk over the flat parameter buffer, the
// forward's workspace, the size check of both entries, the arguments of the forward's two kernels and their launches (defined
// in pointnet.hip, which owns the kernels), and the last layer of a round with the winners the adjoint needs.
#pragma once
#include <climits>

#include "mlp_common.h"

namespace fx3d {
namespace mlp {
namespace pointnet {  // (dgcnn_net.h has a Net of its own)

constexpr size_t kPtLds = (size_t)(2 * kTile * kLd + 2 * kTile * 3) * sizeof(float);
constexpr int kNoPoint = INT_MAX;  // a tile in which no point reproduces its maximum (a NaN maximum)

struct PointArgs {
    const float *x;   // (3, N, B): MODE 0, 1
    float *h;         // workspace (64, N, B): written by MODE 1, read by MODE 2
    const float *tf;  // the cloud's transform, (3, 3, B) for MODE 1, (64, 64, B) for MODE 2
    Conv c0;          // MODE 1: conv_block1
    Conv c1, c2, c3;  // the round's convolutions (MODE 2: c2, c3)
    float *tmax;      // (1024, ntiles, B)
    int N, ntiles;
    int32_t *tfirst;  // the adjoint's launches (WIN): (1024, ntiles, B), the first point of the tile that equals the tile's maximum
    float *tpre;      //   and what the last layer's BatchNorm was given at that point
};

struct HeadArgs {
    const float *tmax;  // (1024, ntiles, B)
    int ntiles;
    Dense d1, d2, d3;   // 1024 -> 512, 512 -> 256, 256 -> n3
    Bn bn1, bn2;        // FEAT: BatchNorm(512) after d1; both: BatchNorm(256) after d2
    int n3, K;          // outputs of d3; stn / fstn: n3 = K K
    float *mat, *mat_user;  // stn / fstn: (K, K, B) in the workspace and, optionally, the caller's copy
    float *pooled;          // FEAT, optional: (1024, B)
    float *logits, *probs;  // FEAT: (n3, B) each; logits is the caller's array or the workspace
};

struct Stn { Conv c1, c2, c3; Dense d1, d2, d3; Bn bn; };
struct Net {
    Stn stn, fstn;
    Conv block1, f1, f2;
    Dense fd1, fd2, cls;
    Bn fbn1, fbn2;
    long long count;
};

inline Stn layout_stn(Cursor &c, int K) {
    Stn s;
    s.c1 = c.conv(K, 64);     s.c1.bn = c.bn(64);
    s.c2 = c.conv(64, 128);   s.c2.bn = c.bn(128);
    s.c3 = c.conv(128, 1024); s.c3.bn = c.bn(1024);
    s.d1 = c.dense(1024, 512);
    s.d2 = c.dense(512, 256);
    s.bn = c.bn(256);
    s.d3 = c.dense(256, K * K);
    return s;
}

inline Net layout(const float *params, int num_classes) {
    Cursor c{params, 0};
    Net n;
    n.stn = layout_stn(c, 3);
    n.block1 = c.conv(3, 64);   n.block1.bn = c.bn(64);
    n.fstn = layout_stn(c, 64);
    n.f1 = c.conv(64, 128);     n.f1.bn = c.bn(128);
    n.f2 = c.conv(128, 1024);   n.f2.bn = c.bn(1024);
    n.fd1 = c.dense(1024, 512); n.fbn1 = c.bn(512);
    n.fd2 = c.dense(512, 256);  n.fbn2 = c.bn(256);
    n.cls = c.dense(256, num_classes);
    n.count = c.at;
    return n;
}

// ---- training mode (pointnet_train.hip): the 13 BatchNorms in forward order -- stn.bn1 .. bn4, conv_block1.bn, fstn.bn1 .. bn4,
// feat.bn1 .. bn4 -- which is the order of their mu / sigma2 slots in the flat parameter buffer and of the statistics buffer
// (flux3d_hip.h "PointNet training-mode forward": per BatchNorm mean (C) then variance (C)).  f(bn, C) for each of them.
constexpr int kNumBn = 13;
constexpr int kStatChannels = 2 * (64 + 128 + kFeat + 256) + 64 + 128 + kFeat + 512 + 256;  // 4928
template <class NetT, class F>
inline void for_each_bn(NetT &n, F f) {
    auto stn = [&](auto &s) { f(s.c1.bn, 64); f(s.c2.bn, 128); f(s.c3.bn, kFeat); f(s.bn, 256); };
    stn(n.stn);
    f(n.block1.bn, 64);
    stn(n.fstn);
    f(n.f1.bn, 128); f(n.f2.bn, kFeat); f(n.fbn1, 512); f(n.fbn2, 256);
}
// the network whose BatchNorms read their mean and variance from a statistics buffer instead of the running values: the
// test-mode kernels then evaluate every layer whose statistics are there in training mode
inline Net with_batch_stats(Net n, const float *stats) {
    size_t at = 0;
    for_each_bn(n, [&](Bn &bn, int C) {
        bn.m = stats + at;
        bn.v = stats + at + C;
        at += 2 * (size_t)C;
    });
    return n;
}

// the workspace: h (64, N, B) | per-tile maxima (1024, ntiles, B) | T (3, 3, B) | F (64, 64, B) | logits (num_classes, B)
struct WsPlan { size_t h, tmax, T, F, logits, total; int ntiles; };
inline WsPlan ws_plan(int N, int B, int nc) {
    WsPlan w;
    w.ntiles = (N + kTile - 1) / kTile;
    WsBump ws;
    w.h = ws.put((size_t)64 * N * B * sizeof(float));
    w.tmax = ws.put((size_t)kFeat * w.ntiles * B * sizeof(float));
    w.T = ws.put((size_t)9 * B * sizeof(float));
    w.F = ws.put((size_t)4096 * B * sizeof(float));
    w.logits = ws.put((size_t)nc * B * sizeof(float));
    w.total = ws.at;
    return w;
}

inline fx3d_status check_sizes(const char *fn, int32_t N, int32_t B, int32_t nc) {
    FX3D_REQUIRE(nc >= 1 && nc <= (1 << 20), "%s: num_classes must be in [1, 2^20], got %d", fn, nc);
    FX3D_REQUIRE(N >= 1 && B >= 1, "%s: N and B must be positive, got N=%d B=%d", fn, N, B);
    FX3D_REQUIRE(B <= 65535, "%s: B must be at most 65535, got %d", fn, B);
    FX3D_REQUIRE((long long)N * B <= (1ll << 31), "%s: N * B must be at most 2^31, got %lld", fn, (long long)N * B);
    return FX3D_OK;
}

inline HeadArgs stn_head(const Stn &s, int K, const float *tmax, int ntiles, float *mat, float *mat_user) {
    HeadArgs h{};
    h.tmax = tmax; h.ntiles = ntiles;
    h.d1 = s.d1; h.d2 = s.d2; h.d3 = s.d3; h.bn2 = s.bn;
    h.n3 = K * K; h.K = K; h.mat = mat; h.mat_user = mat_user;
    return h;
}

// pointnet_points_kernel<mode> (win: the instantiation that also writes a.tfirst and a.tpre) and pointnet_head_kernel<feat>
// on st; pointnet.hip
fx3d_status launch_points(int mode, bool win, const PointArgs &a, int B, hipStream_t st);
fx3d_status launch_head(bool feat, const HeadArgs &a, int B, hipStream_t st);

// what the last layer's BatchNorm is given: relu(acc + bias) for kReluBn, acc + bias for kBnOnly
template <int EPI>
__device__ __forceinline__ float before_bn(float acc, float bias) { return EPI == kReluBn ? relu(acc + bias) : acc + bias; }

// conv_mfma<128, EPI, true> -- the same slabs, epilogue and fold, so the same tmax -- that also finds, while the slab's values
// are still in the accumulators, the first of the tile's valid points whose value EQUALS the tile's maximum (Float32 ==, so
// -0 equals +0; a NaN maximum equals nothing: kNoPoint), and keeps what the BatchNorm was given there.  p0: the tile's first
// point.  A lane's rows mfma_row(r, h) ascend with r, the second half's follow the first's.
template <int EPI>
__device__ __forceinline__ void conv_final_win(const float *in, const float *__restrict__ W, const float *__restrict__ bias,
                                               const Bn bn, int nvalid, int p0, float *__restrict__ tmax,
                                               int32_t *__restrict__ tfirst, float *__restrict__ tpre) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, h = lane >> 5, j = lane & 31;
    const float *a0 = in + j * kLd + h, *a1 = a0 + 32 * kLd;
    for (int sl = wave; sl < kFeat / 32; sl += kPtThreads / 64) {
        const int o = sl * 32 + j;
        f32x16 acc0 = {0}, acc1 = {0};
        mfma_slab<128>(a0, a1, W + (size_t)128 * o, h, acc0, acc1);
        const float bi = bias[o], g = bn.g[o], be = bn.b[o], mu = bn.m[o], sd = sqrtf(bn.v[o] + kBnEps);
        float m = __int_as_float(0xff800000);
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int p = mfma_row(r, h);
            if (p < nvalid) m = jmax(m, epilogue<EPI>(acc0[r], bi, g, be, mu, sd));
            if (p + 32 < nvalid) m = jmax(m, epilogue<EPI>(acc1[r], bi, g, be, mu, sd));
        }
        m = jmax(m, __shfl_xor(m, 32, 64));
        int first = kNoPoint;
        float pre = 0.0f;
#pragma unroll
        for (int r = 15; r >= 0; --r) {  // descending, the second half first: the last assignment is the smallest point
            const int p = mfma_row(r, h) + 32;
            if (p < nvalid && epilogue<EPI>(acc1[r], bi, g, be, mu, sd) == m) { first = p0 + p; pre = before_bn<EPI>(acc1[r], bi); }
        }
#pragma unroll
        for (int r = 15; r >= 0; --r) {
            const int p = mfma_row(r, h);
            if (p < nvalid && epilogue<EPI>(acc0[r], bi, g, be, mu, sd) == m) { first = p0 + p; pre = before_bn<EPI>(acc0[r], bi); }
        }
        const int ofirst = __shfl_xor(first, 32, 64);
        const float opre = __shfl_xor(pre, 32, 64);
        if (h == 0) {
            tmax[o] = m;
            tfirst[o] = min(first, ofirst);
            tpre[o] = ofirst < first ? opre : pre;
        }
    }
}

}  // namespace pointnet
}  // namespace mlp
}  // namespace fx3d
