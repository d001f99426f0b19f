// PointNet's training-mode adjoint (gfx950): the gradients of sum(glogits . logits) for the logits of fx3d_pointnet_forward_train with
// respect to every parameter and to the input points, Float32, mu and sigma2 of all 13 BatchNorms functions of the batch and the
// dropout multipliers constants.  include/flux3d_hip.h ("PointNet training-mode adjoint") states the definition and the order of
// every sum; tests/pointnet_grad_train_ref.py restates it on the host.
//
// A BatchNorm's input gradient needs dbeta = sum gy and dgamma = sum gy xh over ALL the values of the channel, so every BatchNorm is
// a cut: what is above it runs for the whole batch, two Float64 sums per channel are finished, and only then what is below it starts.
// The forward's three rounds run first, as in pointnet_grad.hip, with the test-mode kernels at with_batch_stats (what
// forward_train's closing passes are).  Then, round by round from the last to the first (feat, fstn, stn):
//   pointnet_gt_head_{a,b,c}_kernel: the head's adjoint, one block per cloud, cut at the head's dense BatchNorms (and ended at the
//     round's last BatchNorm, whose gy lives at the winners only); pointnet_gt_cloud_sums_kernel between them: one thread per channel,
//     one Float64 chain over b.
//   pointnet_gt_last_bwd_kernel<MODE>: one block = 64 points of one cloud.  round_trunk up to the last layer's input, which it stores
//     (128, N, B); then pointnet_net.h's last_back<128, kLd, EPI>: the last layer's slabs four at a time -- 128 output channels, one slab
//     per wave --, the gradient at the contraction d formed while a slab is in the accumulators (dense: every point has one, through
//     dbeta / m and xh dgamma / m), the chain over all 1024 outputs ascending on v_mfma_f32_32x32x2_f32, the gradient at the last
//     layer's input (128, N, B).
//   pointnet_gt_last_pgrad_kernel<EPI>: dW and db of the last layer, one block of 8 waves per (cloud, 128 output channels):
//     pointnet_net.h's last_pgrad<128, kLd, EPI>, one chain over the cloud's points.  pointnet_reduce_kernel then sums the clouds.
//     (The two bodies live in pointnet_net.h because dgcnn_grad_train.hip's conv_3 kernels are their instantiations at 256 channels.)
//   pointnet_gt_sums_kernel<MODE, L>: the Float64 tile sums of (gy, gy xh) of BatchNorm L, pointnet_stats_kernel's tile and order with
//     gy read from the workspace; pointnet_gt_finish_kernel: fold_tile_sums, then dbeta, dgamma and the two means.
//   pointnet_gt_layer_bwd_kernel<MODE, L>: layer L of the round once its sums are known: the relu's output again (the forward's call),
//     the column pass, dW / db per tile (hsum_mfma, hsum3), the way back (back_mfma) and what the round does below it (F and gF, the
//     sum of the two paths into h, conv_block1 with gxt and gT, the two paths into x).
// No atomics; every sum has one owner and one order, which depends on (N, B, num_classes) alone.
#include <initializer_list>

#include "pointnet_net.h"

using namespace fx3d;
using namespace fx3d::mlp;
using namespace fx3d::mlp::pointnet;

namespace {

constexpr int kImg = kTile * kLd;
constexpr int kThird = 2 * kImg + 2 * kTile * 3;  // round_trunk's two images, x and x T; then a third image (floats)
constexpr size_t kLayerLds = (size_t)(kThird + kImg) * sizeof(float);
constexpr size_t kPgradLds = (size_t)2 * kImg * sizeof(float);
static_assert(kLayerLds <= 160 * 1024, "the layer adjoint's LDS");
static_assert(FX3D_POINTNET_GRAD_TRAIN_CLOUD_CHAINS == 1, "dW / db of a last convolution: one chain per cloud (last_pgrad)");

// ---- the head ----------------------------------------------------------------------------------------------------------------------
struct HeadGtArgs : HeadArgs {  // the forward's head of the round at the batch statistics
    const int32_t *tfirst;  // (1024, ntiles, B)
    const float *tpre;
    Bn bn3;                 // the BatchNorm of the round's last convolution
    const float *gup;       // FEAT: glogits (n3, B); else the gradient at the transform (K, K, B)
    const float *dropout;   // FEAT: (256, B) or NULL
    const float *mb, *mg;   // the means of the BatchNorm the phase starts below
    int32_t *nstar;         // (1024, B)
    float *r1, *a1, *r2, *a2;  // relu(dense1), d2's input, relu(dense2), d3's input
    float *dd1, *dd2, *dd3;
    float *gy1, *xh1, *gy2, *xh2, *gy3, *xh3;
};

// the forward's head again (pointnet_net.h's phases, the training head's dropout), dd3, and gy / xh of the head's last BatchNorm
template <bool FEAT>
__global__ __launch_bounds__(kHeadThreads) void pointnet_gt_head_a_kernel(const HeadGtArgs a) {
    __shared__ float v0[kFeat], v1[512], v2[256];
    const int b = blockIdx.x, tid = threadIdx.x;
    const float m = fold_tile_maxima(a.tmax, a.ntiles, b);
    int first = kNoPoint;
    float pre = 0.0f;
    {
        const size_t at = (size_t)b * a.ntiles * kFeat + tid;
        for (int k = a.ntiles - 1; k >= 0; --k)  // descending: the last assignment is the first tile that equals the maximum
            if (a.tmax[at + (size_t)k * kFeat] == m) {
                first = a.tfirst[at + (size_t)k * kFeat];
                pre = a.tpre[at + (size_t)k * kFeat];
            }
    }
    {
        const bool won = first != kNoPoint;
        const size_t at = (size_t)b * kFeat + tid;
        a.nstar[at] = won ? first : -1;
        a.xh3[at] = won ? (pre - a.bn3.m[tid]) / bn_sd(a.bn3, tid) : 0.0f;
    }
    v0[tid] = m;
    a.pooled[(size_t)b * kFeat + tid] = m;
    __syncthreads();
    if (tid < 512) {
        const float r1 = head_relu_dense<512>(a.d1, v0);
        v1[tid] = FEAT ? head_bn(a.bn1, r1) : r1;
        a.r1[(size_t)b * 512 + tid] = r1;
        a.a1[(size_t)b * 512 + tid] = v1[tid];
    }
    __syncthreads();
    if (tid < 256) {
        const float r2 = head_relu_dense<256>(a.d2, v1);
        float v = r2;
        if (FEAT && a.dropout) v = v * a.dropout[(size_t)b * 256 + tid];
        v2[tid] = head_bn(a.bn2, v);
        a.r2[(size_t)b * 256 + tid] = r2;
        a.a2[(size_t)b * 256 + tid] = v2[tid];
        a.xh2[(size_t)b * 256 + tid] = (v - a.bn2.m[tid]) / bn_sd(a.bn2, tid);
    }
    __syncthreads();
    float *dd3 = a.dd3 + (size_t)b * a.n3;
    for (int o = tid; o < a.n3; o += kHeadThreads) {
        float d;
        if (FEAT) {
            const float l = relu(head_dense3(a.d3, v2, a.n3, o));
            d = l > 0.0f ? a.gup[(size_t)b * a.n3 + o] : 0.0f;
        } else {
            d = a.gup[(size_t)b * a.n3 + (o / a.K) + (size_t)a.K * (o % a.K)];
        }
        dd3[o] = d;
    }
    __syncthreads();  // the block's dd3 is in memory
    if (tid < 256) {
        float g = 0.0f;
        if ((a.n3 & 3) == 0) {
            g = transposed_chain(dd3, a.n3, a.d3.W, tid);
        } else {
            const float *w = a.d3.W + (size_t)a.n3 * tid;
            for (int o = 0; o < a.n3; ++o) g = fmaf(dd3[o], w[o], g);
        }
        a.gy2[(size_t)b * 256 + tid] = g;
    }
}

// the maximum over the points: the gradient at pooled from z1 = dd1 (512, in LDS), kept at the winner as gy of the last BatchNorm
__device__ __forceinline__ void head_pool_back(const HeadGtArgs &a, int b, const float *z1) {
    const int tid = threadIdx.x;
    const float gp = transposed_chain(z1, 512, a.d1.W, tid);
    const size_t at = (size_t)b * kFeat + tid;
    a.gy3[at] = a.nstar[at] >= 0 ? gp : 0.0f;
}

// below the head's last BatchNorm (its means in mb / mg): the dropout multiplier, relu(dense2)'s mask, dense2's way back; feat stops
// at its BatchNorm(512), stn / fstn go on through relu(dense1) to the maximum
template <bool FEAT>
__global__ __launch_bounds__(kHeadThreads) void pointnet_gt_head_b_kernel(const HeadGtArgs a) {
    __shared__ float z1[512], z2[256];
    const int b = blockIdx.x, tid = threadIdx.x;
    if (tid < 256) {
        const size_t at = (size_t)b * 256 + tid;
        float g = bn_gv(a.gy2[at], a.xh2[at], a.mb[tid], a.mg[tid], a.bn2.g[tid], bn_sd(a.bn2, tid));
        if (FEAT && a.dropout) g = g * a.dropout[at];
        const float d = a.r2[at] > 0.0f ? g : 0.0f;
        a.dd2[at] = d;
        z2[tid] = d;
    }
    __syncthreads();
    if (tid < 512) {
        const size_t at = (size_t)b * 512 + tid;
        const float g = transposed_chain(z2, 256, a.d2.W, tid);
        if (FEAT) {
            a.gy1[at] = g;
            a.xh1[at] = (a.r1[at] - a.bn1.m[tid]) / bn_sd(a.bn1, tid);
        } else {
            const float d = a.r1[at] > 0.0f ? g : 0.0f;
            a.dd1[at] = d;
            z1[tid] = d;
        }
    }
    if (FEAT) return;
    __syncthreads();
    head_pool_back(a, b, z1);
}

// feat, below its BatchNorm(512)
__global__ __launch_bounds__(kHeadThreads) void pointnet_gt_head_c_kernel(const HeadGtArgs a) {
    __shared__ float z1[512];
    const int b = blockIdx.x, tid = threadIdx.x;
    if (tid < 512) {
        const size_t at = (size_t)b * 512 + tid;
        const float g = bn_gv(a.gy1[at], a.xh1[at], a.mb[tid], a.mg[tid], a.bn1.g[tid], bn_sd(a.bn1, tid));
        const float d = a.r1[at] > 0.0f ? g : 0.0f;
        a.dd1[at] = d;
        z1[tid] = d;
    }
    __syncthreads();
    head_pool_back(a, b, z1);
}

// a BatchNorm whose values are (C, B): thread c, one Float64 chain over b ascending; with nstar over the clouds that have a winner
__global__ __launch_bounds__(256) void pointnet_gt_cloud_sums_kernel(const float *__restrict__ gy, const float *__restrict__ xh,
                                                                     const int32_t *__restrict__ nstar, int C, int B, const BnOut o) {
    const int c = blockIdx.x * 256 + threadIdx.x;  // C is a multiple of 256
    PairSum t;
    for (int b = 0; b < B; ++b) {
        const size_t at = (size_t)b * C + c;
        if (nstar != nullptr && nstar[at] < 0) continue;
        t.add(gy[at], xh[at]);
    }
    finish_bn(o, c, t.s1, t.s2);
}

// ---- the rounds' last layer: pointnet_net.h's last_back and last_pgrad at CIN = 128, the image stride kLd -----------------------------
struct RoundLastArgs : LastArgs {
    PointArgs p;  // the round at the batch statistics
    float *a2;    // (128, N, B): the last convolution's input, written here and read by last_pgrad (LastArgs::in)
};

template <int MODE>
__global__ __launch_bounds__(kPtThreads) void pointnet_gt_last_bwd_kernel(const RoundLastArgs a) {
    extern __shared__ float lds[];
    const int tile = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
    const int p0 = tile * kTile;
    const int nvalid = min(kTile, a.N - p0);
    round_trunk<MODE, kLastLayer[MODE], false>(a.p, lds, b, p0, nvalid, [&](const float *in, const Conv &c, auto layer) {
        float *D = in == lds ? lds + kImg : lds;  // the image the last layer's input does not live in
        const size_t row0 = ((size_t)b * a.N + p0) * 128;
        for (int i = tid; i < nvalid * 128; i += kPtThreads) a.a2[row0 + i] = in[(i >> 7) * kLd + (i & 127)];
        last_back<128, kLd, decltype(layer)::EPI>(in, D, c, a, b, p0, nvalid);
    });
}

template <int EPI>
__global__ __launch_bounds__(kPgradThreads) void pointnet_gt_last_pgrad_kernel(const LastArgs a) {
    extern __shared__ float lds[];
    last_pgrad<128, kLd, EPI>(lds, a);
}

// ---- the BatchNorms below a round's last: their Float64 tile sums -------------------------------------------------------------------
struct SumArgs {
    PointArgs p;
    const float *g;  // (C, N, B): the gradient at the BatchNorm's output (conv_block1: at h, before its relu's mask)
    double *sums;    // (2, C, ntiles, B)
};

// gy of the BatchNorm from what arrives: conv_block1 (BatchNorm, then relu) masks on the relu's output
template <int EPI>
__device__ __forceinline__ float bn_gy(float g, float pre, const Bn &bn, int o, float sd) {
    if (EPI != kBnRelu) return g;
    return relu(batchnorm(pre, bn.g[o], bn.b[o], bn.m[o], sd)) > 0.0f ? g : 0.0f;
}

// conv_stat_mfma of pointnet_train.hip with (gy, xh) in the place of v; gt: the tile's rows of g
template <int CIN, int COUT, int EPI>
__device__ __forceinline__ void grad_stat_mfma(const float *in, const Conv &c, int nvalid, const float *__restrict__ gt,
                                               double *__restrict__ sums) {
    for_each_slab<CIN>(in, c.W, COUT, [&](int o, int h, const f32x16 &acc0, const f32x16 &acc1) {
        const float bi = c.b[o], mu = c.bn.m[o], sd = bn_sd(c.bn, o);
        PairSum t;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int p = mfma_row(r, h);
            if (p < nvalid) {
                const float pre = before_bn<EPI>(acc0[r], bi);
                t.add(bn_gy<EPI>(gt[(size_t)p * COUT + o], pre, c.bn, o, sd), (pre - mu) / sd);
            }
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int p = mfma_row(r, h) + 32;
            if (p < nvalid) {
                const float pre = before_bn<EPI>(acc1[r], bi);
                t.add(bn_gy<EPI>(gt[(size_t)p * COUT + o], pre, c.bn, o, sd), (pre - mu) / sd);
            }
        }
        const double o1 = __shfl_xor(t.s1, 32, 64), o2 = __shfl_xor(t.s2, 32, 64);
        if (h == 0) {
            sums[2 * o] = t.s1 + o1;
            sums[2 * o + 1] = t.s2 + o2;
        }
    });
}

// conv_stat3 of pointnet_train.hip likewise: waves 0 and 1 are the two chains of a channel
template <int EPI>
__device__ __forceinline__ void grad_stat3(const float *xs, const Conv &c, int nvalid, const float *__restrict__ gt,
                                           double *__restrict__ sums) {
    __shared__ double other[2][64];
    const int o = threadIdx.x & 63, h = threadIdx.x >> 6;
    PairSum t;
    if (h < 2) {
        const float w0 = c.W[3 * o], w1 = c.W[3 * o + 1], w2 = c.W[3 * o + 2], bi = c.b[o], mu = c.bn.m[o], sd = bn_sd(c.bn, o);
        for (int q = 0; q < 8; ++q)
            for (int i = 0; i < 4; ++i) {
                const int p = 8 * q + 4 * h + i;
                if (p >= nvalid) continue;
                float acc = 0.0f;
                acc = fmaf(xs[p * 3 + 0], w0, acc);
                acc = fmaf(xs[p * 3 + 1], w1, acc);
                acc = fmaf(xs[p * 3 + 2], w2, acc);
                const float pre = before_bn<EPI>(acc, bi);
                t.add(bn_gy<EPI>(gt[(size_t)p * 64 + o], pre, c.bn, o, sd), (pre - mu) / sd);
            }
    }
    if (h == 1) { other[0][o] = t.s1; other[1][o] = t.s2; }
    __syncthreads();
    if (h == 0) {
        sums[2 * o] = t.s1 + other[0][o];
        sums[2 * o + 1] = t.s2 + other[1][o];
    }
}

template <int MODE, int L>
__global__ __launch_bounds__(kPtThreads) void pointnet_gt_sums_kernel(const SumArgs s) {
    extern __shared__ float lds[];
    const int tile = blockIdx.x, b = blockIdx.y;
    const int p0 = tile * kTile;
    const int nvalid = min(kTile, s.p.N - p0);
    round_trunk<MODE, L, false>(s.p, lds, b, p0, nvalid, [&](const float *in, const Conv &c, auto layer) {
        using Ly = decltype(layer);
        double *sums = s.sums + 2 * ((size_t)b * s.p.ntiles + tile) * Ly::COUT;
        const float *gt = s.g + ((size_t)b * s.p.N + p0) * Ly::COUT;
        if constexpr (Ly::CIN == 3) grad_stat3<Ly::EPI>(in, c, nvalid, gt, sums);
        else grad_stat_mfma<Ly::CIN, Ly::COUT, Ly::EPI>(in, c, nvalid, gt, sums);
    });
}

__global__ __launch_bounds__(kFinishThreads) void pointnet_gt_finish_kernel(const double *__restrict__ sums, int C, long long T,
                                                                          const BnOut o) {
    fold_tile_sums(sums, C, T, [&](int c, double s1, double s2) { finish_bn(o, c, s1, s2); });
}

// ---- a layer below a round's last, once its BatchNorm's sums are known --------------------------------------------------------------
struct LayerArgs {
    PointArgs p;
    const float *g;        // (COUT, N, B): the gradient at the layer's BatchNorm output (conv_block1: at h)
    const float *mb, *mg;  // (COUT)
    float *part;           // (psize, ntiles, B): W (CIN COUT) | b (COUT) | gF (4096) or gT (9) where the round has one
    int psize;
    float *gin;            // (64, N, B): the gradient at the layer's input; (1, 1): at h, both paths; (2, 0): the feat path at h
    const float *ghf;      // (1, 1): the feat path at h
    float *gxt;            // (3, N, B): written by (1, 0), read by (0, 0)
    float *gx;             // (0, 0), optional
    const float *T;        // (0, 0): the input transform (3, 3, B)
};

template <int MODE, int L>
__global__ __launch_bounds__(kPtThreads) void pointnet_gt_layer_bwd_kernel(const LayerArgs a) {
    extern __shared__ float lds[];
    const int tile = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
    const int p0 = tile * kTile;
    const int nvalid = min(kTile, a.p.N - p0);
    round_trunk<MODE, L, false>(a.p, lds, b, p0, nvalid, [&](const float *in, const Conv &c, auto layer) {
        using Ly = decltype(layer);
        constexpr int CIN = Ly::CIN, COUT = Ly::COUT, EPI = Ly::EPI;
        float *R = in == lds ? lds + kImg : lds, *G = lds + kThird;
        const float *xs = lds + 2 * kImg;
        float *part = a.part + ((size_t)b * a.p.ntiles + tile) * a.psize;
        const size_t pt0 = (size_t)b * a.p.N + p0;
        // R: the relu's output (conv_block1: the contraction, its bias is added in the column pass); G: what arrives
        if constexpr (CIN == 3) conv3<(EPI == kBnRelu ? kNone : kRelu)>(in, R, kLd, 64, c.W, c.b, c.bn);
        else conv_mfma<CIN, kRelu, false>(in, R, COUT, c.W, c.b, c.bn, nvalid, nullptr);
        {
            const float *gt = a.g + pt0 * COUT;
            for (int i = tid; i < kTile * COUT; i += kPtThreads) G[(i / COUT) * kLd + (i % COUT)] = i < nvalid * COUT ? gt[i] : 0.0f;
        }
        __syncthreads();
        // the column pass, thread o: d takes gy's place; db of the tile, rows ascending
        if (tid < COUT) {
            const int o = tid;
            const float bi = c.b[o], gam = c.bn.g[o], mu = c.bn.m[o], sd = bn_sd(c.bn, o), mb = a.mb[o], mg = a.mg[o];
            float sb = 0.0f;
            for (int p = 0; p < nvalid; ++p) {
                const float rv = R[p * kLd + o];
                float d;
                if (EPI == kBnRelu) {
                    const float pre = rv + bi;
                    d = bn_gv(bn_gy<EPI>(G[p * kLd + o], pre, c.bn, o, sd), (pre - mu) / sd, mb, mg, gam, sd);
                } else {
                    const float g = bn_gv(G[p * kLd + o], (rv - mu) / sd, mb, mg, gam, sd);
                    d = rv > 0.0f ? g : 0.0f;
                }
                sb = sb + d;
                G[p * kLd + o] = d;
            }
            for (int p = nvalid; p < kTile; ++p) G[p * kLd + o] = 0.0f;
            part[CIN * COUT + o] = sb;
        }
        __syncthreads();
        if constexpr (CIN == 3) {
            hsum3(in, G, nvalid, 0, part);
            if (tid < kTile * 3) {
                const int p = tid / 3, i = tid - 3 * p;
                float acc = 0.0f;  // the chain over the layer's outputs
                if (p < nvalid)
                    for (int o = 0; o < 64; ++o) acc = fmaf(G[p * kLd + o], c.W[i + 3 * o], acc);
                if constexpr (MODE == 0) {
                    if (a.gx != nullptr && p < nvalid) {  // the path through T: over j
                        const float *g = a.gxt + (pt0 + p) * 3, *T = a.T + (size_t)b * 9;
                        float tp = 0.0f;
                        for (int jj = 0; jj < 3; ++jj) tp = fmaf(g[jj], T[i + 3 * jj], tp);
                        a.gx[(pt0 + p) * 3 + i] = tp + acc;
                    }
                } else {
                    if (p < nvalid) a.gxt[(pt0 + p) * 3 + i] = acc;
                    R[p * kLd + 64 + i] = acc;  // beside the contraction, for gT
                }
            }
            if constexpr (MODE == 1) {
                __syncthreads();
                if (tid < 9) {  // gT[i, j] = the chain over the tile's valid rows of x[i, n] gxt[j, n]
                    const int i = tid % 3, jj = tid / 3;
                    float acc = 0.0f;
                    for (int p = 0; p < nvalid; ++p) acc = fmaf(xs[p * 3 + i], R[p * kLd + 64 + jj], acc);
                    part[CIN * COUT + COUT + tid] = acc;
                }
            }
        } else {
            hsum_mfma(in, G, CIN, COUT, part);
            back_mfma<COUT>(G, R, 64, c.W);  // the gradient at the layer's input, in the relu's place
            __syncthreads();
            float *go = a.gin + pt0 * 64;
            if constexpr (MODE == 2) {
                load_tile64(G, a.p.h, b, a.p.N, p0, nvalid);  // h again, in d's place
                __syncthreads();
                hsum_mfma(G, R, 64, 64, part + CIN * COUT + COUT);       // gF[i, j] = sum_n h[i, n] g[j, n]
                back_mfma<64>(R, R + 64, 64, a.p.tf + (size_t)b * 4096);  // the feat path into h: the chain over j of g[j] F[i, j]
                __syncthreads();
                for (int i = tid; i < nvalid * 64; i += kPtThreads) go[i] = R[(i >> 6) * kLd + 64 + (i & 63)];
            } else if constexpr (MODE == 1 && L == 1) {
                const float *gf = a.ghf + pt0 * 64;
                for (int i = tid; i < nvalid * 64; i += kPtThreads) go[i] = gf[i] + R[(i >> 6) * kLd + (i & 63)];  // feat + fstn
            } else {
                for (int i = tid; i < nvalid * 64; i += kPtThreads) go[i] = R[(i >> 6) * kLd + (i & 63)];
            }
        }
    });
}

// ---- the host side -----------------------------------------------------------------------------------------------------------------
constexpr int kPartMax = 64 * 128 + 128 + 4096;  // feat.conv1 with gF

struct GtWs {
    size_t h, T, F, tmax[3], tfirst[3], tpre[3];
    size_t nstar, pooled, r1, a1, r2, a2h, dd1, dd2, dd3, gy1, xh1, gy2, xh2, gy3, xh3, coef, sums;
    size_t a2, g128, g64, ghf, gh, gxt, gT, gF, Hc, hc, part, total;
    int ntiles;
};
GtWs gt_ws(int N, int B, int nc) {
    GtWs w;
    w.ntiles = (N + kTile - 1) / kTile;
    const size_t f = sizeof(float), nb = (size_t)N * B, tb = (size_t)kFeat * w.ntiles * B;
    WsBump ws;
    w.h = ws.put(64 * nb * f);
    w.T = ws.put((size_t)9 * B * f);
    w.F = ws.put((size_t)4096 * B * f);
    for (int r = 0; r < 3; ++r) {
        w.tmax[r] = ws.put(tb * f);
        w.tfirst[r] = ws.put(tb * sizeof(int32_t));
        w.tpre[r] = ws.put(tb * f);
    }
    w.nstar = ws.put((size_t)kFeat * B * sizeof(int32_t));
    w.pooled = ws.put((size_t)kFeat * B * f);
    w.r1 = ws.put((size_t)512 * B * f);
    w.a1 = ws.put((size_t)512 * B * f);
    w.r2 = ws.put((size_t)256 * B * f);
    w.a2h = ws.put((size_t)256 * B * f);
    w.dd1 = ws.put((size_t)512 * B * f);
    w.dd2 = ws.put((size_t)256 * B * f);
    w.dd3 = ws.put((size_t)(nc > 4096 ? nc : 4096) * B * f);
    w.gy1 = ws.put((size_t)512 * B * f);
    w.xh1 = ws.put((size_t)512 * B * f);
    w.gy2 = ws.put((size_t)256 * B * f);
    w.xh2 = ws.put((size_t)256 * B * f);
    w.gy3 = ws.put((size_t)kFeat * B * f);
    w.xh3 = ws.put((size_t)kFeat * B * f);
    w.coef = ws.put((size_t)2 * kFeat * f);
    w.sums = ws.put((size_t)2 * 128 * w.ntiles * B * sizeof(double));
    w.a2 = ws.put(128 * nb * f);
    w.g128 = ws.put(128 * nb * f);
    w.g64 = ws.put(64 * nb * f);
    w.ghf = ws.put(64 * nb * f);
    w.gh = ws.put(64 * nb * f);
    w.gxt = ws.put(3 * nb * f);
    w.gT = ws.put((size_t)9 * B * f);
    w.gF = ws.put((size_t)4096 * B * f);
    w.Hc = ws.put((size_t)128 * kFeat * B * f);
    w.hc = ws.put((size_t)kFeat * B * f);
    w.part = ws.put((size_t)kPartMax * w.ntiles * B * f);
    w.total = ws.at;
    return w;
}

fx3d_status check_gt_sizes(const char *fn, int32_t N, int32_t B, int32_t nc) {
    const fx3d_status rc = check_sizes(fn, N, B, nc);
    if (rc != FX3D_OK) return rc;
    FX3D_REQUIRE(B >= 2, "%s: training-mode BatchNorm needs B >= 2 clouds (fx3d_pointnet_forward_train's limit), got %d", fn, B);
    return FX3D_OK;
}

template <int MODE, int L>
fx3d_status launch_sums(const SumArgs &s, int B, hipStream_t st) {
    return launch_tile(&pointnet_gt_sums_kernel<MODE, L>, "pointnet_gt_sums_kernel", "pointnet_gt_sums", kPtLds, s.p.ntiles, B, kPtThreads,
                       st, s);
}
template <int MODE, int L>
fx3d_status launch_layer(const LayerArgs &a, int B, hipStream_t st) {
    return launch_tile(&pointnet_gt_layer_bwd_kernel<MODE, L>, "pointnet_gt_layer_bwd_kernel", "pointnet_gt_layer_bwd", kLayerLds,
                       a.p.ntiles, B, kPtThreads, st, a);
}
fx3d_status launch_last(int mode, const RoundLastArgs &a, int B, hipStream_t st) {
    const char *nm = "pointnet_gt_last_bwd_kernel", *lb = "pointnet_gt_last_bwd";
    if (mode == 0) return launch_tile(&pointnet_gt_last_bwd_kernel<0>, nm, lb, kPtLds, a.ntiles, B, kPtThreads, st, a);
    if (mode == 1) return launch_tile(&pointnet_gt_last_bwd_kernel<1>, nm, lb, kPtLds, a.ntiles, B, kPtThreads, st, a);
    return launch_tile(&pointnet_gt_last_bwd_kernel<2>, nm, lb, kPtLds, a.ntiles, B, kPtThreads, st, a);
}
fx3d_status launch_last_pgrad(int mode, const LastArgs &a, int B, hipStream_t st) {
    const char *nm = "pointnet_gt_last_pgrad_kernel", *lb = "pointnet_gt_last_pgrad";
    if (mode == 2) return launch_tile(&pointnet_gt_last_pgrad_kernel<kBnOnly>, nm, lb, kPgradLds, kFeat / kGroup, B, kPgradThreads, st, a);
    return launch_tile(&pointnet_gt_last_pgrad_kernel<kReluBn>, nm, lb, kPgradLds, kFeat / kGroup, B, kPgradThreads, st, a);
}

}  // namespace

namespace fx3d {
namespace mlp {
namespace pointnet {
fx3d_status launch_cloud_sums(const float *gy, const float *xh, const int32_t *nstar, int C, int B, const BnOut &o, hipStream_t st) {
    hipLaunchKernelGGL(pointnet_gt_cloud_sums_kernel, dim3(C / 256), dim3(256), 0, st, gy, xh, nstar, C, B, o);
    FX3D_LAUNCH_CHECK();
    return FX3D_OK;
}
}  // namespace pointnet
}  // namespace mlp
}  // namespace fx3d

extern "C" {

fx3d_status fx3d_pointnet_grad_train_workspace_bytes(int32_t N, int32_t B, int32_t num_classes, size_t *bytes) {
    FX3D_REQUIRE(bytes != nullptr, "fx3d_pointnet_grad_train_workspace_bytes: bytes is NULL");
    const fx3d_status rc = check_gt_sizes("fx3d_pointnet_grad_train_workspace_bytes", N, B, num_classes);
    if (rc != FX3D_OK) return rc;
    *bytes = gt_ws(N, B, num_classes).total;
    return FX3D_OK;
}

fx3d_status fx3d_pointnet_grad_train(const float *params_dev, int32_t num_classes, const float *x, int32_t N, int32_t B,
                                     const float *dropout, const float *batch_stats, const float *glogits, float *gparams, float *gx,
                                     float *gstn, float *gfstn, float *gh, float *gxt, void *ws, size_t ws_bytes, fx3d_stream_t s) {
    const char *fn = "fx3d_pointnet_grad_train";
    FX3D_REQUIRE(params_dev && x && batch_stats && glogits && gparams && ws,
                 "%s: params_dev, x, batch_stats, glogits, gparams and ws must not be NULL", fn);
    fx3d_status r = check_gt_sizes(fn, N, B, num_classes);
    if (r != FX3D_OK) return r;
    const GtWs w = gt_ws(N, B, num_classes);
    FX3D_REQUIRE(ws_bytes >= w.total, "%s: workspace of %zu bytes, fx3d_pointnet_grad_train_workspace_bytes says %zu", fn, ws_bytes,
                 w.total);
    FX3D_REQUIRE((reinterpret_cast<uintptr_t>(ws) & 255) == 0, "%s: ws must be 256-byte aligned", fn);
    const Net n = with_batch_stats(layout(params_dev, num_classes), batch_stats), gn = layout(gparams, num_classes);
    hipStream_t st = as_stream(s);
    const WsView v{static_cast<char *>(ws)};
    float *T = v.f32(w.T), *F = v.f32(w.F), *gT = gstn ? gstn : v.f32(w.gT), *gF = gfstn ? gfstn : v.f32(w.gF);
    float *gxt_ = gxt ? gxt : v.f32(w.gxt), *gh_ = gh ? gh : v.f32(w.gh);
    float *mb = v.f32(w.coef), *mg = mb + kFeat;
    const int nt = w.ntiles;
    const long long ntl = (long long)nt * B, npts = (long long)N * B;

    // the forward's three rounds at the batch statistics, each with its winners per tile
    PointArgs p{};
    p.x = x; p.h = v.f32(w.h); p.N = N; p.ntiles = nt;
    for (int mode = 0; mode < 3; ++mode) {
        set_round(p, n, mode, T, F);
        p.tmax = v.f32(w.tmax[mode]); p.tfirst = v.i32(w.tfirst[mode]); p.tpre = v.f32(w.tpre[mode]);
        if ((r = launch_points(mode, true, p, B, st)) != FX3D_OK) return r;
        if (mode < 2 && (r = launch_head(false, stn_head(n, mode, p.tmax, nt, T, F, nullptr), B, st)) != FX3D_OK) return r;
    }

    HeadGtArgs hb{};
    hb.dropout = dropout; hb.mb = mb; hb.mg = mg; hb.nstar = v.i32(w.nstar);
    hb.r1 = v.f32(w.r1); hb.a1 = v.f32(w.a1); hb.r2 = v.f32(w.r2); hb.a2 = v.f32(w.a2h);
    hb.dd1 = v.f32(w.dd1); hb.dd2 = v.f32(w.dd2); hb.dd3 = v.f32(w.dd3);
    hb.gy1 = v.f32(w.gy1); hb.xh1 = v.f32(w.xh1); hb.gy2 = v.f32(w.gy2); hb.xh2 = v.f32(w.xh2);
    hb.gy3 = v.f32(w.gy3); hb.xh3 = v.f32(w.xh3);
    auto head_of = [&](const Net &net, int k) {
        const float *tmax = v.f32(w.tmax[k]);
        return k == 2 ? feat_head(net, num_classes, tmax, nt, nullptr, nullptr, nullptr) : stn_head(net, k, tmax, nt, T, F, nullptr);
    };
    auto bn_out = [&](const Bn &g, long long m) { return BnOut{grad_block(g), mb, mg, m}; };
    auto cloud_sums = [&](const float *gy, const float *xh, const int32_t *ns, int C, const BnOut &o) {
        return launch_cloud_sums(gy, xh, ns, C, B, o, st);
    };
    // round k's head: its adjoint cut at the dense BatchNorms, down to gy of the round's last BatchNorm and that BatchNorm's sums;
    // then the dense layers' sums over the clouds
    auto head_round = [&](int k, const Conv &c3, const Conv &g3, const float *gup) -> fx3d_status {
        ProfileScope prof("pointnet_gt_head", st);
        const bool feat = k == 2;
        static_cast<HeadArgs &>(hb) = head_of(n, k);
        const HeadArgs g = head_of(gn, k);
        hb.pooled = v.f32(w.pooled); hb.tfirst = v.i32(w.tfirst[k]); hb.tpre = v.f32(w.tpre[k]); hb.bn3 = c3.bn; hb.gup = gup;
        if (feat) hipLaunchKernelGGL(pointnet_gt_head_a_kernel<true>, dim3(B), dim3(kHeadThreads), 0, st, hb);
        else hipLaunchKernelGGL(pointnet_gt_head_a_kernel<false>, dim3(B), dim3(kHeadThreads), 0, st, hb);
        FX3D_LAUNCH_CHECK();
        if ((r = cloud_sums(hb.gy2, hb.xh2, nullptr, 256, bn_out(g.bn2, B))) != FX3D_OK) return r;
        if (feat) hipLaunchKernelGGL(pointnet_gt_head_b_kernel<true>, dim3(B), dim3(kHeadThreads), 0, st, hb);
        else hipLaunchKernelGGL(pointnet_gt_head_b_kernel<false>, dim3(B), dim3(kHeadThreads), 0, st, hb);
        FX3D_LAUNCH_CHECK();
        if (feat) {
            if ((r = cloud_sums(hb.gy1, hb.xh1, nullptr, 512, bn_out(g.bn1, B))) != FX3D_OK) return r;
            hipLaunchKernelGGL(pointnet_gt_head_c_kernel, dim3(B), dim3(kHeadThreads), 0, st, hb);
            FX3D_LAUNCH_CHECK();
        }
        if ((r = cloud_sums(hb.gy3, hb.xh3, hb.nstar, kFeat, bn_out(g3.bn, npts))) != FX3D_OK) return r;
        const DenseSums s1{hb.dd1, hb.pooled, kFeat, 512, B, mut(g.d1.W), mut(g.d1.b)}, s2{hb.dd2, hb.a1, 512, 256, B, mut(g.d2.W), mut(g.d2.b)},
            s3{hb.dd3, hb.a2, 256, g.n3, B, mut(g.d3.W), mut(g.d3.b)};
        for (const DenseSums &q : {s1, s2, s3})
            if ((r = launch_dense_sums(q, st)) != FX3D_OK) return r;
        return FX3D_OK;
    };

    RoundLastArgs la{};
    la.nstar = hb.nstar; la.gy3 = hb.gy3; la.mb = mb; la.mg = mg; la.a2 = v.f32(w.a2); la.in = la.a2; la.g = v.f32(w.g128);
    la.Hc = v.f32(w.Hc); la.hc = v.f32(w.hc); la.N = N; la.ntiles = nt;
    // the round's last layer: the gradient at its input (all points), then dW and db per cloud and their sums over b ascending
    auto last_round = [&](int k, const Conv &c3, const Conv &g3) -> fx3d_status {
        la.p = p; la.c3 = c3;
        if ((r = launch_last(k, la, B, st)) != FX3D_OK) return r;
        if ((r = launch_last_pgrad(k, la, B, st)) != FX3D_OK) return r;
        ProfileScope prof("pointnet_gt_reduce", st);
        ReduceArgs ra{};
        ra.part = la.Hc; ra.psize = 128 * kFeat; ra.nparts = B; ra.s[0] = Seg{0, mut(g3.W), 128 * kFeat, 0};
        if ((r = launch_reduce(ra, 1, st)) != FX3D_OK) return r;
        ra.part = la.hc; ra.psize = kFeat; ra.s[0] = Seg{0, mut(g3.b), kFeat, 0};
        return launch_reduce(ra, 1, st);
    };

    SumArgs sa{};
    sa.sums = v.f64(w.sums);
    LayerArgs ly{};
    ly.mb = mb; ly.mg = mg; ly.part = v.f32(w.part); ly.ghf = v.f32(w.ghf); ly.gxt = gxt_; ly.gx = gx; ly.T = T;
    // BatchNorm L of the round (its convolution c, the gradient's g): the sums of what arrives in `up`, then the layer's adjoint,
    // which leaves the gradient at its input in `down`, and the chains over its tile partials
    auto finish = [&](const Conv &g, int C) -> fx3d_status {
        ProfileScope prof("pointnet_gt_finish", st);
        hipLaunchKernelGGL(pointnet_gt_finish_kernel, dim3(C / kFinishChannels), dim3(kFinishThreads), 0, st, sa.sums, C, ntl,
                           bn_out(g.bn, npts));
        FX3D_LAUNCH_CHECK();
        return FX3D_OK;
    };
    auto reduce = [&](const Conv &g, int cin, int cout) -> fx3d_status {
        ProfileScope prof("pointnet_gt_reduce", st);
        ReduceArgs ra{};
        ra.part = ly.part; ra.psize = ly.psize; ra.nparts = nt * B; ra.s[0] = Seg{0, mut(g.W), cin * cout + cout, 0};
        return launch_reduce(ra, 1, st);
    };
#define FX3D_GT_LAYER(MODE, L, G, CIN, COUT, UP, DOWN, EXTRA)                                \
    do {                                                                                     \
        sa.p = p; sa.g = (UP);                                                               \
        if ((r = launch_sums<MODE, L>(sa, B, st)) != FX3D_OK) return r;                      \
        if ((r = finish((G), (COUT))) != FX3D_OK) return r;                                  \
        ly.p = p; ly.g = (UP); ly.gin = (DOWN); ly.psize = (CIN) * (COUT) + (COUT) + (EXTRA); \
        if ((r = launch_layer<MODE, L>(ly, B, st)) != FX3D_OK) return r;                     \
        if ((r = reduce((G), (CIN), (COUT))) != FX3D_OK) return r;                           \
    } while (0)

    float *g128 = v.f32(w.g128), *g64 = v.f32(w.g64);
    // feat and cls
    set_round(p, n, 2, T, F);
    if ((r = head_round(2, n.f2, gn.f2, glogits)) != FX3D_OK) return r;
    if ((r = last_round(2, n.f2, gn.f2)) != FX3D_OK) return r;
    FX3D_GT_LAYER(2, 0, gn.f1, 64, 128, g128, v.f32(w.ghf), 4096);
    if ((r = launch_cloud_reduce(ly.part, ly.psize, 64 * 128 + 128, nt, 4096, B, gF, st)) != FX3D_OK) return r;

    // fstn, conv_block1 and the input transform
    set_round(p, n, 1, T, F);
    if ((r = head_round(1, n.fstn.c3, gn.fstn.c3, gF)) != FX3D_OK) return r;
    if ((r = last_round(1, n.fstn.c3, gn.fstn.c3)) != FX3D_OK) return r;
    FX3D_GT_LAYER(1, 2, gn.fstn.c2, 64, 128, g128, g64, 0);
    FX3D_GT_LAYER(1, 1, gn.fstn.c1, 64, 64, g64, gh_, 0);
    FX3D_GT_LAYER(1, 0, gn.block1, 3, 64, gh_, nullptr, 9);
    if ((r = launch_cloud_reduce(ly.part, ly.psize, 3 * 64 + 64, nt, 9, B, gT, st)) != FX3D_OK) return r;

    // stn, and the two paths into x
    set_round(p, n, 0, T, F);
    if ((r = head_round(0, n.stn.c3, gn.stn.c3, gT)) != FX3D_OK) return r;
    if ((r = last_round(0, n.stn.c3, gn.stn.c3)) != FX3D_OK) return r;
    FX3D_GT_LAYER(0, 1, gn.stn.c2, 64, 128, g128, g64, 0);
    FX3D_GT_LAYER(0, 0, gn.stn.c1, 3, 64, g64, nullptr, 0);
#undef FX3D_GT_LAYER
    return FX3D_OK;
}

}  // extern "C"
