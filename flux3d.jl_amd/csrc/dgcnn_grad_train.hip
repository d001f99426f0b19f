// DGCNN's training-mode adjoint (gfx950): the gradients of sum(glogits . logits) for the logits of fx3d_dgcnn_forward_train with
// respect to every parameter and to the input points, Float32, mu and sigma2 of all 8 BatchNorms functions of the batch, the
// dropout multipliers and both neighbour lists constants.  include/flux3d_hip.h ("DGCNN training-mode adjoint") states the
// definition and the order of every sum; tests/dgcnn_grad_train_ref.py restates it on the host.  The two EdgeConv stages are
// fx3d_edgeconv_grad_train itself (edgeconv_grad_train.hip) on the ec2 and then the ec1 slice of the parameters and of the
// statistics; this file is the tail: conv_3, the maximum over the points, fc_4, fc_5, fc_6.
//
// Through a batch-statistic BatchNorm the maximum no longer makes conv_3's adjoint a gather: gv = (((gy - mb) - xh mg) gamma) / sd
// is non-zero at every row of every cloud, so conv_3's input gradient and its dW are dense contractions (pointnet_grad_train.hip's
// last layer, with a 256-channel input in the 258-stride image and the block order conv, BatchNorm, relu).  Per call:
//   dgcnn_gt_argmax_kernel: dgcnn_net.h's conv3_winners<true>, the body of dgcnn_argmax_kernel (dgcnn_grad.hip) at the batch
//     statistics -- the forward's tile, slabs and epilogue, compared with pooled where that is positive -- that also keeps conv +
//     bias at the tile's first match.
//   dgcnn_gt_head_{a,b,c}_kernel: the head's adjoint, one block per cloud, cut at fc5.bn and fc4.bn, ended at gy / xh of conv3.bn
//     at the winners; PointNet's pointnet_gt_cloud_sums_kernel after each (launch_cloud_sums): one Float64 chain over b, the third
//     over the clouds that have a winner.  Then dense_sums_kernel on fc_4, fc_5, fc_6 with gv in d's place, straight to gparams.
//   dgcnn_gt_conv3_bwd_kernel: one block = 64 points of one cloud.  The forward's tile (load_x2_tile), then pointnet_net.h's
//     last_back<256, kLd3, kBnRelu>, the body of pointnet_gt_last_bwd_kernel: the slabs four at a time, LastChannel<kBnRelu> forms gv3
//     from the accumulators into a second LDS image, the 16 (32 x 32) tiles of (256 inputs x 64 points), four per wave, kept across
//     the eight groups: one chain over all 1024 outputs ascending.  Stores gx2.
//   dgcnn_gt_conv3_pgrad_kernel: one block of 8 waves per (cloud, 128 outputs): pointnet_net.h's last_pgrad<256, kLd3, kBnRelu>, the
//     body of pointnet_gt_last_pgrad_kernel: (256 x 128) of dW3 as one chain over the cloud's points, four tiles per wave, db3 as one
//     Float32 chain.  pointnet_reduce_kernel (launch_reduce) then sums the clouds in ascending b into gparams.
//   fx3d_edgeconv_grad_train on ec2 (gout = gx2 -> gx1), then on ec1 (gout = gx1 -> gx), sharing one scratch region.
// One stream, no host synchronisation, no atomics: every sum has one owner and one order, which depends on (N, B, K, num_classes)
// alone.
#include <initializer_list>

#include "dgcnn_net.h"
#include "edgeconv_net.h"
#include "pointnet_net.h"

using namespace fx3d;
using namespace fx3d::mlp;
using pointnet::BnOut;
using pointnet::bn_gv;
using pointnet::kGroup;
using pointnet::kNoPoint;
using pointnet::kPgradThreads;
using pointnet::last_back;
using pointnet::last_pgrad;
using pointnet::LastArgs;
using pointnet::launch_tile;

namespace {

constexpr int kImg3 = kTile * kLd3, kImgD = kTile * kLd;
constexpr size_t kDenseLds = (size_t)(kImg3 + kImgD) * sizeof(float);  // the x2 tile | gv3 of 128 outputs: 99328 bytes
static_assert(kDenseLds <= 160 * 1024, "conv_3's dense adjoint: the 258-stride image and the 130-stride image of gv");

// ---- the winners: dgcnn_net.h's conv3_winners, keeping what conv3.bn was given at the first match (tpre; 0 where the tile has none) ---
__global__ __launch_bounds__(kPtThreads) void dgcnn_gt_argmax_kernel(const float *__restrict__ x2, const Conv c,
                                                                     const float *__restrict__ pooled, int32_t *__restrict__ tfirst,
                                                                     float *__restrict__ tpre, int N, int ntiles) {
    extern __shared__ float lds[];
    conv3_winners<true>(lds, x2, c, pooled, tfirst, tpre, N, ntiles);
}

// ---- the head ------------------------------------------------------------------------------------------------------------------------
struct HeadGtArgs {
    const int32_t *tfirst;  // (1024, ntiles, B)
    const float *tpre;
    int ntiles, nc;
    const float *pooled;    // (1024, B)
    const float *glogits;   // (nc, B)
    Conv c3;                // at the batch statistics, as bn4 and bn5
    Dense d4, d5, d6;
    Bn bn4, bn5;
    const float *drop4, *drop5;  // (512, B), (256, B) or NULL
    const float *mb, *mg;        // the means of the BatchNorm the phase starts below
    int32_t *nstar;              // (1024, B): the winning point, -1 where there is none
    float *r4, *in5, *r5, *in6;  // relu(BN(fc_4)) (512, B), fc_5's input; relu(BN(fc_5)) (256, B), fc_6's input
    float *gy4, *xh4, *gv4, *gy5, *xh5, *gv5, *gy3, *xh3;
};

// n* and xh3 at the winner; the forward's head again (dgcnn_train_head_{a,b,c}_kernel's calls); gy and xh of fc5.bn
__global__ __launch_bounds__(kHeadThreads) void dgcnn_gt_head_a_kernel(const HeadGtArgs a) {
    __shared__ float v0[kFeat], v1[512], v2[256];
    const int b = blockIdx.x, tid = threadIdx.x;
    {
        int first = kNoPoint;
        float pre = 0.0f;
        const size_t at = (size_t)b * a.ntiles * kFeat + tid;
        for (int k = a.ntiles - 1; k >= 0; --k)  // descending: the last assignment is the first tile that has a match
            if (a.tfirst[at + (size_t)k * kFeat] != kNoPoint) {
                first = a.tfirst[at + (size_t)k * kFeat];
                pre = a.tpre[at + (size_t)k * kFeat];
            }
        const bool won = first != kNoPoint;
        a.nstar[(size_t)b * kFeat + tid] = won ? first : -1;
        a.xh3[(size_t)b * kFeat + tid] = won ? (pre - a.c3.bn.m[tid]) / pointnet::bn_sd(a.c3.bn, tid) : 0.0f;
    }
    v0[tid] = a.pooled[(size_t)b * kFeat + tid];
    __syncthreads();
    if (tid < 512) {
        const size_t at = (size_t)b * 512 + tid;
        const float v = dense_chain(v0, kFeat, a.d4.W, 512, tid) + a.d4.b[tid];
        const float r = head_bn_relu(a.bn4, v);
        v1[tid] = a.drop4 ? r * a.drop4[at] : r;
        a.r4[at] = r;
        a.in5[at] = v1[tid];
        a.xh4[at] = (v - a.bn4.m[tid]) / pointnet::bn_sd(a.bn4, tid);
    }
    __syncthreads();
    if (tid < 256) {
        const size_t at = (size_t)b * 256 + tid;
        const float v = dense_chain(v1, 512, a.d5.W, 256, tid) + a.d5.b[tid];
        const float r = head_bn_relu(a.bn5, v);
        v2[tid] = a.drop5 ? r * a.drop5[at] : r;
        a.in6[at] = v2[tid];
        a.xh5[at] = (v - a.bn5.m[tid]) / pointnet::bn_sd(a.bn5, tid);
        // the gradient at the block's output: one chain over the classes ascending; the multiplier, then the relu's own mask
        const float *d6 = a.glogits + (size_t)b * a.nc;
        float g = 0.0f;
        if ((a.nc & 3) == 0) {
            g = transposed_chain(d6, a.nc, a.d6.W, tid);
        } else {
            const float *w = a.d6.W + (size_t)a.nc * tid;
            for (int o = 0; o < a.nc; ++o) g = fmaf(d6[o], w[o], g);
        }
        if (a.drop5) g = g * a.drop5[at];
        a.gy5[at] = r > 0.0f ? g : 0.0f;
    }
}

// below fc5.bn (its means in mb / mg): gv5, fc_5's way back, the multiplier, relu(BN(fc_4))'s mask: gy and xh of fc4.bn
__global__ __launch_bounds__(512) void dgcnn_gt_head_b_kernel(const HeadGtArgs a) {
    __shared__ float z2[256];
    const int b = blockIdx.x, tid = threadIdx.x;
    if (tid < 256) {
        const size_t at = (size_t)b * 256 + tid;
        const float g = bn_gv(a.gy5[at], a.xh5[at], a.mb[tid], a.mg[tid], a.bn5.g[tid], pointnet::bn_sd(a.bn5, tid));
        a.gv5[at] = g;
        z2[tid] = g;
    }
    __syncthreads();
    const size_t at = (size_t)b * 512 + tid;
    float g = transposed_chain(z2, 256, a.d5.W, tid);
    if (a.drop4) g = g * a.drop4[at];
    a.gy4[at] = a.r4[at] > 0.0f ? g : 0.0f;
}

// below fc4.bn: gv4, fc_4's way back to pooled, kept at the winner as gy of conv3.bn
__global__ __launch_bounds__(kHeadThreads) void dgcnn_gt_head_c_kernel(const HeadGtArgs a) {
    __shared__ float z1[512];
    const int b = blockIdx.x, tid = threadIdx.x;
    if (tid < 512) {
        const size_t at = (size_t)b * 512 + tid;
        const float g = bn_gv(a.gy4[at], a.xh4[at], a.mb[tid], a.mg[tid], a.bn4.g[tid], pointnet::bn_sd(a.bn4, tid));
        a.gv4[at] = g;
        z1[tid] = g;
    }
    __syncthreads();
    const float gp = transposed_chain(z1, 512, a.d4.W, tid);
    const size_t at = (size_t)b * kFeat + tid;
    a.gy3[at] = a.nstar[at] >= 0 ? gp : 0.0f;
}

// ---- conv_3, dense: pointnet_net.h's last_back and last_pgrad at CIN = 256, the image stride kLd3, the block order conv, BatchNorm, relu
__global__ __launch_bounds__(kPtThreads) void dgcnn_gt_conv3_bwd_kernel(const LastArgs a) {
    extern __shared__ float lds[];
    const int tile = blockIdx.x, b = blockIdx.y;
    const int p0 = tile * kTile;
    const int nvalid = min(kTile, a.N - p0);
    load_x2_tile(lds, a.in, b, a.N, p0, nvalid);
    __syncthreads();
    last_back<256, kLd3, kBnRelu>(lds, lds + kImg3, a.c3, a, b, p0, nvalid);
}

__global__ __launch_bounds__(kPgradThreads) void dgcnn_gt_conv3_pgrad_kernel(const LastArgs a) {
    extern __shared__ float lds[];
    last_pgrad<256, kLd3, kBnRelu>(lds, a);
}

// ---- the host side -------------------------------------------------------------------------------------------------------------------
// The workspace: the per-tile first matches and what conv3.bn was given there | n* | the head's vectors | the means | dW3 and db3
// per cloud | gx2, gx1 (used where the caller gives none) | one scratch region, the larger of the two stages'
// fx3d_edgeconv_grad_train workspaces, which use it in turn
struct GtWs {
    size_t tfirst, tpre, nstar, r4, in5, r5, in6, gy4, xh4, gv4, gy5, xh5, gv5, gy3, xh3, coef, Hc, hc, gx2, gx1, scratch, total;
    size_t ec1_bytes, ec2_bytes;
    int ntiles;
};
fx3d_status gt_ws(int N, int B, int K, GtWs *w) {
    w->ntiles = (N + kTile - 1) / kTile;
    const size_t f = sizeof(float), nb = (size_t)N * B, tb = (size_t)kFeat * w->ntiles * B;
    WsBump ws;
    w->tfirst = ws.put(tb * sizeof(int32_t));
    w->tpre = ws.put(tb * f);
    w->nstar = ws.put((size_t)kFeat * B * sizeof(int32_t));
    for (size_t *at : {&w->r4, &w->in5, &w->gy4, &w->xh4, &w->gv4}) *at = ws.put((size_t)512 * B * f);
    for (size_t *at : {&w->r5, &w->in6, &w->gy5, &w->xh5, &w->gv5}) *at = ws.put((size_t)256 * B * f);
    w->gy3 = ws.put((size_t)kFeat * B * f);
    w->xh3 = ws.put((size_t)kFeat * B * f);
    w->coef = ws.put((size_t)2 * kFeat * f);
    w->Hc = ws.put((size_t)256 * kFeat * B * f);
    w->hc = ws.put((size_t)kFeat * B * f);
    w->gx2 = ws.put(256 * nb * f);
    w->gx1 = ws.put(64 * nb * f);
    fx3d_status rc;
    if ((rc = fx3d_edgeconv_grad_train_workspace_bytes(kEc1, 4, K, N, B, &w->ec1_bytes)) != FX3D_OK) return rc;
    if ((rc = fx3d_edgeconv_grad_train_workspace_bytes(kEc2, 3, K, N, B, &w->ec2_bytes)) != FX3D_OK) return rc;
    w->scratch = ws.put(w->ec1_bytes > w->ec2_bytes ? w->ec1_bytes : w->ec2_bytes);
    w->total = ws.at;
    return FX3D_OK;
}

}  // namespace

extern "C" {

fx3d_status fx3d_dgcnn_grad_train_workspace_bytes(int32_t N, int32_t B, int32_t K, int32_t num_classes, size_t *bytes) {
    const char *fn = "fx3d_dgcnn_grad_train_workspace_bytes";
    FX3D_REQUIRE(bytes != nullptr, "%s: bytes is NULL", fn);
    fx3d_status rc = dgcnn_check_train_sizes(fn, N, B, K, num_classes);
    if (rc != FX3D_OK) return rc;
    GtWs w;
    if ((rc = gt_ws(N, B, K, &w)) != FX3D_OK) return rc;
    *bytes = w.total;
    return FX3D_OK;
}

fx3d_status fx3d_dgcnn_grad_train(const float *params_dev, int32_t num_classes, int32_t K, const float *x, int32_t N, int32_t B,
                                  const float *dropout4, const float *dropout5, const int32_t *idx1, const float *x1,
                                  const int32_t *idx2, const float *x2, const float *pooled, const float *batch_stats,
                                  const float *glogits, float *gparams, float *gx, float *gx2, float *gx1, void *ws, size_t ws_bytes,
                                  fx3d_stream_t s) {
    const char *fn = "fx3d_dgcnn_grad_train";
    FX3D_REQUIRE(params_dev && x && idx1 && x1 && idx2 && x2 && pooled && batch_stats && glogits && gparams && ws,
                 "%s: params_dev, x, idx1, x1, idx2, x2, pooled, batch_stats, glogits, gparams and ws must not be NULL", fn);
    fx3d_status r = dgcnn_check_train_sizes(fn, N, B, K, num_classes);
    if (r != FX3D_OK) return r;
    GtWs w;
    if ((r = gt_ws(N, B, K, &w)) != FX3D_OK) return r;
    FX3D_REQUIRE(ws_bytes >= w.total, "%s: workspace of %zu bytes, fx3d_dgcnn_grad_train_workspace_bytes says %zu", fn, ws_bytes, w.total);
    FX3D_REQUIRE((reinterpret_cast<uintptr_t>(ws) & 255) == 0, "%s: ws must be 256-byte aligned", fn);
    // the statistics layout (dgcnn_train.hip): ec1.bn1 .. bn3 | ec2.bn1, bn2 | conv3.bn | fc4.bn | fc5.bn, mu (C) then var (C)
    const size_t at2 = (size_t)edgeconv_stat_count(kEc1, 4), at3 = at2 + (size_t)edgeconv_stat_count(kEc2, 3);
    const size_t at4 = at3 + 2 * kFeat, at5 = at4 + 2 * 512;
    Net n = dgcnn_layout(params_dev, num_classes);
    const Net gn = dgcnn_layout(gparams, num_classes);
    n.c3.bn.m = batch_stats + at3; n.c3.bn.v = batch_stats + at3 + kFeat;
    n.bn4.m = batch_stats + at4; n.bn4.v = batch_stats + at4 + 512;
    n.bn5.m = batch_stats + at5; n.bn5.v = batch_stats + at5 + 256;
    hipStream_t st = as_stream(s);
    const pointnet::WsView v{static_cast<char *>(ws)};
    using pointnet::mut;
    float *g2 = gx2 ? gx2 : v.f32(w.gx2), *g1 = gx1 ? gx1 : v.f32(w.gx1);
    float *mb = v.f32(w.coef), *mg = mb + kFeat;
    const int nt = w.ntiles;

    // the point that took the maximum, per tile, with what conv3.bn was given there
    if ((r = launch_tile(&dgcnn_gt_argmax_kernel, "dgcnn_gt_argmax_kernel", "dgcnn_gt_argmax", kConv3Lds, nt, B, kPtThreads, st, x2, n.c3,
                         pooled, v.i32(w.tfirst), v.f32(w.tpre), N, nt)) != FX3D_OK) return r;

    // the head's adjoint, cut at fc5.bn and fc4.bn, down to gy of conv3.bn and that BatchNorm's sums; then the dense layers' sums
    HeadGtArgs hb{};
    hb.tfirst = v.i32(w.tfirst); hb.tpre = v.f32(w.tpre); hb.ntiles = nt; hb.nc = num_classes; hb.pooled = pooled; hb.glogits = glogits;
    hb.c3 = n.c3; hb.d4 = n.d4; hb.d5 = n.d5; hb.d6 = n.d6; hb.bn4 = n.bn4; hb.bn5 = n.bn5;
    hb.drop4 = dropout4; hb.drop5 = dropout5; hb.mb = mb; hb.mg = mg; hb.nstar = v.i32(w.nstar);
    hb.r4 = v.f32(w.r4); hb.in5 = v.f32(w.in5); hb.r5 = v.f32(w.r5); hb.in6 = v.f32(w.in6);
    hb.gy4 = v.f32(w.gy4); hb.xh4 = v.f32(w.xh4); hb.gv4 = v.f32(w.gv4);
    hb.gy5 = v.f32(w.gy5); hb.xh5 = v.f32(w.xh5); hb.gv5 = v.f32(w.gv5);
    hb.gy3 = v.f32(w.gy3); hb.xh3 = v.f32(w.xh3);
    auto bn_out = [&](const Bn &g, long long m) { return BnOut{pointnet::grad_block(g), mb, mg, m}; };
    {
        ProfileScope prof("dgcnn_gt_head", st);
        hipLaunchKernelGGL(dgcnn_gt_head_a_kernel, dim3(B), dim3(kHeadThreads), 0, st, hb);
        FX3D_LAUNCH_CHECK();
        if ((r = pointnet::launch_cloud_sums(hb.gy5, hb.xh5, nullptr, 256, B, bn_out(gn.bn5, B), st)) != FX3D_OK) return r;
        hipLaunchKernelGGL(dgcnn_gt_head_b_kernel, dim3(B), dim3(512), 0, st, hb);
        FX3D_LAUNCH_CHECK();
        if ((r = pointnet::launch_cloud_sums(hb.gy4, hb.xh4, nullptr, 512, B, bn_out(gn.bn4, B), st)) != FX3D_OK) return r;
        hipLaunchKernelGGL(dgcnn_gt_head_c_kernel, dim3(B), dim3(kHeadThreads), 0, st, hb);
        FX3D_LAUNCH_CHECK();
        if ((r = pointnet::launch_cloud_sums(hb.gy3, hb.xh3, hb.nstar, kFeat, B, bn_out(gn.c3.bn, (long long)N * B), st)) != FX3D_OK) return r;
        const DenseSums s4{hb.gv4, pooled, kFeat, 512, B, mut(gn.d4.W), mut(gn.d4.b)}, s5{hb.gv5, hb.in5, 512, 256, B, mut(gn.d5.W), mut(gn.d5.b)},
            s6{glogits, hb.in6, 256, num_classes, B, mut(gn.d6.W), mut(gn.d6.b)};
        for (const DenseSums &q : {s4, s5, s6})
            if ((r = pointnet::launch_dense_sums(q, st)) != FX3D_OK) return r;
    }

    // conv_3: the gradient at x2 (all points), then dW3 and db3 per cloud and their sums over b ascending
    LastArgs ca{};
    ca.in = x2; ca.c3 = n.c3; ca.nstar = hb.nstar; ca.gy3 = hb.gy3; ca.mb = mb; ca.mg = mg; ca.g = g2;
    ca.Hc = v.f32(w.Hc); ca.hc = v.f32(w.hc); ca.N = N; ca.ntiles = nt;
    if ((r = launch_tile(&dgcnn_gt_conv3_bwd_kernel, "dgcnn_gt_conv3_bwd_kernel", "dgcnn_gt_conv3_bwd", kDenseLds, nt, B, kPtThreads, st,
                         ca)) != FX3D_OK) return r;
    if ((r = launch_tile(&dgcnn_gt_conv3_pgrad_kernel, "dgcnn_gt_conv3_pgrad_kernel", "dgcnn_gt_conv3_pgrad", kDenseLds, kFeat / kGroup, B,
                         kPgradThreads, st, ca)) != FX3D_OK) return r;
    {
        ProfileScope prof("dgcnn_gt_reduce", st);
        pointnet::ReduceArgs ra{};
        ra.part = ca.Hc; ra.psize = 256 * kFeat; ra.nparts = B; ra.s[0] = pointnet::Seg{0, mut(gn.c3.W), 256 * kFeat, 0};
        if ((r = pointnet::launch_reduce(ra, 1, st)) != FX3D_OK) return r;
        ra.part = ca.hc; ra.psize = kFeat; ra.s[0] = pointnet::Seg{0, mut(gn.c3.b), kFeat, 0};
        if ((r = pointnet::launch_reduce(ra, 1, st)) != FX3D_OK) return r;
    }

    // the two stages: EdgeConv2 on x1 with gout = gx2, then EdgeConv1 on x with gout = gx1
    char *scratch = static_cast<char *>(ws) + w.scratch;
    if ((r = fx3d_edgeconv_grad_train(n.ec2, kEc2, 3, K, x1, N, B, idx2, x2, batch_stats + at2, g2, mut(gn.ec2), g1, scratch,
                                      w.ec2_bytes, s)) != FX3D_OK) return r;
    return fx3d_edgeconv_grad_train(n.ec1, kEc1, 4, K, x, N, B, idx1, x1, batch_stats, g1, mut(gn.ec1), gx, scratch, w.ec1_bytes, s);
}

}  // extern "C"
