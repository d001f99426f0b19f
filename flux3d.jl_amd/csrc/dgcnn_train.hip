// DGCNN in training mode (gfx950), the forward: all 8 BatchNorms normalise by the statistics of the current batch, the two
// Dropout(0.5) multiply by given masks, and the running statistics Flux would leave behind are returned.  include/flux3d_hip.h
// ("DGCNN / EdgeConv training-mode forward") states the statistics, their orders and the running update; this file is how they
// are computed.
//
// Per forward, in dependency order:
//   the two EdgeConv stages through edgeconv_train_run (edgeconv_train.hip) on the ec1 / ec2 slices of the parameters and of
//     the statistics: per BatchNorm a statistics pass and the finishing kernel, then the unchanged edgeconv_kernel.  EdgeConv2's
//     neighbour search runs on the training-mode x1.
//   conv_3: dgcnn_conv3_stats_kernel -- the forward's tile of x2 (load_x2_tile), its slabs (for_each_slab) with PointNet's
//     statistics epilogue (conv_stat_mfma, pointnet_net.h) -- and the finishing kernel; then the forward's dgcnn_conv3_kernel at
//     the statistics (launch_conv3).
//   the head, dgcnn_head_kernel's phases cut at its two BatchNorms, which need all B clouds: head_a (maxima, fc_4's dense),
//     head_b (BatchNorm, relu, the dropout multiplier, fc_5's dense), head_c (BatchNorm, relu, the multiplier, fc_6, softmax), with
//     PointNet's pointnet_dense_stats_kernel in between (launch_dense_stats) on the (512, B) and (256, B) activations.
// One stream, no host synchronisation, no atomics: every sum has one owner and one order.
#include "dgcnn_net.h"
#include "edgeconv_net.h"
#include "pointnet_net.h"

using namespace fx3d;
using namespace fx3d::mlp;
using fx3d::mlp::pointnet::StatOut;

namespace {

constexpr int kStatChannels = 32 + 64 + 64 + 128 + 256 + kFeat + 512 + 256;  // 2336

// conv_3's statistics pass: sums (2, 1024, ntiles, B), the tile sums of conv + bias in PointNet's order
__global__ __launch_bounds__(kPtThreads) void dgcnn_conv3_stats_kernel(const float *__restrict__ x2, const Conv c, double *__restrict__ sums,
                                                                       int N, int ntiles) {
    extern __shared__ float lds[];
    const int tile = blockIdx.x, b = blockIdx.y;
    const int p0 = tile * kTile;
    const int nvalid = min(kTile, N - p0);
    load_x2_tile(lds, x2, b, N, p0, nvalid);
    __syncthreads();
    pointnet::conv_stat_mfma<256, kBnOnly, kLd3>(lds, kFeat, c.W, c.b, nvalid, sums + 2 * ((size_t)b * ntiles + tile) * kFeat);
}

struct TrainHeadArgs {
    const float *tmax;  // (1024, ntiles, B)
    int ntiles;
    Dense d4, d5, d6;
    Bn bn4, bn5;        // at the batch statistics
    int nc;
    const float *drop4, *drop5;  // (512, B), (256, B) multipliers or NULL
    float *a4, *a5;              // workspace: fc_4's dense + bias (512, B), fc_5's (256, B): what the two BatchNorms are given
    float *pooled;               // optional: (1024, B)
    float *logits, *probs;
};

// MaxPool over the cloud's points, fc_4's dense layer
__global__ __launch_bounds__(kHeadThreads) void dgcnn_train_head_a_kernel(const TrainHeadArgs a) {
    __shared__ float v0[kFeat];
    const int b = blockIdx.x, tid = threadIdx.x;
    const float m = fold_tile_maxima(a.tmax, a.ntiles, b);
    v0[tid] = m;
    if (a.pooled) a.pooled[(size_t)b * kFeat + tid] = m;
    __syncthreads();
    if (tid < 512) a.a4[(size_t)b * 512 + tid] = dense_chain(v0, kFeat, a.d4.W, 512, tid) + a.d4.b[tid];
}

// fc_4's BatchNorm at the batch statistics, relu, the dropout multiplier; fc_5's dense layer
__global__ __launch_bounds__(512) void dgcnn_train_head_b_kernel(const TrainHeadArgs a) {
    __shared__ float v1[512];
    const int b = blockIdx.x, tid = threadIdx.x;
    float v = head_bn_relu(a.bn4, a.a4[(size_t)b * 512 + tid]);
    if (a.drop4) v = v * a.drop4[(size_t)b * 512 + tid];
    v1[tid] = v;
    __syncthreads();
    if (tid < 256) a.a5[(size_t)b * 256 + tid] = dense_chain(v1, 512, a.d5.W, 256, tid) + a.d5.b[tid];
}

// fc_5's BatchNorm at the batch statistics, relu, the dropout multiplier; fc_6 and the softmax
__global__ __launch_bounds__(kHeadThreads) void dgcnn_train_head_c_kernel(const TrainHeadArgs a) {
    __shared__ float v2[256];
    const int b = blockIdx.x, tid = threadIdx.x;
    if (tid < 256) {
        float v = head_bn_relu(a.bn5, a.a5[(size_t)b * 256 + tid]);
        if (a.drop5) v = v * a.drop5[(size_t)b * 256 + tid];
        v2[tid] = v;
    }
    __syncthreads();
    float *z = a.logits + (size_t)b * a.nc, *pr = a.probs + (size_t)b * a.nc;
    for (int o = tid; o < a.nc; o += kHeadThreads) z[o] = dense_chain(v2, 256, a.d6.W, a.nc, o) + a.d6.b[o];
    softmax_of_logits(z, pr, a.nc);
}

// the forward's workspace | the tile sums of the widest layer, conv_3's (2, 1024, ntiles, B) Float64 | fc_4's and fc_5's dense
// outputs (512, B), (256, B)
struct TrainPlan { DgcnnWsPlan fwd; size_t sums, a4, a5, total; };
fx3d_status train_plan(int N, int B, int K, int nc, TrainPlan *t) {
    const fx3d_status rc = dgcnn_ws_plan(N, B, K, nc, &t->fwd);
    if (rc != FX3D_OK) return rc;
    WsBump ws;
    ws.at = t->fwd.total;
    t->sums = ws.put((size_t)2 * kFeat * t->fwd.ntiles * B * sizeof(double));  // (an EdgeConv stage's are smaller: 256 channels at most)
    t->a4 = ws.put((size_t)512 * B * sizeof(float));
    t->a5 = ws.put((size_t)256 * B * sizeof(float));
    t->total = ws.at;
    return FX3D_OK;
}

// one BatchNorm's slot of the statistics buffers, `at` floats in, and the running values it updates
StatOut stat_out(const Bn &run, int C, size_t at, float *batch_stats, float *running, float momentum, long long m) {
    StatOut o{};
    o.run_m = run.m; o.run_v = run.v;
    o.mu = batch_stats + at; o.var = batch_stats + at + C;
    o.new_m = running ? running + at : nullptr; o.new_v = running ? running + at + C : nullptr;
    o.mtm = momentum;
    o.m = m;
    return o;
}

}  // namespace

extern "C" {

fx3d_status fx3d_dgcnn_stat_count(int64_t *count) {
    FX3D_REQUIRE(count != nullptr, "fx3d_dgcnn_stat_count: count is NULL");
    *count = 2 * kStatChannels;
    return FX3D_OK;
}

fx3d_status fx3d_dgcnn_train_workspace_bytes(int32_t N, int32_t B, int32_t K, int32_t num_classes, size_t *bytes) {
    const char *fn = "fx3d_dgcnn_train_workspace_bytes";
    FX3D_REQUIRE(bytes != nullptr, "%s: bytes is NULL", fn);
    fx3d_status rc = dgcnn_check_train_sizes(fn, N, B, K, num_classes);
    if (rc != FX3D_OK) return rc;
    TrainPlan t;
    if ((rc = train_plan(N, B, K, num_classes, &t)) != FX3D_OK) return rc;
    *bytes = t.total;
    return FX3D_OK;
}

fx3d_status fx3d_dgcnn_forward_train(const float *params_dev, int32_t num_classes, int32_t K, const float *x, int32_t N, int32_t B,
                                     const float *dropout4, const float *dropout5, float momentum, float *probs, float *logits,
                                     int32_t *idx1, float *x1, int32_t *idx2, float *x2, float *pooled, float *batch_stats,
                                     float *running, void *ws, size_t ws_bytes, fx3d_stream_t s) {
    const char *fn = "fx3d_dgcnn_forward_train";
    FX3D_REQUIRE(params_dev && x && probs && batch_stats && ws, "%s: params_dev, x, probs, batch_stats and ws must not be NULL", fn);
    fx3d_status r = dgcnn_check_train_sizes(fn, N, B, K, num_classes);
    if (r != FX3D_OK) return r;
    FX3D_REQUIRE(std::isfinite(momentum) && momentum >= 0.0f && momentum <= 1.0f, "%s: momentum must be finite and in [0, 1], got %g",
                 fn, (double)momentum);
    TrainPlan t;
    if ((r = train_plan(N, B, K, num_classes, &t)) != FX3D_OK) return r;
    const DgcnnWsPlan &w = t.fwd;
    FX3D_REQUIRE(ws_bytes >= t.total, "%s: workspace of %zu bytes, fx3d_dgcnn_train_workspace_bytes says %zu", fn, ws_bytes, t.total);
    FX3D_REQUIRE((reinterpret_cast<uintptr_t>(ws) & 255) == 0, "%s: ws must be 256-byte aligned", fn);
    FX3D_REQUIRE(!x1 || (reinterpret_cast<uintptr_t>(x1) & 15) == 0, "%s: x1 must be 16-byte aligned", fn);
    const Net run = dgcnn_layout(params_dev, num_classes);  // its mu / var: the running statistics, read for `running` alone
    hipStream_t st = as_stream(s);
    char *wsb = static_cast<char *>(ws);
    float *f1 = x1 ? x1 : reinterpret_cast<float *>(wsb + w.x1), *f2 = x2 ? x2 : reinterpret_cast<float *>(wsb + w.x2);
    float *tmax = reinterpret_cast<float *>(wsb + w.tmax);
    float *lg = logits ? logits : reinterpret_cast<float *>(wsb + w.logits);
    double *sums = reinterpret_cast<double *>(wsb + t.sums);

    // the statistics layout: ec1.bn1 .. bn3 | ec2.bn1, bn2 | conv3.bn | fc4.bn | fc5.bn, per BatchNorm mu (C), then var (C)
    const size_t at2 = (size_t)edgeconv_stat_count(kEc1, 4), at3 = at2 + (size_t)edgeconv_stat_count(kEc2, 3);
    const size_t at4 = at3 + 2 * kFeat, at5 = at4 + 2 * 512;
    const EdgeTrainLabels l1{"dgcnn_train_ec1_stats", "dgcnn_train_ec1_stats_last", "dgcnn_train_finish", "dgcnn_train_ec1_closing"};
    const EdgeTrainLabels l2{"dgcnn_train_ec2_stats", "dgcnn_train_ec2_stats_last", "dgcnn_train_finish", "dgcnn_train_ec2_closing"};
    if ((r = edgeconv_train_run(run.ec1, kEc1, 4, K, x, N, B, nullptr, momentum, f1, idx1, batch_stats, running, wsb + w.ec, sums, s,
                                l1)) != FX3D_OK) return r;
    if ((r = edgeconv_train_run(run.ec2, kEc2, 3, K, f1, N, B, nullptr, momentum, f2, idx2, batch_stats + at2,
                                running ? running + at2 : nullptr, wsb + w.ec, sums, s, l2)) != FX3D_OK) return r;

    // conv_3: its statistics, then the forward's maxima kernel at them
    if ((r = ensure_dynamic_lds(reinterpret_cast<const void *>(&dgcnn_conv3_stats_kernel), (int)kConv3Lds, "dgcnn_conv3_stats_kernel")) != FX3D_OK) return r;
    {
        ProfileScope prof("dgcnn_train_conv3_stats", st);
        hipLaunchKernelGGL(dgcnn_conv3_stats_kernel, dim3(w.ntiles, B), dim3(kPtThreads), kConv3Lds, st, f2, run.c3, sums, N, w.ntiles);
        FX3D_LAUNCH_CHECK();
    }
    if ((r = pointnet::launch_stat_finish(sums, kFeat, (long long)w.ntiles * B,
                                          stat_out(run.c3.bn, kFeat, at3, batch_stats, running, momentum, (long long)N * B), st,
                                          "dgcnn_train_finish")) != FX3D_OK) return r;
    Conv c3 = run.c3;
    c3.bn.m = batch_stats + at3; c3.bn.v = batch_stats + at3 + kFeat;
    if ((r = launch_conv3(f2, c3, tmax, N, w.ntiles, B, st, "dgcnn_train_conv3_closing")) != FX3D_OK) return r;

    // the head, cut at its two BatchNorms
    TrainHeadArgs hd{};
    hd.tmax = tmax; hd.ntiles = w.ntiles;
    hd.d4 = run.d4; hd.d5 = run.d5; hd.d6 = run.d6;
    hd.bn4 = run.bn4; hd.bn4.m = batch_stats + at4; hd.bn4.v = batch_stats + at4 + 512;
    hd.bn5 = run.bn5; hd.bn5.m = batch_stats + at5; hd.bn5.v = batch_stats + at5 + 256;
    hd.nc = num_classes; hd.drop4 = dropout4; hd.drop5 = dropout5;
    hd.a4 = reinterpret_cast<float *>(wsb + t.a4); hd.a5 = reinterpret_cast<float *>(wsb + t.a5);
    hd.pooled = pooled; hd.logits = lg; hd.probs = probs;
    {
        ProfileScope prof("dgcnn_train_head", st);
        hipLaunchKernelGGL(dgcnn_train_head_a_kernel, dim3(B), dim3(kHeadThreads), 0, st, hd);
        FX3D_LAUNCH_CHECK();
    }
    if ((r = pointnet::launch_dense_stats(hd.a4, 512, B, stat_out(run.bn4, 512, at4, batch_stats, running, momentum, B), st,
                                          "dgcnn_train_dense_stats")) != FX3D_OK) return r;
    {
        ProfileScope prof("dgcnn_train_head", st);
        hipLaunchKernelGGL(dgcnn_train_head_b_kernel, dim3(B), dim3(512), 0, st, hd);
        FX3D_LAUNCH_CHECK();
    }
    if ((r = pointnet::launch_dense_stats(hd.a5, 256, B, stat_out(run.bn5, 256, at5, batch_stats, running, momentum, B), st,
                                          "dgcnn_train_dense_stats")) != FX3D_OK) return r;
    ProfileScope prof("dgcnn_train_head", st);
    hipLaunchKernelGGL(dgcnn_train_head_c_kernel, dim3(B), dim3(kHeadThreads), 0, st, hd);
    FX3D_LAUNCH_CHECK();
    return FX3D_OK;
}

}  // extern "C"
