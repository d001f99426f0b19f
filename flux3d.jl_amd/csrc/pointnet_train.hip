// PointNet in training mode (gfx950), the forward: every BatchNorm normalises by the statistics of the current batch, Dropout
// multiplies by a given mask, and the running statistics Flux would leave behind are returned.  include/flux3d_hip.h
// ("PointNet training-mode forward") states the statistics, their orders and the running update; this file is how they are computed.
//
// A Bn holds four pointers and the test-mode kernels read the mean and the variance through bn.m / bn.v, so a layer whose batch
// statistics exist IS the test-mode layer with m / v pointed at the statistics buffer (pointnet_net.h: with_batch_stats).  What is
// new is producing the statistics in dependency order.  Per round (stn, fstn, feat) and BatchNorm L of the round:
//   pointnet_stats_kernel<MODE, L>: the forward's tile (one block = 64 points of one cloud; round_trunk of pointnet_net.h runs
//     the layers below L, whose statistics are known, as the forward does), then layer L's contraction; while its slab is in
//     the accumulators, what the BatchNorm is given (before_bn) is summed per channel over the tile's valid rows in Float64,
//     S1 = sum v and S2 = sum v v, and both are stored with plain stores to sums (2, C, ntiles, B).  Layer L itself goes nowhere else.
//   pointnet_stat_finish_kernel: folds the tile sums of a layer over (tile, cloud) and writes the mean, the variance and the
//     updated running statistics.
//   then the forward's own pointnet_points_kernel<MODE> (launch_points) gives the per-tile maxima (and h in the fstn round).
// The heads are the forward's phases (pointnet_net.h) cut at their BatchNorms, which need all B clouds: head_a (maxima, dense1, relu; stn / fstn: dense2, relu too),
// feat only head_b (BatchNorm, dense2, relu, the dropout multiplier), head_c (BatchNorm, dense3 / cls, relu + softmax), with
// pointnet_dense_stats_kernel in between: one thread per channel sums the (C, B) activations in ascending b.
// No atomics anywhere: every sum has one owner and one order, which depends on (N, B) alone.
// What a statistic is made of -- the Float64 tile sums and their epilogue on the MFMA (TileSum, conv_stat_mfma), the fold, mean,
// variance and running update (fold_tile_sums, finish_channel) -- is in pointnet_net.h; the two finishing kernels below are launched
// through it (launch_stat_finish, launch_dense_stats) by the training-mode forwards of DGCNN and EdgeConv as well.  stnKD(K) as a
// layer of its own (stnkd.hip) is round_trunk's MODE 3 -- MODE 0's layers with the input width at run time -- on the statistics
// kernel and the heads of this file (launch_stats, launch_train_head, declared in pointnet_net.h too).
#include <initializer_list>

#include "pointnet_net.h"

using namespace fx3d;
using namespace fx3d::mlp;
using namespace fx3d::mlp::pointnet;

namespace {

constexpr int kDenseStatThreads = 256;

// layer L = a convolution of 3 input channels (conv3's chain) to 64: waves 0 and 1 are the two chains of a channel
template <int EPI>
__device__ __forceinline__ void conv_stat3(const float *xs, const float *__restrict__ W, const float *__restrict__ bias, int nvalid,
                                           double *__restrict__ sums) {
    __shared__ double other[2][64];
    const int o = threadIdx.x & 63, h = threadIdx.x >> 6;
    TileSum t;
    if (h < 2) {
        const float w0 = W[3 * o], w1 = W[3 * o + 1], w2 = W[3 * o + 2], bi = bias[o];
        for (int q = 0; q < 8; ++q)
            for (int i = 0; i < 4; ++i) {
                const int p = 8 * q + 4 * h + i;
                if (p >= nvalid) continue;
                float acc = 0.0f;
                acc = fmaf(xs[p * 3 + 0], w0, acc);
                acc = fmaf(xs[p * 3 + 1], w1, acc);
                acc = fmaf(xs[p * 3 + 2], w2, acc);
                t.add(before_bn<EPI>(acc, bi));
            }
    }
    if (h == 1) { other[0][o] = t.s1; other[1][o] = t.s2; }
    __syncthreads();
    if (h == 0) store_tile_sum(sums, o, t.s1 + other[0][o], t.s2 + other[1][o]);
}

// BatchNorm L of the round, in the order they run (round_trunk, pointnet_net.h): the layers below L are the forward's own
// calls (h is not written here), layer L's width and epilogue come with it.
template <int MODE, int L>
__global__ __launch_bounds__(kPtThreads) void pointnet_stats_kernel(const StatArgs s) {
    extern __shared__ float lds[];
    const int tile = blockIdx.x, b = blockIdx.y;
    const int p0 = tile * kTile;
    const int nvalid = min(kTile, s.p.N - p0);
    round_trunk<MODE, L, false>(s.p, lds, b, p0, nvalid, [&](const float *in, const Conv &c, auto layer) {
        using Ly = decltype(layer);
        double *sums = s.sums + 2 * ((size_t)b * s.p.ntiles + tile) * Ly::COUT;
        if constexpr (Ly::CIN == 3) conv_stat3<Ly::EPI>(in, c.W, c.b, nvalid, sums);
        else conv_stat_mfma<Ly::CIN, Ly::EPI>(in, Ly::COUT, c.W, c.b, nvalid, sums, Ly::CIN == 0 ? s.p.K : Ly::CIN);
    });
}

// the fold of a layer's tile sums (fold_tile_sums, pointnet_net.h), then the mean, the variance and the running statistics
__global__ __launch_bounds__(kFinishThreads) void pointnet_stat_finish_kernel(const double *__restrict__ sums, int C, long long T,
                                                                            const StatOut o) {
    fold_tile_sums(sums, C, T, [&](int c, double s1, double s2) { finish_channel(o, c, s1, s2); });
}

// a dense BatchNorm: thread c sums channel c of act (C, B) over the clouds in ascending b from +0.0, and finishes it
__global__ __launch_bounds__(kDenseStatThreads) void pointnet_dense_stats_kernel(const float *__restrict__ act, int C, int B,
                                                                               const StatOut o) {
    const int c = blockIdx.x * kDenseStatThreads + threadIdx.x;  // C is a multiple of 256
    TileSum t;
#pragma unroll 8
    for (int b = 0; b < B; ++b) t.add(act[(size_t)b * C + c]);
    finish_channel(o, c, t.s1, t.s2);
}

// up to the head's first BatchNorm: MaxPool, relu(dense1); stn / fstn have no BatchNorm there and go on through relu(dense2)
template <bool FEAT>
__global__ __launch_bounds__(kHeadThreads) void pointnet_train_head_a_kernel(const TrainHeadArgs t) {
    const HeadArgs &a = t.h;
    __shared__ float v0[kFeat], v1[512];
    const int b = blockIdx.x, tid = threadIdx.x;
    head_pool<FEAT>(a, b, v0);
    __syncthreads();
    if (tid < 512) {
        const float v = head_relu_dense<512>(a.d1, v0);
        if (FEAT) t.a1[(size_t)b * 512 + tid] = v;
        else v1[tid] = v;
    }
    if (FEAT) return;
    __syncthreads();
    if (tid < 256) t.a2[(size_t)b * 256 + tid] = head_relu_dense<256>(a.d2, v1);
}

// feat: BatchNorm(512) at the batch statistics, relu(dense2), the dropout multiplier
__global__ __launch_bounds__(512) void pointnet_train_head_b_kernel(const TrainHeadArgs t) {
    const HeadArgs &a = t.h;
    __shared__ float v1[512];
    const int b = blockIdx.x, tid = threadIdx.x;
    v1[tid] = head_bn(a.bn1, t.a1[(size_t)b * 512 + tid]);
    __syncthreads();
    if (tid < 256) {
        float v = head_relu_dense<256>(a.d2, v1);
        if (t.dropout) v = v * t.dropout[(size_t)b * 256 + tid];
        t.a2[(size_t)b * 256 + tid] = v;
    }
}

// BatchNorm(256) at the batch statistics, then the head's end
template <bool FEAT>
__global__ __launch_bounds__(kHeadThreads) void pointnet_train_head_c_kernel(const TrainHeadArgs t) {
    const HeadArgs &a = t.h;
    __shared__ float v2[256];
    const int b = blockIdx.x, tid = threadIdx.x;
    if (tid < 256) v2[tid] = head_bn(a.bn2, t.a2[(size_t)b * 256 + tid]);
    __syncthreads();
    head_finish<FEAT>(a, b, v2);
}

template <int MODE, int L>
fx3d_status launch_stats_of(const StatArgs &s, int B, bool last, hipStream_t st) {
    const fx3d_status rc = ensure_dynamic_lds(reinterpret_cast<const void *>(&pointnet_stats_kernel<MODE, L>), (int)kPtLds,
                                              "pointnet_stats_kernel");
    if (rc != FX3D_OK) return rc;
    ProfileScope prof(last ? "pointnet_train_stats_last" : "pointnet_train_stats", st);
    hipLaunchKernelGGL((pointnet_stats_kernel<MODE, L>), dim3(s.p.ntiles, B), dim3(kPtThreads), kPtLds, st, s);
    FX3D_LAUNCH_CHECK();
    return FX3D_OK;
}

// the forward's workspace, then the tile sums of the widest layer, relu(dense1) of feat and relu(dense2) of every head
struct TrainPlan { WsPlan fwd; size_t sums, a1, a2, total; };
TrainPlan train_plan(int N, int B, int nc) {
    TrainPlan t;
    t.fwd = ws_plan(N, B, nc);
    WsBump ws;
    ws.at = t.fwd.total;
    t.sums = ws.put((size_t)2 * kFeat * t.fwd.ntiles * B * sizeof(double));
    t.a1 = ws.put((size_t)512 * B * sizeof(float));
    t.a2 = ws.put((size_t)256 * B * sizeof(float));
    t.total = ws.at;
    return t;
}

fx3d_status check_train_sizes(const char *fn, int32_t N, int32_t B, int32_t nc) {
    const fx3d_status rc = check_sizes(fn, N, B, nc);
    if (rc != FX3D_OK) return rc;
    FX3D_REQUIRE(B >= 2, "%s: training-mode BatchNorm needs B >= 2 clouds (a Dense BatchNorm's running variance divides by B - 1), got %d",
                 fn, B);
    return FX3D_OK;
}

}  // namespace

// ---- what the training-mode forwards share (pointnet_net.h): the statistics pass and the heads (stnkd.hip), the finishing kernels
namespace fx3d {
namespace mlp {
namespace pointnet {

// BatchNorm L of round `mode`; `last`: the round's 1024-channel layer (a label of its own in the library's profile)
fx3d_status launch_stats(int mode, int L, const StatArgs &s, int B, hipStream_t st) {
    switch (mode * 4 + L) {
        case 0: return launch_stats_of<0, 0>(s, B, false, st);
        case 1: return launch_stats_of<0, 1>(s, B, false, st);
        case 2: return launch_stats_of<0, 2>(s, B, true, st);
        case 4: return launch_stats_of<1, 0>(s, B, false, st);
        case 5: return launch_stats_of<1, 1>(s, B, false, st);
        case 6: return launch_stats_of<1, 2>(s, B, false, st);
        case 7: return launch_stats_of<1, 3>(s, B, true, st);
        case 8: return launch_stats_of<2, 0>(s, B, false, st);
        case 9: return launch_stats_of<2, 1>(s, B, true, st);
        case 12: return launch_stats_of<3, 0>(s, B, false, st);
        case 13: return launch_stats_of<3, 1>(s, B, false, st);
        default: return launch_stats_of<3, 2>(s, B, true, st);
    }
}

// part 0 = head_a, 1 = head_b (feat), 2 = head_c
fx3d_status launch_train_head(int part, bool feat, const TrainHeadArgs &t, int B, hipStream_t st) {
    ProfileScope prof("pointnet_train_head", st);
    if (part == 0) {
        if (feat) hipLaunchKernelGGL(pointnet_train_head_a_kernel<true>, dim3(B), dim3(kHeadThreads), 0, st, t);
        else hipLaunchKernelGGL(pointnet_train_head_a_kernel<false>, dim3(B), dim3(kHeadThreads), 0, st, t);
    } else if (part == 1) {
        hipLaunchKernelGGL(pointnet_train_head_b_kernel, dim3(B), dim3(512), 0, st, t);
    } else {
        if (feat) hipLaunchKernelGGL(pointnet_train_head_c_kernel<true>, dim3(B), dim3(kHeadThreads), 0, st, t);
        else hipLaunchKernelGGL(pointnet_train_head_c_kernel<false>, dim3(B), dim3(kHeadThreads), 0, st, t);
    }
    FX3D_LAUNCH_CHECK();
    return FX3D_OK;
}

fx3d_status launch_stat_finish(const double *sums, int C, long long T, const StatOut &o, hipStream_t st, const char *label) {
    ProfileScope prof(label, st);
    hipLaunchKernelGGL(pointnet_stat_finish_kernel, dim3((C + kFinishChannels - 1) / kFinishChannels), dim3(kFinishThreads), 0, st,
                       sums, C, T, o);
    FX3D_LAUNCH_CHECK();
    return FX3D_OK;
}

fx3d_status launch_dense_stats(const float *act, int C, int B, const StatOut &o, hipStream_t st, const char *label) {
    ProfileScope prof(label, st);
    hipLaunchKernelGGL(pointnet_dense_stats_kernel, dim3(C / kDenseStatThreads), dim3(kDenseStatThreads), 0, st, act, C, B, o);
    FX3D_LAUNCH_CHECK();
    return FX3D_OK;
}

}  // namespace pointnet
}  // namespace mlp
}  // namespace fx3d

extern "C" {

fx3d_status fx3d_pointnet_stat_count(int64_t *count) {
    FX3D_REQUIRE(count != nullptr, "fx3d_pointnet_stat_count: count is NULL");
    *count = 2 * kStatChannels;
    return FX3D_OK;
}

fx3d_status fx3d_pointnet_train_workspace_bytes(int32_t N, int32_t B, int32_t num_classes, size_t *bytes) {
    FX3D_REQUIRE(bytes != nullptr, "fx3d_pointnet_train_workspace_bytes: bytes is NULL");
    const fx3d_status rc = check_train_sizes("fx3d_pointnet_train_workspace_bytes", N, B, num_classes);
    if (rc != FX3D_OK) return rc;
    *bytes = train_plan(N, B, num_classes).total;
    return FX3D_OK;
}

fx3d_status fx3d_pointnet_forward_train(const float *params_dev, int32_t num_classes, const float *x, int32_t N, int32_t B,
                                        const float *dropout, float momentum, float *probs, float *logits, float *stn, float *fstn,
                                        float *pooled, float *batch_stats, float *running, void *ws, size_t ws_bytes,
                                        fx3d_stream_t s) {
    const char *fn = "fx3d_pointnet_forward_train";
    FX3D_REQUIRE(params_dev && x && probs && batch_stats && ws, "%s: params_dev, x, probs, batch_stats and ws must not be NULL", fn);
    const fx3d_status rc = check_train_sizes(fn, N, B, num_classes);
    if (rc != FX3D_OK) return rc;
    FX3D_REQUIRE(std::isfinite(momentum) && momentum >= 0.0f && momentum <= 1.0f, "%s: momentum must be finite and in [0, 1], got %g",
                 fn, (double)momentum);
    const TrainPlan tp = train_plan(N, B, num_classes);
    const WsPlan &w = tp.fwd;
    FX3D_REQUIRE(ws_bytes >= tp.total, "%s: workspace of %zu bytes, fx3d_pointnet_train_workspace_bytes says %zu", fn, ws_bytes,
                 tp.total);
    FX3D_REQUIRE((reinterpret_cast<uintptr_t>(ws) & 15) == 0, "%s: ws must be 16-byte aligned", fn);
    const Net run = layout(params_dev, num_classes);  // the running statistics, read for `running` alone
    const Net n = with_batch_stats(run, batch_stats);
    // the 13 BatchNorms in forward order, which is the order they run in: their slots of the statistics buffers, their running
    // values and their widths
    StatOut so[kNumBn];
    int width[kNumBn];
    {
        int i = 0;
        size_t at = 0;
        for_each_bn(run, [&](const Bn &bn, int C) {
            so[i].run_m = bn.m; so[i].run_v = bn.v;
            so[i].mu = batch_stats + at; so[i].var = batch_stats + at + C;
            so[i].new_m = running ? running + at : nullptr; so[i].new_v = running ? running + at + C : nullptr;
            so[i].mtm = momentum;
            so[i].m = (long long)N * B;
            width[i] = C;
            at += 2 * (size_t)C;
            ++i;
        });
        for (int k : {3, 8, 11, 12}) so[k].m = B;  // the BatchNorms after a dense layer
    }
    hipStream_t st = as_stream(s);
    const WsView v{static_cast<char *>(ws)};
    float *tmax = v.f32(w.tmax), *T = v.f32(w.T), *F = v.f32(w.F);
    const long long ntl = (long long)w.ntiles * B;

    StatArgs sa{};
    PointArgs &p = sa.p;
    sa.sums = v.f64(tp.sums);
    p.x = x; p.h = v.f32(w.h); p.tmax = tmax; p.N = N; p.ntiles = w.ntiles;
    TrainHeadArgs t{};
    t.a1 = v.f32(tp.a1); t.a2 = v.f32(tp.a2); t.dropout = dropout;
    fx3d_status r;
    int slot = 0;
    // stn: T (3, 3) of every cloud; x T, conv_block1, fstn: F (64, 64); h F, feat, cls, softmax
    for (int mode = 0; mode < 3; ++mode) {
        const bool feat = mode == 2;
        set_round(p, n, mode, T, F);
        // the round's point BatchNorms in order, then the round's closing full pass (which keeps conv_block1 as h)
        for (int L = 0; L <= kLastLayer[mode]; ++L, ++slot) {
            if ((r = launch_stats(mode, L, sa, B, st)) != FX3D_OK) return r;
            if ((r = launch_stat_finish(sa.sums, width[slot], ntl, so[slot], st, "pointnet_train_finish")) != FX3D_OK) return r;
        }
        if ((r = launch_points(mode, false, p, B, st)) != FX3D_OK) return r;
        // the head: relu(dense1) and for feat its BatchNorm's statistics, relu(dense2) and its BatchNorm's statistics, the end
        t.h = feat ? feat_head(n, num_classes, tmax, w.ntiles, pooled, logits ? logits : v.f32(w.logits), probs)
                   : stn_head(n, mode, tmax, w.ntiles, T, F, mode == 0 ? stn : fstn);
        if ((r = launch_train_head(0, feat, t, B, st)) != FX3D_OK) return r;
        if (feat) {
            if ((r = launch_dense_stats(t.a1, width[slot], B, so[slot], st, "pointnet_train_dense_stats")) != FX3D_OK) return r;
            if ((r = launch_train_head(1, true, t, B, st)) != FX3D_OK) return r;
            ++slot;
        }
        if ((r = launch_dense_stats(t.a2, width[slot], B, so[slot], st, "pointnet_train_dense_stats")) != FX3D_OK) return r;
        if ((r = launch_train_head(2, feat, t, B, st)) != FX3D_OK) return r;
        ++slot;
    }
    return FX3D_OK;
}

}  // extern "C"
