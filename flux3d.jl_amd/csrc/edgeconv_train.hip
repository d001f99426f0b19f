// EdgeConv(layers, K) in training mode (gfx950), the forward: every BatchNorm normalises by the statistics of the current batch,
// m = K N B edge rows per channel, and the running statistics Flux would leave behind are returned.  include/flux3d_hip.h
// ("DGCNN / EdgeConv training-mode forward") states the statistics, their order and the running update; this file is how they
// are computed.  Both EdgeConv stages of fx3d_dgcnn_forward_train (dgcnn_train.hip) go through edgeconv_train_run below.
//
// The (K N, C, B) activation a BatchNorm is given is never written: its sums are taken where the forward's tile lives.  Per layer
// l = 1 .. L, in dependency order:
//   edgeconv_stats_kernel<LD>: the forward's kernel on the layer cut after block l (edge_pass of the first l blocks, whose
//     BatchNorms 1 .. l - 1 read the statistics buffer: they are finished): one block = 64 points of one cloud, the loop over k of
//     edge_trunk (edgeconv_net.h) -- the gather and the layers below l are the forward's own calls.  Layer l's slabs are computed as
//     the forward computes its last layer (mfma_slab_rt, the same lanes, the same split_halves), and while a slab is in the
//     accumulators acc + bias is added into Float64 (S1, S2) pairs the lane carries across k: one pair per 32-point half of a
//     slab, 8 VGPRs per slab in place of the forward's 32 of running maxima.  Rows beyond the cloud's last point add +0.0 (which
//     changes no bit of a chain that began at +0.0); lanes beyond a partial slab store nothing.  After the last k the two half-waves
//     meet through __shfl_xor, the two halves in the lane (or, split_halves, through LDS), and the tile's pair is stored with
//     plain stores to sums (2, C, ntiles, B).
//   pointnet_stat_finish_kernel (pointnet_net.h: launch_stat_finish): the fold over (tile, cloud) in 32 interleaved chains, the
//     mean, the variance and the running statistics.
// Then the unchanged edgeconv_kernel with every BatchNorm at the statistics.  No atomics: every sum has one owner and one order.
#include "edgeconv_net.h"
#include "pointnet_net.h"

using namespace fx3d;
using namespace fx3d::mlp;
using fx3d::mlp::pointnet::StatOut;
using fx3d::mlp::pointnet::TileSum;

namespace {

// the 16 rows of one 32-point half a lane holds of a slab, rows p0 + mfma_row(r, h), into the half's chain: v = acc + bias is
// what the BatchNorm is given; a row beyond the cloud's last point adds +0.0
__device__ __forceinline__ void add_half(TileSum &t, const f32x16 &acc, float bias, int first, int h, int nvalid) {
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const float v = acc[r] + bias;
        t.add(first + mfma_row(r, h) < nvalid ? v : 0.0f);
    }
}

// Layer l for the current k into the lane's chains.  A wave owns what it owns of the forward's last layer (conv_rt_fold): the
// slabs wave, wave + 4 for both halves -- ts[s][0], ts[s][1] -- or, split_halves, one half of one slab -- ts[0][0].
template <int LD>
__device__ __forceinline__ void conv_rt_stats(const float *in, int cin, int cout, const Conv &c, int nvalid, TileSum (&ts)[2][2]) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, h = lane >> 5, j = lane & 31;
    if (split_halves(cout)) {
        if ((wave >> 1) * 32 >= cout) return;
        const int oc = min((wave >> 1) * 32 + j, cout - 1);  // (a lane beyond a partial slab sums the last channel; never stored)
        f32x16 acc[1] = {f32x16{0}};
        mfma_slab_rt<LD, 1>(in + (wave & 1) * 32 * LD, c.W + (size_t)cin * oc, cin, h, j, acc);
        add_half(ts[0][0], acc[0], c.b[oc], (wave & 1) * 32, h, nvalid);
        return;
    }
#pragma unroll
    for (int s = 0; s < 2; ++s) {
        const int sl = wave + s * (kPtThreads / 64);
        if (sl * 32 >= cout) break;  // wave-uniform
        const int oc = min(sl * 32 + j, cout - 1);
        f32x16 acc[2] = {f32x16{0}, f32x16{0}};
        mfma_slab_rt<LD, 2>(in, c.W + (size_t)cin * oc, cin, h, j, acc);
        const float bi = c.b[oc];
        add_half(ts[s][0], acc[0], bi, 0, h, nvalid);
        add_half(ts[s][1], acc[1], bi, 32, h, nvalid);
    }
}

// a half's two chains meet: own + other, which is chain(0) + chain(1) in the half-wave h = 0 that stores it
__device__ __forceinline__ TileSum meet_half_waves(const TileSum &t) {
    TileSum r;
    r.s1 = t.s1 + __shfl_xor(t.s1, 32, 64);
    r.s2 = t.s2 + __shfl_xor(t.s2, 32, 64);
    return r;
}

// a: the pass cut at the layer whose statistics are wanted (a.nl = l, a.cout = its width); sums: (2, a.cout, ntiles, B)
template <int LD>
__global__ __launch_bounds__(kPtThreads) void edgeconv_stats_kernel(const EdgeConvArgs a, double *__restrict__ sums) {
    extern __shared__ float lds[];
    const int tile = blockIdx.x, b = blockIdx.y;
    const int p0 = tile * kTile;
    const int nvalid = min(kTile, a.N - p0);
    const int cout = a.cout;
    TileSum ts[2][2];
    edge_trunk<LD>(a, lds, b, p0, nvalid,
                   [&](const float *src, int cin, int co, const Conv &c) { conv_rt_stats<LD>(src, cin, co, c, nvalid, ts); });
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, h = lane >> 5, j = lane & 31;
    double *out = sums + 2 * ((size_t)b * gridDim.x + tile) * cout;
    if (split_halves(cout)) {
        // the wave's half: chain(0) + chain(1); the two halves of a slab are on the waves 2 s and 2 s + 1 and meet in LDS, which
        // no wave reads any more once all have left the loop over k
        double *other = reinterpret_cast<double *>(lds);  // [2][64]
        const TileSum t = meet_half_waves(ts[0][0]);
        __syncthreads();
        if ((wave & 1) && h == 0) {
            other[(wave >> 1) * 32 + j] = t.s1;
            other[64 + (wave >> 1) * 32 + j] = t.s2;
        }
        __syncthreads();
        const int o = (wave >> 1) * 32 + j;
        if (!(wave & 1) && h == 0 && o < cout) pointnet::store_tile_sum(out, o, t.s1 + other[o], t.s2 + other[64 + o]);
        return;
    }
#pragma unroll
    for (int s = 0; s < 2; ++s) {
        const int o = (wave + s * (kPtThreads / 64)) * 32 + j;
        if (o - j >= cout) break;  // wave-uniform
        const TileSum t0 = meet_half_waves(ts[s][0]), t1 = meet_half_waves(ts[s][1]);
        if (h == 0 && o < cout) pointnet::store_tile_sum(out, o, t0.s1 + t1.s1, t0.s2 + t1.s2);
    }
}

template <int LD>
fx3d_status launch_stats_of(const EdgePass &p, double *sums, int B, hipStream_t st, const char *label) {
    const fx3d_status rc = ensure_dynamic_lds(reinterpret_cast<const void *>(&edgeconv_stats_kernel<LD>), (int)kMaxLds, "edgeconv_stats_kernel");
    if (rc != FX3D_OK) return rc;
    ProfileScope prof(label, st);
    hipLaunchKernelGGL((edgeconv_stats_kernel<LD>), dim3((p.a.N + kTile - 1) / kTile, B), dim3(kPtThreads), p.lds_bytes, st, p.a, sums);
    FX3D_LAUNCH_CHECK();
    return FX3D_OK;
}

fx3d_status launch_stats(const EdgePass &p, double *sums, int B, hipStream_t st, const char *label) {
    switch (p.ld) {
        case 66: return launch_stats_of<66>(p, sums, B, st, label);
        case kLd: return launch_stats_of<kLd>(p, sums, B, st, label);
        default: return launch_stats_of<258>(p, sums, B, st, label);
    }
}

// the forward's workspace | the tile sums of the widest layer, (2, C, ntiles, B) Float64
struct TrainPlan { size_t fwd, sums, total; };
fx3d_status train_plan(const int32_t *layers, int nlayers, int N, int B, int K, TrainPlan *t) {
    const fx3d_status rc = edgeconv_workspace_bytes(layers[0], N, B, K, &t->fwd);
    if (rc != FX3D_OK) return rc;
    WsBump ws;
    ws.at = t->fwd;
    t->sums = ws.put(edgeconv_train_sums_bytes(layers, nlayers, N, B));
    t->total = ws.at;
    return FX3D_OK;
}

}  // namespace

namespace fx3d {
namespace mlp {

long long edgeconv_stat_count(const int32_t *layers, int nlayers) {
    long long n = 0;
    for (int i = 1; i < nlayers; ++i) n += 2 * (long long)layers[i];
    return n;
}

size_t edgeconv_train_sums_bytes(const int32_t *layers, int nlayers, int N, int B) {
    int widest = 0;
    for (int i = 1; i < nlayers; ++i) widest = layers[i] > widest ? layers[i] : widest;
    return (size_t)2 * widest * ((N + kTile - 1) / kTile) * B * sizeof(double);
}

fx3d_status edgeconv_train_run(const float *params_dev, const int32_t *layers, int nlayers, int K, const float *x, int N, int B,
                               const int32_t *idx_in, float momentum, float *out, int32_t *idx_out, float *batch_stats, float *running,
                               void *ws, double *sums, fx3d_stream_t s, const EdgeTrainLabels &lb) {
    const int32_t *idx = nullptr;
    fx3d_status r = edgeconv_neighbours(x, layers[0], N, B, K, idx_in, idx_out, ws, s, &idx);
    if (r != FX3D_OK) return r;
    hipStream_t st = as_stream(s);
    const long long T = (long long)((N + kTile - 1) / kTile) * B;
    Conv run[kMaxLayers];  // the running statistics, read for `running` alone
    edgeconv_layout(params_dev, layers, nlayers, run);
    size_t at = 0;
    for (int l = 1; l < nlayers; ++l) {
        const int C = layers[l];
        // layers 1 .. l - 1 at their batch statistics, layer l's slabs into the sums
        const EdgePass p = edge_pass(params_dev, batch_stats, layers, l + 1, K, x, N, idx, nullptr);
        if ((r = launch_stats(p, sums, B, st, l + 1 == nlayers ? lb.stats_last : lb.stats)) != FX3D_OK) return r;
        StatOut o{};
        o.run_m = run[l - 1].bn.m; o.run_v = run[l - 1].bn.v;
        o.mu = batch_stats + at; o.var = batch_stats + at + C;
        o.new_m = running ? running + at : nullptr; o.new_v = running ? running + at + C : nullptr;
        o.mtm = momentum;
        o.m = (long long)K * N * B;
        if ((r = pointnet::launch_stat_finish(sums, C, T, o, st, lb.finish)) != FX3D_OK) return r;
        at += 2 * (size_t)C;
    }
    return edgeconv_launch(edge_pass(params_dev, batch_stats, layers, nlayers, K, x, N, idx, out), B, st, lb.closing);
}

}  // namespace mlp
}  // namespace fx3d

extern "C" {

fx3d_status fx3d_edgeconv_stat_count(const int32_t *layers, int32_t nlayers, int64_t *count) {
    const char *fn = "fx3d_edgeconv_stat_count";
    FX3D_REQUIRE(count != nullptr, "%s: count is NULL", fn);
    const fx3d_status rc = check_layers(fn, layers, nlayers);
    if (rc != FX3D_OK) return rc;
    *count = edgeconv_stat_count(layers, nlayers);
    return FX3D_OK;
}

fx3d_status fx3d_edgeconv_train_workspace_bytes(const int32_t *layers, int32_t nlayers, int32_t K, int32_t N, int32_t B,
                                                size_t *bytes) {
    const char *fn = "fx3d_edgeconv_train_workspace_bytes";
    FX3D_REQUIRE(bytes != nullptr, "%s: bytes is NULL", fn);
    fx3d_status rc = check_layers(fn, layers, nlayers);
    if (rc != FX3D_OK) return rc;
    if ((rc = check_edgeconv_sizes(fn, N, B, K)) != FX3D_OK) return rc;
    TrainPlan t;
    if ((rc = train_plan(layers, nlayers, N, B, K, &t)) != FX3D_OK) return rc;
    *bytes = t.total;
    return FX3D_OK;
}

fx3d_status fx3d_edgeconv_forward_train(const float *params_dev, const int32_t *layers, int32_t nlayers, int32_t K, const float *x,
                                        int32_t N, int32_t B, const int32_t *idx_in, float momentum, float *out, int32_t *idx_out,
                                        float *batch_stats, float *running, void *ws, size_t ws_bytes, fx3d_stream_t s) {
    const char *fn = "fx3d_edgeconv_forward_train";
    FX3D_REQUIRE(params_dev && x && out && batch_stats && ws, "%s: params_dev, x, out, batch_stats and ws must not be NULL", fn);
    fx3d_status r = check_layers(fn, layers, nlayers);
    if (r != FX3D_OK) return r;
    if ((r = check_edgeconv_sizes(fn, N, B, K)) != FX3D_OK) return r;
    FX3D_REQUIRE(std::isfinite(momentum) && momentum >= 0.0f && momentum <= 1.0f, "%s: momentum must be finite and in [0, 1], got %g",
                 fn, (double)momentum);
    TrainPlan t;
    if ((r = train_plan(layers, nlayers, N, B, K, &t)) != FX3D_OK) return r;
    FX3D_REQUIRE(ws_bytes >= t.total, "%s: workspace of %zu bytes, fx3d_edgeconv_train_workspace_bytes says %zu", fn, ws_bytes, t.total);
    FX3D_REQUIRE((reinterpret_cast<uintptr_t>(ws) & 255) == 0, "%s: ws must be 256-byte aligned", fn);
    const EdgeTrainLabels lb{"edgeconv_train_stats", "edgeconv_train_stats_last", "edgeconv_train_finish", "edgeconv_train_closing"};
    return edgeconv_train_run(params_dev, layers, nlayers, K, x, N, B, idx_in, momentum, out, idx_out, batch_stats, running, ws,
                              reinterpret_cast<double *>(static_cast<char *>(ws) + t.sums), s, lb);
}

}  // extern "C"
