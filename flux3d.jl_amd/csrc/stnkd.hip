// stnKD(K) as a layer in its own right (gfx950): src/models/pointnet.jl:3-20 in test mode and in training mode, for every
// 1 <= K <= 128.  include/flux3d_hip_layers.h states the layer, its arithmetic and the parameter layout; this file is the host walk.
//
// The layer is one round of PointNet (pointnet_net.h): round_trunk's MODE 3 is MODE 0's layer chain with the input width at run
// time -- the tile of x (K, N, B) in columns 0 .. K - 1 of an image, the first convolution on mfma_slab_rt (the MFMA over the first
// 4 floor(K / 4) channels, v_fma_f32 on the same accumulators for the rest: no padding), then the 64 -> 128 and 128 -> 1024 calls
// MODE 0 makes -- and the head is pointnet_head_kernel<false>, which takes K and K K as arguments.  So the kernels are
// pointnet.hip's (pointnet_points_kernel<3>, the head) and, in training mode, pointnet_train.hip's (pointnet_stats_kernel<3, L>, the
// finishing kernels and the heads cut at the dense BatchNorm); what is here is the parameter walk (layout_stn, so the stn.* and
// fstn.* slices of a PointNet buffer are stnKD(3) and stnKD(64) buffers), the workspace, the refusals, and the optional pooled
// feature, which the transform heads do not write: one small kernel folds the per-tile maxima again.
#include "flux3d_hip_layers.h"
#include "pointnet_net.h"

using namespace fx3d;
using namespace fx3d::mlp;
using namespace fx3d::mlp::pointnet;

namespace {

constexpr int kMaxK = FX3D_STNKD_MAX_K;  // the image's columns
static_assert(kMaxK <= kLd - 2, "the tile's K channels are one row of an image");
constexpr int kWidth[4] = {64, 128, kFeat, 256};  // bn1 .. bn4
static_assert(2 * (kWidth[0] + kWidth[1] + kWidth[2] + kWidth[3]) == FX3D_STNKD_STAT_COUNT, "the statistics layout");

// pooled (1024, B): thread c folds channel c of the cloud's per-tile maxima, as the head's first phase does
__global__ __launch_bounds__(kHeadThreads) void stnkd_pool_kernel(const float *__restrict__ tmax, int ntiles, float *__restrict__ pooled) {
    pooled[(size_t)blockIdx.x * kFeat + threadIdx.x] = fold_tile_maxima(tmax, ntiles, blockIdx.x);
}

// the workspace: per-tile maxima (1024, ntiles, B); training mode: | the tile sums of the widest layer | relu(dense2) (256, B)
struct Plan { size_t tmax, sums, a2, total; int ntiles; };
Plan plan(int N, int B, bool train) {
    Plan p{};
    p.ntiles = (N + kTile - 1) / kTile;
    WsBump ws;
    p.tmax = ws.put((size_t)kFeat * p.ntiles * B * sizeof(float));
    if (train) {
        p.sums = ws.put((size_t)2 * kFeat * p.ntiles * B * sizeof(double));
        p.a2 = ws.put((size_t)256 * B * sizeof(float));
    }
    p.total = ws.at;
    return p;
}

fx3d_status check_k(const char *fn, int32_t K) {
    if (K < 1 || K > kMaxK) {
        set_error("%s: K must be in [1, %d] (the tile's K channels are one row of an LDS image), got %d", fn, kMaxK, K);
        return FX3D_ERR_UNSUPPORTED;
    }
    return FX3D_OK;
}

fx3d_status check_stn_sizes(const char *fn, int32_t K, int32_t N, int32_t B, bool train) {
    const fx3d_status rc = check_k(fn, K);
    if (rc != FX3D_OK) return rc;
    FX3D_REQUIRE(N >= 1 && B >= 1, "%s: N and B must be positive, got N=%d B=%d", fn, N, B);
    FX3D_REQUIRE(B <= 65535, "%s: B must be at most 65535, got %d", fn, B);
    FX3D_REQUIRE((long long)N * B <= (1ll << 31), "%s: N * B must be at most 2^31, got %lld", fn, (long long)N * B);
    FX3D_REQUIRE(!train || B >= 2, "%s: training-mode BatchNorm needs B >= 2 clouds (the dense BatchNorm's running variance divides by B - 1), got %d",
                 fn, B);
    return FX3D_OK;
}

fx3d_status check_ws(const char *fn, const char *query, const void *ws, size_t ws_bytes, size_t need) {
    FX3D_REQUIRE(ws_bytes >= need, "%s: workspace of %zu bytes, %s says %zu", fn, ws_bytes, query, need);
    FX3D_REQUIRE((reinterpret_cast<uintptr_t>(ws) & 15) == 0, "%s: ws must be 16-byte aligned", fn);
    return FX3D_OK;
}

Stn stn_layout(const float *params, int K, long long *count) {
    Cursor c{params, 0};
    const Stn s = layout_stn(c, K);
    if (count) *count = c.at;
    return s;
}

PointArgs point_args(const Stn &s, int K, const float *x, int N, const Plan &p, float *tmax) {
    PointArgs a{};
    a.x = x; a.K = K; a.c1 = s.c1; a.c2 = s.c2; a.c3 = s.c3;
    a.tmax = tmax; a.N = N; a.ntiles = p.ntiles;
    return a;
}

// the head's arguments: the (K, K) matrix goes straight to the caller's array
HeadArgs head_args(const Stn &s, int K, const float *tmax, int ntiles, float *out) {
    HeadArgs h{};
    h.tmax = tmax; h.ntiles = ntiles;
    h.d1 = s.d1; h.d2 = s.d2; h.d3 = s.d3; h.bn2 = s.bn;
    h.n3 = K * K; h.K = K; h.mat = out;
    return h;
}

fx3d_status launch_pool(const float *tmax, int ntiles, float *pooled, int B, hipStream_t st) {
    ProfileScope prof("stnkd_pool", st);
    hipLaunchKernelGGL(stnkd_pool_kernel, dim3(B), dim3(kHeadThreads), 0, st, tmax, ntiles, pooled);
    FX3D_LAUNCH_CHECK();
    return FX3D_OK;
}

}  // namespace

extern "C" {

fx3d_status fx3d_stnkd_param_count(int32_t K, int64_t *count) {
    FX3D_REQUIRE(count != nullptr, "fx3d_stnkd_param_count: count is NULL");
    const fx3d_status rc = check_k("fx3d_stnkd_param_count", K);
    if (rc != FX3D_OK) return rc;
    long long n = 0;
    stn_layout(nullptr, K, &n);
    *count = n;
    return FX3D_OK;
}

fx3d_status fx3d_stnkd_workspace_bytes(int32_t N, int32_t B, int32_t K, size_t *bytes) {
    FX3D_REQUIRE(bytes != nullptr, "fx3d_stnkd_workspace_bytes: bytes is NULL");
    const fx3d_status rc = check_stn_sizes("fx3d_stnkd_workspace_bytes", K, N, B, false);
    if (rc != FX3D_OK) return rc;
    *bytes = plan(N, B, false).total;
    return FX3D_OK;
}

fx3d_status fx3d_stnkd_train_workspace_bytes(int32_t N, int32_t B, int32_t K, size_t *bytes) {
    FX3D_REQUIRE(bytes != nullptr, "fx3d_stnkd_train_workspace_bytes: bytes is NULL");
    const fx3d_status rc = check_stn_sizes("fx3d_stnkd_train_workspace_bytes", K, N, B, true);
    if (rc != FX3D_OK) return rc;
    *bytes = plan(N, B, true).total;
    return FX3D_OK;
}

fx3d_status fx3d_stnkd_forward(const float *params_dev, int32_t K, const float *x, int32_t N, int32_t B, float *out, float *pooled,
                               void *ws, size_t ws_bytes, fx3d_stream_t s) {
    const char *fn = "fx3d_stnkd_forward";
    FX3D_REQUIRE(params_dev && x && out && ws, "%s: params_dev, x, out and ws must not be NULL", fn);
    fx3d_status r = check_stn_sizes(fn, K, N, B, false);
    if (r != FX3D_OK) return r;
    const Plan p = plan(N, B, false);
    if ((r = check_ws(fn, "fx3d_stnkd_workspace_bytes", ws, ws_bytes, p.total)) != FX3D_OK) return r;
    const Stn net = stn_layout(params_dev, K, nullptr);
    hipStream_t st = as_stream(s);
    float *tmax = WsView{static_cast<char *>(ws)}.f32(p.tmax);
    if ((r = launch_points(3, false, point_args(net, K, x, N, p, tmax), B, st)) != FX3D_OK) return r;
    if (pooled && (r = launch_pool(tmax, p.ntiles, pooled, B, st)) != FX3D_OK) return r;
    return launch_head(false, head_args(net, K, tmax, p.ntiles, out), B, st);
}

fx3d_status fx3d_stnkd_forward_train(const float *params_dev, int32_t K, const float *x, int32_t N, int32_t B, float momentum,
                                     float *out, float *pooled, float *batch_stats, float *running, void *ws, size_t ws_bytes,
                                     fx3d_stream_t s) {
    const char *fn = "fx3d_stnkd_forward_train";
    FX3D_REQUIRE(params_dev && x && out && batch_stats && ws, "%s: params_dev, x, out, batch_stats and ws must not be NULL", fn);
    fx3d_status r = check_stn_sizes(fn, K, N, B, true);
    if (r != FX3D_OK) return r;
    FX3D_REQUIRE(std::isfinite(momentum) && momentum >= 0.0f && momentum <= 1.0f, "%s: momentum must be finite and in [0, 1], got %g",
                 fn, (double)momentum);
    const Plan p = plan(N, B, true);
    if ((r = check_ws(fn, "fx3d_stnkd_train_workspace_bytes", ws, ws_bytes, p.total)) != FX3D_OK) return r;
    const Stn run = stn_layout(params_dev, K, nullptr);  // the running statistics, read for `running` alone
    Stn net = run;                                   // the layer at the batch statistics
    Bn *bns[4] = {&net.c1.bn, &net.c2.bn, &net.c3.bn, &net.bn};
    const Bn *runs[4] = {&run.c1.bn, &run.c2.bn, &run.c3.bn, &run.bn};
    StatOut so[4];
    size_t at = 0;
    for (int i = 0; i < 4; ++i) {
        const int C = kWidth[i];
        bns[i]->m = batch_stats + at;
        bns[i]->v = batch_stats + at + C;
        so[i].run_m = runs[i]->m; so[i].run_v = runs[i]->v;
        so[i].mu = batch_stats + at; so[i].var = batch_stats + at + C;
        so[i].new_m = running ? running + at : nullptr; so[i].new_v = running ? running + at + C : nullptr;
        so[i].mtm = momentum;
        so[i].m = i < 3 ? (long long)N * B : B;
        at += 2 * (size_t)C;
    }
    hipStream_t st = as_stream(s);
    const WsView v{static_cast<char *>(ws)};
    float *tmax = v.f32(p.tmax);
    StatArgs sa{};
    sa.p = point_args(net, K, x, N, p, tmax);
    sa.sums = v.f64(p.sums);
    // the three point BatchNorms in order, each a statistics pass over the layers below it, then the full pass
    for (int L = 0; L < 3; ++L) {
        if ((r = launch_stats(3, L, sa, B, st)) != FX3D_OK) return r;
        if ((r = launch_stat_finish(sa.sums, kWidth[L], (long long)p.ntiles * B, so[L], st, "stnkd_train_finish")) != FX3D_OK) return r;
    }
    if ((r = launch_points(3, false, sa.p, B, st)) != FX3D_OK) return r;
    if (pooled && (r = launch_pool(tmax, p.ntiles, pooled, B, st)) != FX3D_OK) return r;
    // the head up to relu(dense2), the dense BatchNorm's statistics over the clouds, the head's end
    TrainHeadArgs t{};
    t.h = head_args(net, K, tmax, p.ntiles, out);
    t.a2 = v.f32(p.a2);
    if ((r = launch_train_head(0, false, t, B, st)) != FX3D_OK) return r;
    if ((r = launch_dense_stats(t.a2, kWidth[3], B, so[3], st, "stnkd_train_dense_stats")) != FX3D_OK) return r;
    return launch_train_head(2, false, t, B, st);
}

}  // extern "C"
