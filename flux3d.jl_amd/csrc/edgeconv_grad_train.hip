// EdgeConv(layers, K) in training mode (gfx950), the adjoint: the gradients of sum(gout . out) for out = fx3d_edgeconv_forward_train(x)
// with respect to the parameters and, when asked, to x, through the batch statistics.  include/flux3d_hip.h ("EdgeConv training-mode
// adjoint") states the definition and the order of every sum; tests/edgeconv_grad_train_ref.py restates it on the host.
//
// Every BatchNorm is a cut: dbeta_l = sum gy_l and dgamma_l = sum gy_l xh_l run over all K N B edge rows and must be finished before
// gv_l = (((gy_l - mb_l) - xh_l mg_l) gamma_l) / sd_l can be formed for any row.  The (K N, C, B) arrays are still never written: a
// pass recomputes the forward tile per neighbour rank k, as the test-mode adjoints do, with the steps of edgeconv_adjoint.h in
// their training mode (TrainBn).  Per call, after the host preamble of every adjoint (edgeconv_adjoint_prepare at the statistics):
//   for l = L .. 1:
//     edgeconv_gt_sums_kernel<LD, NS> with stop = l: one block = one half-tile of 32 points of one cloud, 4 waves, the loop over k
//       of the parameter adjoint on its LDS plan (image l - 2 is alive while layer l walks back): gather_rows, hidden_fwd_chain,
//       last_compare, back_layer down to layer l with the finished means of the layers above.  At layer l nothing is written:
//       (gy_l, gy_l xh_l) is added into the Float64 pair the lane carries across k for its channel -- one chain per half-wave,
//       the 16 rows mfma_row(r, h) in ascending r.  xh_L is in the compare's accumulators; xh of a hidden layer is one more forward
//       slab from the image below (hidden_bwd).  After the last k the half-waves meet through __shfl_xor, chain(0) + chain(1), and
//       half-wave 0 stores the pair with plain stores to sums (2, C, half-tiles, B).
//     edgeconv_gt_finish_kernel: fold_tile_sums (pointnet_net.h) over t = half-tile + nhalf b, then dbeta_l, dgamma_l and +0 for the
//       mu / var slots straight into gparams, and mb_l, mg_l into the means (the statistics buffer's layout).
//   the closing pass: edgeconv_pgrad_kernel on PgradTrainArgs (edgeconv_pgrad_net.h) -- the parameter adjoint's kernel, its steps
//     writing gv_l where they wrote dz_l and its sinks contracting gv_l with a_{l-1}: H_l is dW_l and h_l is db_l, in that kernel's
//     orders; pass 0 owns the db chains and gx.  Then pgrad_reduce, unchanged, with gparams as its destination: dW and db are
//     written as they come out of the chain over (b, chunk).
// No atomics: every sum has one owner and one order.
#include "edgeconv_pgrad_net.h"
#include "pointnet_net.h"

using namespace fx3d;
using namespace fx3d::mlp;
using fx3d::mlp::pointnet::PairSum;

namespace {

// the H tiles the closing pass keeps in registers (edgeconv_pgrad_net.h: plan): what leaves the training-mode instantiation
// without scratch
constexpr int kTrainTilesNarrow = 12, kTrainTilesWide = 8;

// the wave's slab sl of the stop layer into the lane's chains: the 16 rows in ascending r
template <int NS>
__device__ __forceinline__ void add_pairs(PairSum (&ps)[NS], const f32x16 &gy, const f32x16 &xh, int sl, int wave) {
    const int s = __builtin_amdgcn_readfirstlane((sl - wave) / kWaves);  // (hidden_bwd's slab index is no scalar to the compiler)
#pragma unroll
    for (int q = 0; q < NS; ++q)
        if (s == q) {
#pragma unroll
            for (int r = 0; r < 16; ++r) ps[q].add(gy[r], xh[r]);
        }
}

// a: the chain at the batch statistics; bn.stop: the layer whose sums are wanted; sums: (2, c_stop, half-tiles, B).  STOP: 0 where
// that is layer L (no walk back), else the hidden layer itself, 1 .. 3 (a kernel each: with the stop layer known at run time only,
// the SGPR spills of the walk back left stack slots behind).
template <int LD, int NS, int STOP>
__global__ __launch_bounds__(kPtThreads) void edgeconv_gt_sums_kernel(const AdjointArgs a, const TrainBn bn, double *__restrict__ sums) {
    extern __shared__ float lds[];
    constexpr int T = 32, IMG = T * LD;
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), h = lane >> 5, j = lane & 31;
    const int b = blockIdx.y, p0 = blockIdx.x * T;
    const int nvalid = min(T, a.N - p0);
    const int F = a.w[0], L = a.nl, cout = a.cout;
    constexpr bool LAST = STOP == 0;
    const float *xb = a.x + (size_t)b * a.N * F;
    const int32_t *ib = a.idx + ((size_t)b * a.N + p0) * a.K;
    float *rows = lds;
    float *dzl = L == 1 ? lds + IMG : L == 2 ? lds + 2 * IMG : lds;  // where gv_L goes: the parameter adjoint's plan
    const Conv cl = L == 1 ? a.c[0] : L == 2 ? a.c[1] : L == 3 ? a.c[2] : a.c[3];
    const int cinl = L == 1 ? 2 * F : L == 2 ? a.w[1] : L == 3 ? a.w[2] : a.w[3];
    TrainBn m = bn;
    m.nvalid = nvalid;
    if (!LAST) m.stop = STOP;

    f32x16 tgt[NS][1], gv[NS][1];
    float dz0[NS];
    const float nan = quiet_nan();
    // the target load (each adjoint's own, edgeconv_adjoint.h says why): tgt = out where positive, else NaN; gv = gout
    {
        const size_t ob = ((size_t)b * a.N + p0) * cout;
#pragma unroll
        for (int s = 0; s < NS; ++s) {
            const int sl = wave + s * kWaves;
            dz0[s] = 0.0f;
            tgt[s][0] = gv[s][0] = f32x16{0};
            if (sl * 32 >= cout) continue;  // wave-uniform
            const int oc = min(sl * 32 + j, cout - 1);
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int p = mfma_row(r, h);
                float ov = nan, g = 0.0f;
                if (p < nvalid) {
                    ov = a.out[ob + (size_t)p * cout + oc];
                    g = a.gout[ob + (size_t)p * cout + oc];
                }
                tgt[s][0][r] = ov > 0.0f ? ov : nan;
                gv[s][0][r] = g;
            }
        }
    }
    PairSum ps[NS];
    for (int k = 0; k < a.K; ++k) {
        gather_rows<T>(rows, LD, xb, ib, F, a.N, a.K, k, p0, nvalid);
        __syncthreads();
        const float *src = hidden_fwd_chain<LD, 1>(a, lds, F, L);
        last_compare<LD, 1, NS, false>(
            src, dzl, cl, cinl, cout, wave, h, j, tgt, gv, dz0,
            [&ps, wave](int sl, const f32x16(&gy)[1], const f32x16(&xh)[1], const f32x16(&)[1]) {
                if (LAST) add_pairs<NS>(ps, gy[0], xh[0], sl, wave);
            },
            m, stat_offset(a.w, L), LAST);
        __syncthreads();
#pragma unroll
        for (int l = kMaxLayers; l >= 2; --l) {
            if (LAST || l > L || l <= STOP) continue;  // block-uniform
            back_layer<LD, 1>(
                a, lds, dzl, L, l,
                [&ps, wave](int lb, int sl, const f32x16(&gy)[1], const f32x16(&xh)[1], const f32x16(&)[1]) {
                    if (lb - 1 == STOP) add_pairs<NS>(ps, gy[0], xh[0], sl, wave);
                },
                m);
            if (l == L && L >= 3 && STOP == 1) {  // gv_L is consumed: the edge rows of this k again, for layer 1's slab
                gather_rows<T>(rows, LD, xb, ib, F, a.N, a.K, k, p0, nvalid);
                __syncthreads();
            }
        }
        // (`rows` and the images are written again after barriers that a wave reaches after these reads)
    }
    const int C = LAST ? cout : a.w[STOP];
    double *out = sums + 2 * ((size_t)b * gridDim.x + blockIdx.x) * C;
#pragma unroll
    for (int s = 0; s < NS; ++s) {
        const int o = (wave + s * kWaves) * 32 + j;
        if (o - j >= C) continue;  // wave-uniform
        const double s1 = ps[s].s1 + __shfl_xor(ps[s].s1, 32, 64), s2 = ps[s].s2 + __shfl_xor(ps[s].s2, 32, 64);
        if (h == 0 && o < C) pointnet::store_tile_sum(out, o, s1, s2);  // chain(0) + chain(1)
    }
}

// one BatchNorm's finished sums: its gamma | beta | mu | var slots of gparams and its means
struct GtFinish {
    float *dgamma, *dbeta, *zm, *zv;
    float *mb, *mg;
    long long m;  // K N B
};

__global__ __launch_bounds__(pointnet::kFinishThreads) void edgeconv_gt_finish_kernel(const double *__restrict__ sums, int C, long long T,
                                                                                     const GtFinish o) {
    pointnet::fold_tile_sums(sums, C, T, [&](int c, double s1, double s2) {
        const double dm = (double)o.m;
        o.dbeta[c] = (float)s1;
        o.dgamma[c] = (float)s2;
        o.zm[c] = 0.0f;
        o.zv[c] = 0.0f;
        o.mb[c] = (float)(s1 / dm);
        o.mg[c] = (float)(s2 / dm);
    });
}

template <int LD, int NS, int STOP>
fx3d_status launch_sums_of(const AdjointArgs &a, const TrainBn &bn, double *sums, size_t lds_bytes, int nhalf, int B, hipStream_t st) {
    const void *fn = reinterpret_cast<const void *>(&edgeconv_gt_sums_kernel<LD, NS, STOP>);
    const fx3d_status rc = ensure_dynamic_lds(fn, (int)kMaxLds, "edgeconv_gt_sums_kernel");
    if (rc != FX3D_OK) return rc;
    // (a label per stop layer: the passes differ in length, tools/edgeconv_grad_train_time.py reports each)
    ProfileScope prof(STOP == 0 ? "edgeconv_grad_train_sums_last" : STOP == 1 ? "edgeconv_grad_train_sums_1"
                      : STOP == 2 ? "edgeconv_grad_train_sums_2" : "edgeconv_grad_train_sums_3", st);
    hipLaunchKernelGGL((edgeconv_gt_sums_kernel<LD, NS, STOP>), dim3(nhalf, B), dim3(kPtThreads), lds_bytes, st, a, bn, sums);
    FX3D_LAUNCH_CHECK();
    return FX3D_OK;
}
template <int LD, int NS>
fx3d_status launch_sums(const AdjointArgs &a, const TrainBn &bn, double *sums, size_t lds_bytes, int nhalf, int B, hipStream_t st) {
    switch (bn.stop == a.nl ? 0 : bn.stop) {
        case 0: return launch_sums_of<LD, NS, 0>(a, bn, sums, lds_bytes, nhalf, B, st);
        case 1: return launch_sums_of<LD, NS, 1>(a, bn, sums, lds_bytes, nhalf, B, st);
        case 2: return launch_sums_of<LD, NS, 2>(a, bn, sums, lds_bytes, nhalf, B, st);
        default: return launch_sums_of<LD, NS, 3>(a, bn, sums, lds_bytes, nhalf, B, st);
    }
}

// the workspace: the adjoints' prefix (edgeconv_adjoint_plan, with the checks of the entry `fn`) | the chunk partials | the
// Float64 half-tile sums of the widest layer | the means
struct GtWs { AdjointWs adj; size_t part, sums, means, total; long long psize; int chunks, nhalf; };
fx3d_status gt_ws_plan(const char *fn, const int32_t *layers, int nlayers, int N, int B, int K, GtWs *w) {
    WsBump ws;
    const fx3d_status rc = edgeconv_adjoint_plan(fn, layers, nlayers, N, B, K, ws, &w->adj);
    if (rc != FX3D_OK) return rc;
    w->psize = edgeconv_layout(nullptr, layers, nlayers, nullptr);
    w->chunks = (N + kGradChunk - 1) / kGradChunk;
    w->nhalf = (N + 31) / 32;
    int widest = 0;
    long long nstat = 0;
    for (int i = 1; i < nlayers; ++i) {
        widest = layers[i] > widest ? layers[i] : widest;
        nstat += 2 * (long long)layers[i];
    }
    w->part = ws.put((size_t)w->psize * w->chunks * B * sizeof(float));
    w->sums = ws.put((size_t)2 * widest * w->nhalf * B * sizeof(double));
    w->means = ws.put((size_t)nstat * sizeof(float));
    w->total = ws.at;
    return FX3D_OK;
}

}  // namespace

extern "C" {

fx3d_status fx3d_edgeconv_grad_train_workspace_bytes(const int32_t *layers, int32_t nlayers, int32_t K, int32_t N, int32_t B,
                                                     size_t *bytes) {
    const char *fn = "fx3d_edgeconv_grad_train_workspace_bytes";
    FX3D_REQUIRE(bytes != nullptr, "%s: bytes is NULL", fn);
    GtWs w;
    const fx3d_status rc = gt_ws_plan(fn, layers, nlayers, N, B, K, &w);
    if (rc != FX3D_OK) return rc;
    *bytes = w.total;
    return FX3D_OK;
}

fx3d_status fx3d_edgeconv_grad_train(const float *params_dev, const int32_t *layers, int32_t nlayers, int32_t K, const float *x,
                                     int32_t N, int32_t B, const int32_t *idx, const float *out, const float *batch_stats,
                                     const float *gout, float *gparams, float *gx, void *ws, size_t ws_bytes, fx3d_stream_t s) {
    const char *fn = "fx3d_edgeconv_grad_train";
    FX3D_REQUIRE(params_dev && x && batch_stats && gout && gparams && ws,
                 "%s: params_dev, x, batch_stats, gout, gparams and ws must not be NULL", fn);
    GtWs w;
    PgradTrainArgs a{};
    FinishArgs f{};
    fx3d_status r = gt_ws_plan(fn, layers, nlayers, N, B, K, &w);
    if (r != FX3D_OK) return r;
    if ((r = edgeconv_adjoint_prepare(fn, "fx3d_edgeconv_grad_train_workspace_bytes", w.adj, w.total, params_dev, layers, nlayers, K, x,
                                      N, B, idx, out, gout, gx, ws, ws_bytes, s, &a, batch_stats)) != FX3D_OK) return r;
    char *wsb = static_cast<char *>(ws);
    hipStream_t st = as_stream(s);
    const int L = nlayers - 1;
    const Plan p = plan(layers, nlayers, kTrainTilesNarrow, kTrainTilesWide);
    WsPlan pw{};
    pw.part = w.part; pw.sums = w.part; pw.psize = w.psize; pw.chunks = w.chunks;
    pgrad_fill(params_dev, layers, nlayers, pw, p, B, ws, &a, &f);
    double *sums = reinterpret_cast<double *>(wsb + w.sums);
    float *means = reinterpret_cast<float *>(wsb + w.means);
    a.bn.means = means;

    // the sums passes, from layer L down, each finished before the next
    size_t at = 0;
    for (int l = 1; l < L; ++l) at += 2 * (size_t)layers[l];
    for (int l = L; l >= 1; --l) {
        const int C = layers[l];
        TrainBn bn = a.bn;
        bn.stop = l;
        switch (p.ld) {
            case 66: r = launch_sums<66, 1>(a, bn, sums, p.lds_bytes, w.nhalf, B, st); break;
            case kLd: r = launch_sums<kLd, 1>(a, bn, sums, p.lds_bytes, w.nhalf, B, st); break;
            default: r = launch_sums<258, 2>(a, bn, sums, p.lds_bytes, w.nhalf, B, st); break;
        }
        if (r != FX3D_OK) return r;
        GtFinish o{};
        float *g = gparams + (a.c[l - 1].bn.g - params_dev);  // gamma | beta | mu | var, C each
        o.dgamma = g; o.dbeta = g + C; o.zm = g + 2 * (size_t)C; o.zv = g + 3 * (size_t)C;
        o.mb = means + at; o.mg = means + at + C;
        o.m = (long long)K * N * B;
        {
            ProfileScope prof("edgeconv_grad_train_finish", st);
            hipLaunchKernelGGL(edgeconv_gt_finish_kernel, dim3((C + pointnet::kFinishChannels - 1) / pointnet::kFinishChannels),
                               dim3(pointnet::kFinishThreads), 0, st, sums, C, (long long)w.nhalf * B, o);
            FX3D_LAUNCH_CHECK();
        }
        if (l > 1) at -= 2 * (size_t)layers[l - 1];
    }

    // the closing pass: dW and db (and gx), then the chain over the chunks straight into gparams
    const char *label = "edgeconv_grad_train_closing";
    switch (p.ld) {
        case 66: r = launch_pgrad<66, 1, kTrainTilesNarrow>(a, p, w.chunks, B, st, label); break;
        case kLd: r = launch_pgrad<kLd, 1, kTrainTilesNarrow>(a, p, w.chunks, B, st, label); break;
        default: r = launch_pgrad<258, 2, kTrainTilesWide>(a, p, w.chunks, B, st, label); break;
    }
    if (r != FX3D_OK) return r;
    f.sums = gparams;
    ProfileScope prof("edgeconv_grad_train_reduce", st);
    return launch_pgrad_reduce(f, st);
}

}  // extern "C"
